"""bench.py's contract on one GPU: a plain run times exactly --steps steps and prints the headline line only (the instrumented
pass, other configurations and CPU baseline are --full's); --dump-outputs writes the last timed step's outputs as float32 .npy,
the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ('gemm_shapes', 'gemm_tn_roofline', 'roofline_hbm', 'instrumented_step_ms', 'other_configs', 'cpu_baseline')


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '2',
           '--dump-outputs', str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_bench_run_and_its_output_dump(tmp_path):
    line = _bench(tmp_path / 'a')
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0
    assert line['unit'] == 'clips/s' and line['higher_is_better'] is True and line['dtype'] == 'bf16'
    assert abs(line['value'] - 2 / (line['ms_per_step'] * 1e-3)) < 0.01 * line['value']
    assert not set(FULL_ONLY) & set(line), set(FULL_ONLY) & set(line)
    dumps = {}
    for name in ('loss', 'logits', 'params_sample', 'grads_sample'):
        a = np.load(str(tmp_path / 'a' / (name + '.npy')))
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
        dumps[name] = a
    assert dumps['logits'].shape == (2, 400) and dumps['loss'].shape == (1,)
    assert abs(float(dumps['loss'][0]) - line['final_loss']) < 1e-3
    assert dumps['params_sample'].shape == dumps['grads_sample'].shape and np.abs(dumps['grads_sample']).max() > 0
    assert sum(os.path.getsize(str(tmp_path / 'a' / f)) for f in os.listdir(str(tmp_path / 'a'))) < 64 << 20
    again = _bench(tmp_path / 'b')                      # same arguments, same inputs: the same logits (to summation order)
    assert abs(again['final_loss'] - line['final_loss']) < 1e-3
    logits = np.load(str(tmp_path / 'b' / 'logits.npy'))
    assert np.abs(logits - dumps['logits']).max() <= 1e-3 * np.abs(dumps['logits']).max()
