"""Pin the oracle restatement against the reference: what the UNMODIFIED reference models computed on these inputs (same
synthetic weights and clips, same seeds) is recorded in tests/golden/oracle_pin.npz by tests/golden/make_golden_pin.py, together
with each model's state-dict shapes; the oracle runs live here and must reproduce it."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLD, relerr
from oracle import synth, vt_oracle as O

SM = dict(img_size=64, patch_size=16, embed_dims=128, num_heads=2, num_transformer_layers=3)
TSF_ATTN = ['divided_space_time', 'space_only', 'joint_space_time']
VIVIT_ATTN = ['fact_encoder', 'joint_space_time', 'divided_space_time']
RES_ATTN = ['divided_space_time', 'space_only']
RES_HW = [(96, 96), (64, 96), (96, 64), (32, 32)]

_gold = None


def gold(key):
    global _gold
    if _gold is None:
        _gold = dict(np.load(os.path.join(GOLD, 'oracle_pin.npz'), allow_pickle=False))
    return _gold[key]


def shapes(model_key):
    """{state-dict key: shape} of the reference model the record was made with (the weights are synthesised from it)."""
    return {k: tuple(v) for k, v in json.loads(str(gold(model_key + '.shapes'))).items()}


def ref(key):
    return torch.from_numpy(gold(key))


@pytest.mark.parametrize('at', TSF_ATTN)
@pytest.mark.parametrize('train', [False, True])
def test_timesformer(at, train):
    sd = synth.synth_state_dict(shapes(f'tsf4.{at}'), 1)
    x = synth.synth_clip(2, 4, 3, 64, 64)
    torch.manual_seed(5)
    yo = O.timesformer_forward(sd, x, 4, heads=2, layers=3, attention_type=at, training=train)
    assert relerr(yo, ref(f'tsf4.{at}.train{int(train)}.out')) < 1e-5
    ao = O.timesformer_forward(sd, x, 4, heads=2, layers=3, attention_type=at, return_attention=True)
    assert relerr(ao, ref(f'tsf4.{at}.train{int(train)}.attn')) < 1e-5


@pytest.mark.parametrize('at', VIVIT_ATTN)
def test_vivit(at):
    sd = synth.synth_state_dict(shapes(f'vivit8.{at}'), 2)
    x = synth.synth_clip(3, 8, 3, 64, 64)
    torch.manual_seed(7)
    yo = O.vivit_forward(sd, x, 8, heads=2, layers=3, attention_type=at, training=True)
    assert relerr(yo, ref(f'vivit8.{at}.out')) < 1e-5


@pytest.mark.parametrize('hw', RES_HW)
@pytest.mark.parametrize('at', RES_ATTN)
def test_timesformer_other_resolution(at, hw):
    """Clips of another resolution than img_size go through interpolate_pos_encoding (reference video_transformer.py:171-191,
    :209): bicubic resize of the positional table, with the reference's width / height quirk for non-square clips."""
    sd = synth.synth_state_dict(shapes(f'tsf2.{at}'), 6)
    x = synth.synth_clip(2, 2, 3, hw[0], hw[1])
    yo = O.timesformer_forward(sd, x, 2, heads=2, layers=3, attention_type=at)
    assert relerr(yo, ref(f'tsf2.{at}.{hw[0]}x{hw[1]}.out')) < 1e-5
    po = O.interpolated_pos_embed(sd['pos_embed'], (hw[0] // 16) * (hw[1] // 16), hw[1], hw[0], 16)
    assert torch.equal(ref(f'tsf2.{at}.{hw[0]}x{hw[1]}.pos_embed'), po)


def test_droppath_rng_stream():
    """one training forward of TimeSformer-B (B=2,T=2) makes 33 torch.rand calls
    (layer 0 draws nothing); the oracle must consume the generator identically: the next draws after the reference's
    forward are recorded."""
    sd = synth.synth_state_dict(shapes('droppath'), 1)
    x = synth.synth_clip(2, 2, 3, 64, 64)
    torch.manual_seed(3)
    O.timesformer_forward(sd, x, 2, heads=2, layers=3, training=True)
    assert torch.equal(ref('droppath.rand_after'), torch.rand(4))
