"""Boundary b1: the REFERENCE's own Lightning module (model_trainer.py, unmodified, with pytorch_lightning / torchmetrics / timm /
torchvision stubbed exactly as absent packages) builds its model, head, Mixup, loss and optimizer ON TOP OF the drop-in
transformer.py / video_transformer.py / optimizer.py / mixup.py / utils.py of this package -- i.e. the reference's entry point
accepts the drop-in files.  What it imported and built there is recorded in tests/golden/host_reference.json
(tests/golden/make_golden_host.py); these tests hold the drop-in modules, and the drop-in model_trainer.py, to that record.
(Its training_step needs a GPU; the same step is driven on the device through the drop-in model_trainer.py in
tests/test_gpu_trainer.py.)"""
import hashlib
import importlib
import json
import os
import types
import warnings

import numpy as np
import pytest

from helpers import GOLD


def _record():
    return json.load(open(os.path.join(GOLD, 'host_reference.json')))


def rng_digest():
    return hashlib.sha256(np.ascontiguousarray(np.random.get_state()[1], dtype='<u4').tobytes()).hexdigest()


def trainer_outcome(MT, arch, attention_type, cfg, max_epochs):
    """What VideoTransformer(cfg) of the Lightning-module file MT builds (also what make_golden_host.py records)."""
    cfg = types.SimpleNamespace(arch=arch, attention_type=attention_type, **cfg)
    trainer = types.SimpleNamespace(max_epochs=max_epochs, current_epoch=0)
    m = MT.VideoTransformer(cfg, trainer, ckpt_dir='.', do_eval=True, do_test=False)
    opts, scheds = m.configure_optimizers()
    lrs = []
    with warnings.catch_warnings():                     # stepping the schedule without an optimizer step is the point here
        warnings.simplefilter('ignore', UserWarning)
        for _ in range(max_epochs):
            lrs.append([g['lr'] for g in opts[0].param_groups])
            scheds[0].step()
    assert m.no_weight_decay_keywords() == m.model.no_weight_decay_keywords()
    return {'model': type(m.model).__name__, 'head_out_features': m.cls_head.cls_head.out_features,
            'optimizer': type(opts[0]).__name__,
            'param_groups': [[len(g['params']), g['weight_decay']] for g in opts[0].param_groups],
            'lr_per_epoch': lrs, 'no_weight_decay_keywords': sorted(m.no_weight_decay_keywords())}


@pytest.mark.parametrize('arch', ['timesformer', 'vivit'])
def test_reference_lightning_module_builds_on_the_drop_in_modules(arch):
    """Every name the reference's model_trainer.py imports from the package exists in the drop-in module and is the object the
    drop-in model_trainer.py uses; the drop-in Lightning module, given the recorded configuration, builds what the reference's
    built on the drop-in modules: same model / head / optimizer classes, parameter groups, schedule and keywords."""
    import model_trainer as MT
    import transformer
    import video_transformer
    rec = _record()['trainer']
    for module, name in rec['imports']:
        mod = importlib.import_module(module)
        if name is not None:
            assert hasattr(mod, name), (module, name)
            assert getattr(MT, name) is getattr(mod, name), (module, name)
    assert MT.TimeSformer is video_transformer.TimeSformer and MT.ClassificationHead is transformer.ClassificationHead
    want = dict(rec['archs'][arch])
    got = trainer_outcome(MT, arch, want.pop('attention_type'), rec['cfg'], rec['max_epochs'])
    assert got['model'] == ('TimeSformer' if arch == 'timesformer' else 'ViViT')
    assert got['head_out_features'] == rec['cfg']['num_class'] == 174
    assert got['optimizer'] == 'FusedAdamW' and len(got['param_groups']) == 2
    assert got == want


def test_drop_in_mixup_plans_a_batch_like_the_reference_draw_for_draw():
    """The host half of mixup.Mixup (``draw``) against the reference's class under the same numpy seed, as recorded: same
    lambda, same CutMix box, same generator state afterwards (reference mixup.py:74-88,:105-109).  The device half is proven
    equal to the reference's tensor formulas in tests/test_gpu_head.py; this package has no CPU tensor path."""
    import mixup as ours
    rec = _record()['mixup']
    shape = tuple(rec['shape'])
    kinds = set()
    assert len(rec['plans']) == 40
    for plan in rec['plans']:
        kw, seed = plan['kwargs'], plan['seed']
        np.random.seed(seed)
        lam_o, box_o = ours.Mixup(num_classes=rec['num_classes'], **kw).draw(shape)
        assert rng_digest() == plan['rng_sha256'], (kw, seed)
        assert float(lam_o) == plan['lam'], (kw, seed)
        assert (box_o is None) == (plan['box'] is None) and (box_o is None or list(box_o) == plan['box']), (kw, seed)
        kinds.add(box_o is not None)
    assert kinds == {True, False}, 'both kinds of plan must have been exercised'
