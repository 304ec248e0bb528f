"""Clip augmentation, host side (no GPU): the resampling tables of vtx_resample_build_table against torch's own
F.interpolate, the draws of vtx.aug.sample_params, and the C ABI of libvtx_aug.so (include/vtx_aug.h)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import aug_ref as R


def test_aug_library_header_and_binding_agree():
    """include/vtx_aug.h, vtx/_lib.py AUG_SIGNATURES and the export list of libvtx_aug.so name the same symbols; the library
    leaves libvtx.so alone: none of its symbols is declared in include/vtx.h."""
    import __graft_entry__ as ge
    from helpers import ROOT
    from vtx import _lib
    ge.ensure_built()

    def declared(header):
        src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        return sorted(set(re.findall(r'\b(vtx_[a-z0-9_]+)\s*\(', src)))
    names = declared('vtx_aug.h')
    assert names == sorted(_lib.AUG_SIGNATURES) and len(names) == 7
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.AUG_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('vtx_')) == names
    assert not set(names) & set(declared('vtx.h'))
    lib = _lib.load_aug()
    assert lib.vtx_aug_version() >= 100
    # the header compiles as plain C
    subprocess.run(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', os.path.join(ROOT, 'include', 'vtx_aug.h')], check=True)


def _tables(box, mode, antialias, flip=False):
    from vtx import ops
    top, left, h, w = box
    ytab = ops.resample_table(R.SRC_HW[0], top, h, R.OUT_HW[0], mode, antialias)
    xtab = ops.resample_table(R.SRC_HW[1], left, w, R.OUT_HW[1], mode, antialias, flip=flip)
    return ytab, xtab


@pytest.mark.parametrize('box', R.BOXES, ids=['down', 'up', 'identity'])
@pytest.mark.parametrize('mode,antialias', R.MODES)
def test_tables_reproduce_interpolate(mode, antialias, box):
    """float64 evaluation of the tables vs CPU F.interpolate of the cropped float image: <= 2e-4 (torch's own float32 evaluation
    measured 8.4e-5 at worst on these shapes); identity box = the crop, exactly; the flipped x table = the result reversed in x."""
    frames = R.source_clip(1, 2, R.SRC_HW, seed=11)[0]
    ytab, xtab = _tables(box, mode, antialias)
    got = R.table_eval(frames.numpy(), ytab, xtab)
    want = R.torch_resize_float(frames, box, R.OUT_HW, mode, antialias).double().numpy()
    err = np.abs(got - want).max()
    print(f'{mode} antialias={antialias} box={box}: max |table - interpolate| = {err:.3e}')
    assert err <= 2e-4
    if box == R.BOXES[2]:
        top, left, h, w = box
        assert np.array_equal(got, frames[:, top:top + h, left:left + w].double().numpy())
        for tab in (ytab, xtab):
            assert np.all(tab[1] == 1) and np.all(tab[2][:, 0] == np.float32(1.0))
    _, xflip = _tables(box, mode, antialias, flip=True)
    assert np.array_equal(R.table_eval(frames.numpy(), ytab, xflip), got[:, :, ::-1])
    # after rounding: torch's uint8 result, except where the value sits on a rounding tie
    u8 = R.torch_resized_crop(frames, box, R.OUT_HW, mode, antialias).numpy()
    mine = np.rint(np.clip(got, 0, 255)).astype(np.uint8)
    assert np.all((mine == u8) | R.near_tie(got))


@pytest.mark.parametrize('mode,antialias', R.MODES)
def test_weight_rows_and_windows(mode, antialias):
    """Rows sum to 1 within 1e-6, tap windows lie inside the crop, vtx_resample_max_taps is never exceeded, entries behind
    the count are not written."""
    from vtx import _lib, ops
    for src_len, start, length, out_len in [(56, 0, 56, 32), (56, 7, 12, 32), (56, 4, 32, 32), (40, 5, 9, 32), (340, 13, 300, 224),
                                            (57, 1, 55, 32), (7, 3, 1, 5), (1080, 0, 1080, 224)]:
        taps = ops.resample_max_taps(length, out_len, mode, antialias)
        first = np.zeros(out_len, np.int32)
        count = np.zeros(out_len, np.int32)
        weights = np.full((out_len, taps + 2), np.float32(77.0))
        _lib.aug_call('vtx_resample_build_table', src_len, start, length, out_len, ops.RESAMPLE_MODES[mode], int(antialias), 0, taps + 2,
                 first.ctypes.data, count.ctypes.data, weights.ctypes.data)
        assert count.min() >= 1 and count.max() <= taps
        assert first.min() >= start and (first + count).max() <= start + length
        for o in range(out_len):
            assert abs(float(weights[o, :count[o]].astype(np.float64).sum()) - 1.0) <= 1e-6
            assert np.all(weights[o, count[o]:] == np.float32(77.0))
    if antialias:
        assert ops.resample_max_taps(56, 32, mode, True) > 4          # the downscale of the GPU cases has more than 4 taps
        assert ops.resample_table(56, 0, 56, 32, mode, True)[1].max() > (4 if mode == 'bicubic' else 2)


def test_build_table_rejects_bad_arguments():
    from vtx import _lib
    lib = _lib.load_aug()
    first = (ctypes.c_int32 * 8)()
    count = (ctypes.c_int32 * 8)()
    w = (ctypes.c_float * 64)()
    ok = lambda *a: lib.vtx_resample_build_table(*a, first, count, w)
    assert ok(16, 0, 16, 8, 1, 0, 0, 4) == 0
    assert ok(16, 9, 8, 8, 1, 0, 0, 4) == -1                 # crop runs over the end
    assert b'does not lie inside' in lib.vtx_aug_last_error_string()
    assert ok(16, -1, 8, 8, 1, 0, 0, 4) == -1
    assert ok(16, 0, 16, 8, 2, 0, 0, 4) == -1                # unknown mode
    assert ok(16, 0, 16, 8, 1, 0, 0, 3) == -1                # max_taps too small
    assert ok(16, 0, 16, 8, 1, 1, 0, 4) == -1                # ... for the antialiased table
    assert lib.vtx_resample_build_table(16, 0, 16, 8, 1, 0, 0, 4, None, count, w) == -1
    assert lib.vtx_resample_max_taps(0, 8, 1, 0) == -1
    assert lib.vtx_resample_max_taps(16, 8, 1, 1) == 9       # support 2 * 2 = 4 -> 2 * 4 + 1
    assert lib.vtx_clip_jitter_workspace(3, 2) == 24
    # the device entry points check their arguments before any launch
    assert lib.vtx_clip_resample_u8(1, 1, 8, 8, 4, 4, None, None, None, None, None, 4, None, None, None, 4, None) == -1
    assert lib.vtx_clip_jitter_u8(1, 1, 8, 8, None, None, None, None, 0, None) == -1


def test_sample_params_draws():
    from vtx import aug
    hw = (40, 56)
    a = aug.sample_params(64, hw, generator=torch.Generator().manual_seed(5))
    b = aug.sample_params(64, hw, generator=torch.Generator().manual_seed(5))
    c = aug.sample_params(64, hw, generator=torch.Generator().manual_seed(6))
    assert a == b and a != c
    assert len(a) == 64                                       # one record per clip
    area = hw[0] * hw[1]
    flips = 0
    orders = set()
    for d in a:
        assert 0 <= d.top and d.top + d.height <= hw[0] and 0 <= d.left and d.left + d.width <= hw[1]
        assert d.height > 0 and d.width > 0
        # the box is the rounded (sqrt(area * ratio), sqrt(area / ratio)): half a pixel per side
        assert 0.08 * area - (d.height + d.width) / 2 - 1 <= d.height * d.width <= area
        assert (d.width - 0.5) / (d.height + 0.5) <= 4. / 3. + 1e-6 and (d.width + 0.5) / (d.height - 0.5) >= 3. / 4. - 1e-6
        assert sorted(d.ops) == [0, 1, 2] and len(d.factors) == 3          # a permutation of the three ops
        assert all(0.6 <= f <= 1.4 for f in d.factors)
        flips += d.flip
        orders.add(d.ops)
    assert 12 <= flips <= 52                                  # a fair coin: 64 draws, > 5 sigma
    assert len(orders) == 6                                   # every order turns up in 64 draws
    # the mim branch: scale (0.5, 1), no colour jitter; hflip = 0: no coin
    m = aug.sample_params(32, hw, scale=(0.5, 1.0), color_jitter=None, hflip=0., generator=torch.Generator().manual_seed(5))
    for d in m:
        assert d.ops == () and d.factors == () and d.flip is False
        assert d.height * d.width >= 0.5 * area - (d.height + d.width) / 2 - 1
    # an impossible ratio range: ten failed tries, then the centre crop with the ratio clamped (40x56: 1.4 < 20 -> full width)
    # (width = sqrt(area share * ratio) >= sqrt(0.08 * 2240 * 20) = 59.9 > 56: no try can succeed)
    for d in aug.sample_params(4, hw, ratio=(20., 40.), generator=torch.Generator().manual_seed(5)):
        assert (d.top, d.left, d.height, d.width) == ((40 - 3) // 2, 0, 3, 56)
    for d in aug.sample_params(4, hw, ratio=(0.05, 0.1), generator=torch.Generator().manual_seed(5)):
        assert (d.top, d.left, d.height, d.width) == (0, (56 - 4) // 2, 40, 4)
    # a per-op tuple; zero switches an op off; hue is not built
    for d in aug.sample_params(8, hw, color_jitter=(0.4, 0.0, 0.2), generator=torch.Generator().manual_seed(5)):
        assert sorted(d.ops) == [0, 2]
        assert 0.8 <= d.factors[d.ops.index(2)] <= 1.2
    with pytest.raises(NotImplementedError):
        aug.sample_params(1, hw, color_jitter=(0.4, 0.4, 0.4, 0.1))


def test_sample_params_follows_torchvision_draw_order():
    """One clip's draws, restated by hand against the same generator: area, log-ratio, box corner (RandomResizedCrop.get_params),
    the flip coin, then randperm(4) and the brightness / contrast / saturation factors (ColorJitter.get_params)."""
    from vtx import aug
    hw = (40, 56)
    d = aug.sample_params(1, hw, scale=(0.5, 1.0), generator=torch.Generator().manual_seed(21))[0]
    g = torch.Generator().manual_seed(21)
    while True:
        ta = hw[0] * hw[1] * torch.empty(1).uniform_(0.5, 1.0, generator=g).item()
        lr = torch.log(torch.tensor([3. / 4., 4. / 3.]))
        ar = torch.exp(torch.empty(1).uniform_(float(lr[0]), float(lr[1]), generator=g)).item()
        w, h = int(round(math.sqrt(ta * ar))), int(round(math.sqrt(ta / ar)))
        if 0 < w <= hw[1] and 0 < h <= hw[0]:
            top = torch.randint(0, hw[0] - h + 1, size=(1,), generator=g).item()
            left = torch.randint(0, hw[1] - w + 1, size=(1,), generator=g).item()
            break
    assert (d.top, d.left, d.height, d.width) == (top, left, h, w)
    assert d.flip == bool(torch.rand(1, generator=g) < 0.5)
    order = [i for i in torch.randperm(4, generator=g).tolist() if i < 3]
    fac = [float(torch.empty(1).uniform_(0.6, 1.4, generator=g)) for _ in range(3)]
    assert list(d.ops) == order and list(d.factors) == [fac[i] for i in order]


def test_cpu_clips_and_bad_shapes_raise():
    from vtx import aug
    a = aug.ClipAugment(img_size=32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        a(torch.zeros(1, 2, 40, 56, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        aug.ClipEval(img_size=32)(torch.zeros(1, 2, 40, 56, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        aug.ClipAugment(interpolation='lanczos')
    e = aug.ClipEval(img_size=224)
    assert e.scale_size == 256 and e.resized_hw(240, 320) == (256, 341) and e.resized_hw(320, 240) == (341, 256)
