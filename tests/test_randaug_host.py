"""RandAugment, host side (no GPU): the C ABI of libvtx_randaug.so (include/vtx_randaug.h), the draws of vtx.aug.sample_randaug
and of sample_params(auto_augment=...), and the float64 form of the warp against torch's own F.grid_sample."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import aug_ref as A
import randaug_ref as R


def test_randaug_library_header_and_binding_agree():
    """include/vtx_randaug.h, vtx/_lib.py RANDAUG_SIGNATURES and the export list of libvtx_randaug.so name the same symbols; none of
    them is declared in include/vtx.h or include/vtx_aug.h; the header compiles as C99."""
    import __graft_entry__ as ge
    from helpers import ROOT
    from vtx import _lib
    ge.ensure_built()

    def declared(header):
        src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        return sorted(set(re.findall(r'\b(vtx_[a-z0-9_]+)\s*\(', src)))
    names = declared('vtx_randaug.h')
    assert names == sorted(_lib.RANDAUG_SIGNATURES) and len(names) == 9
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.RANDAUG_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('vtx_')) == names
    assert not set(names) & set(declared('vtx.h'))
    assert not set(names) & set(declared('vtx_aug.h'))
    assert _lib.load_randaug().vtx_randaug_version() >= 100
    subprocess.run(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', os.path.join(ROOT, 'include', 'vtx_randaug.h')], check=True)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Null device pointers, non-positive sizes, a short workspace and src == dst: VTX_EINVAL (-1) with a reason, on a machine
    without a GPU -- nothing was launched."""
    from vtx import _lib
    lib = _lib.load_randaug()
    p = 4096                                                   # never dereferenced on the host
    assert lib.vtx_clip_warp_nearest_u8(1, 1, 8, 8, None, None, None, None, None) == -1
    assert b'null pointer' in lib.vtx_randaug_last_error_string()
    assert lib.vtx_clip_warp_nearest_u8(1, 1, 8, 8, p, p, p, p, None) == -1
    assert b'in place' in lib.vtx_randaug_last_error_string()
    assert lib.vtx_clip_warp_nearest_u8(0, 1, 8, 8, p, 2 * p, p, p, None) == -1
    assert b'positive' in lib.vtx_randaug_last_error_string()
    assert lib.vtx_clip_warp_nearest_u8(1, 1, 8, -8, p, 2 * p, p, p, None) == -1
    assert lib.vtx_clip_sharpness_u8(1, 1, 8, 8, None, None, None, None, None) == -1
    assert lib.vtx_clip_sharpness_u8(1, 1, 8, 8, p, p, p, p, None) == -1
    assert lib.vtx_clip_sharpness_u8(1, 0, 8, 8, p, 2 * p, p, p, None) == -1
    assert lib.vtx_clip_pointwise_u8(1, 1, 8, 8, None, None, None) == -1
    assert lib.vtx_clip_pointwise_u8(1, 1, 0, 8, p, p, None) == -1
    assert lib.vtx_clip_autocontrast_workspace(3, 2) == 3 * 2 * 3 * 2 * 4
    assert lib.vtx_clip_equalize_workspace(3, 2) == 3 * 2 * 3 * 256 * 4
    assert lib.vtx_clip_autocontrast_workspace(0, 2) == 0 and lib.vtx_clip_equalize_workspace(3, -1) == 0
    assert lib.vtx_clip_autocontrast_u8(1, 1, 8, 8, None, None, None, 0, None) == -1
    assert lib.vtx_clip_autocontrast_u8(3, 2, 8, 8, p, p, p, 143, None) == -1
    assert b'workspace' in lib.vtx_randaug_last_error_string()
    assert lib.vtx_clip_autocontrast_u8(3, 2, 8, 0, p, p, p, 144, None) == -1
    assert lib.vtx_clip_equalize_u8(1, 1, 8, 8, None, None, None, 0, None) == -1
    assert lib.vtx_clip_equalize_u8(3, 2, 8, 8, p, p, p, 18431, None) == -1
    assert b'workspace' in lib.vtx_randaug_last_error_string()
    assert lib.vtx_clip_equalize_u8(-3, 2, 8, 8, p, p, p, 18432, None) == -1
    assert lib.vtx_clip_equalize_u8(70000, 1, 8, 8, p, p, p, 1 << 30, None) == -1          # more frames than the grid holds


def test_sample_randaug_draws():
    from vtx import aug
    hw = (224, 224)
    a = aug.sample_randaug(256, hw, generator=torch.Generator().manual_seed(3))
    b = aug.sample_randaug(256, hw, generator=torch.Generator().manual_seed(3))
    c = aug.sample_randaug(256, hw, generator=torch.Generator().manual_seed(4))
    assert a == b and a != c and len(a) == 256
    assert aug.RANDAUG_OPS == R.OPS
    lin = lambda lo, hi: float(torch.linspace(lo, hi, 31)[9])
    table = {0: 0.0, 1: lin(0, 0.3), 2: lin(0, 0.3), 3: lin(0, 150.0 / 331.0 * 224), 4: lin(0, 150.0 / 331.0 * 224), 5: lin(0, 30.0),
             6: lin(0, 0.9), 7: lin(0, 0.9), 8: lin(0, 0.9), 9: lin(0, 0.9), 10: 7.0, 11: 178.5, 12: 0.0, 13: 0.0}
    assert table[10] == 8 - round(9 / 7.5) and table[11] == lin(255.0, 0.0) and abs(table[5] - 9.0) < 1e-5
    seen = set()
    for rec in a:                                              # 512 draws
        assert len(rec) == 2
        for op, mag in rec:
            assert 0 <= op < 14 and isinstance(op, int) and isinstance(mag, float)
            assert abs(mag) == table[op]
            if op not in R.SIGNED:
                assert mag >= 0
            seen.add((op, mag < 0))
    assert {op for op, _ in seen} == set(range(14))
    assert all((op, True) in seen and (op, False) in seen for op in R.SIGNED)
    # what the kernels are handed: TranslateX on 224 columns is +-30 pixels, Posterize keeps 7 bits, Solarize inverts from 179
    assert int(table[3]) == 30 and int(-table[3]) == -30
    plan = aug._randaug_plan([aug.ClipDraw(0, 0, 8, 8, False, (), (), ((10, table[10]), (11, table[11]))),
                              aug.ClipDraw(0, 0, 8, 8, False, (), (), ((3, -table[3]), (0, 0.0)))], 224, 224)
    assert [k for k, _ in plan] == ['warp', 'pointwise', 'pointwise']
    theta, sel = plan[0][1]
    assert sel.tolist() == [0, 1] and theta[1].tolist() == [1.0, 0.0, 30.0, 0.0, 1.0, 0.0] and theta[0].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert plan[1][1][0].tolist() == [[1, 7], [0, 0]] and plan[2][1][0].tolist() == [[2, 179], [0, 0]]
    # magnitudes follow the frame size and the bin
    m = aug.sample_randaug(64, (40, 56), generator=torch.Generator().manual_seed(3))
    assert {abs(mag) for rec in m for op, mag in rec if op == 3} == {float(torch.linspace(0, 150.0 / 331.0 * 56, 31)[9])}
    assert {abs(mag) for rec in m for op, mag in rec if op == 4} == {float(torch.linspace(0, 150.0 / 331.0 * 40, 31)[9])}
    assert all(len(rec) == 3 for rec in aug.sample_randaug(4, hw, num_ops=3, generator=torch.Generator().manual_seed(1)))
    with pytest.raises(ValueError):
        aug.sample_randaug(1, hw, magnitude=31)


def test_unsigned_ops_consume_no_sign_draw():
    """The generator after sample_randaug equals a generator advanced by a hand count of the draws: one randint(14) per op and
    one randint(2) more for each signed op only."""
    from vtx import aug
    g = torch.Generator().manual_seed(12)
    recs = aug.sample_randaug(40, (32, 32), generator=g)
    h = torch.Generator().manual_seed(12)
    signed = unsigned = 0
    for rec in recs:
        for op, mag in rec:
            assert int(torch.randint(14, (1,), generator=h)) == op
            if op in R.SIGNED:
                signed += 1
                assert bool(torch.randint(2, (1,), generator=h)) == (mag < 0)
            else:
                unsigned += 1
    assert signed + unsigned == 80 and signed > 20 and unsigned > 10
    assert torch.equal(g.get_state(), h.get_state())
    assert int(torch.randint(1 << 30, (1,), generator=g)) == int(torch.randint(1 << 30, (1,), generator=h))


#: sample_params(..., generator=manual_seed(5)) / (..., scale=(0.5, 1.0), color_jitter=None, generator=manual_seed(7)) on 40x56
#: frames, recorded at the commit before ``auto_augment`` existed
PARENT_DRAWS = [(8, 22, 21, 24, False, (2, 0, 1), (1.3847415447235107, 1.1720045804977417, 1.0634620189666748)),
                (9, 8, 31, 23, True, (1, 0, 2), (0.7329080700874329, 0.9124770164489746, 0.8108927607536316)),
                (5, 26, 16, 16, False, (2, 1, 0), (0.6397561430931091, 0.8872010111808777, 1.0654997825622559))]
PARENT_DRAWS_MIM = [(2, 8, 38, 36, True, (), ()), (2, 0, 37, 36, True, (), ())]


def test_sample_params_without_auto_augment_is_unchanged():
    from vtx import aug
    d = aug.sample_params(3, (40, 56), generator=torch.Generator().manual_seed(5))
    assert [tuple(x)[:7] for x in d] == PARENT_DRAWS and all(x.randaug == () for x in d)
    d = aug.sample_params(3, (40, 56), generator=torch.Generator().manual_seed(5), auto_augment=None, out_hw=(32, 32))
    assert [tuple(x)[:7] for x in d] == PARENT_DRAWS and all(x.randaug == () for x in d)
    d = aug.sample_params(2, (40, 56), scale=(0.5, 1.0), color_jitter=None, generator=torch.Generator().manual_seed(7))
    assert [tuple(x)[:7] for x in d] == PARENT_DRAWS_MIM
    # seven positional fields still construct a record
    box = aug.ClipDraw(0, 0, 40, 56, False, (), ())
    assert box.randaug == () and len(box) == 8
    assert aug.ClipDraw(0, 0, 40, 56, False, (1,), (1.2,), ((0, 0.0),)).randaug == ((0, 0.0),)


def test_sample_params_with_auto_augment_draws_crop_flip_randaug():
    """Clip by clip: the crop box, the flip coin, then RandAugment's draws for the OUTPUT size; no ColorJitter draw is made."""
    from vtx import aug
    hw, out = (40, 56), (32, 32)
    g = torch.Generator().manual_seed(8)
    d = aug.sample_params(6, hw, generator=g, auto_augment='rand-m9-mstd0.5-inc1', out_hw=out)
    h = torch.Generator().manual_seed(8)
    mags = R.magnitudes(out)
    for x in d:
        assert (x.top, x.left, x.height, x.width) == aug._crop_box(hw[0], hw[1], (0.08, 1.0), (3. / 4., 4. / 3.), h)
        assert x.flip == bool(float(torch.rand(1, generator=h)) < 0.5)
        assert x.ops == () and x.factors == () and len(x.randaug) == 2
        for op, mag in x.randaug:
            assert int(torch.randint(14, (1,), generator=h)) == op
            sign = -1.0 if op in R.SIGNED and int(torch.randint(2, (1,), generator=h)) else 1.0
            assert mag == sign * mags[op]
    assert torch.equal(g.get_state(), h.get_state())
    with pytest.raises(ValueError, match='out_hw'):
        aug.sample_params(1, hw, auto_augment=True)
    # any truthy value selects the same defaults
    e = aug.sample_params(6, hw, generator=torch.Generator().manual_seed(8), auto_augment=True, out_hw=out)
    assert e == d


def test_check_draws_validates_randaug_records():
    from vtx import aug
    box = aug.ClipDraw(0, 0, 40, 56, False, (), ())
    aug._check_draws([box._replace(randaug=((13, 0.0), (0, 0.0)))], 1, 40, 56)
    for bad in (((14, 0.0),), ((-1, 0.0),), ((1, float('nan')),), ((1, float('inf')),), ((1.5, 0.0),), ((1, 0.1), (2, 0.1), (3, 1.0)), ((1,),)):
        with pytest.raises(ValueError, match='RandAugment'):
            aug._check_draws([box._replace(randaug=bad)], 1, 40, 56)
    with pytest.raises(ValueError, match='RandAugment'):
        aug._check_draws([box._replace(ops=(0,), factors=(1.1,), randaug=((1, 0.1),))], 1, 40, 56)


@pytest.mark.parametrize('hw', R.SHAPES, ids=['40x56', '33x47'])
def test_float64_warp_form_agrees_with_grid_sample(hw):
    """The ten signed geometric cases: source pixel at (rint sx, rint sy) of the float64 coordinate = torch's float32 affine grid +
    F.grid_sample, outside near_tie; at most 2 % of the pixels are near a tie (the condition the GPU test relies on); the matrix
    vtx.aug hands the kernel is the restated one."""
    from vtx import aug
    frames = A.source_clip(1, 2, hw, seed=31)[0]
    frames[0] = torch.randint(1, 256, frames[0].shape, generator=torch.Generator().manual_seed(32), dtype=torch.uint8)
    for op, mag in R.signed_cases(hw):
        m = R.matrix_of(op, mag, hw)
        assert aug.randaug_theta(op, mag, hw[0], hw[1]) == m
        want = R.warp_grid_sample(frames, m).numpy()
        got = R.warp_float64(frames, m)
        tie = R.near_tie(*R.warp_coords64(m, hw))
        same = np.all(got == want, axis=(0, 3))
        print(f'{R.OPS[op]} {mag:+.4f} on {hw}: tie share {tie.mean():.4f}, pixels off outside ties {int((~same & ~tie).sum())}')
        assert tie.mean() <= R.TIE_SHARE
        assert np.all(same | tie)
        assert np.all(R.warp_matches(want, frames, m))
        assert (want != frames.numpy()).any()                  # the case does move pixels
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert np.array_equal(R.warp_float64(frames, ident), frames.numpy()) and torch.equal(R.warp_grid_sample(frames, ident), frames)


def test_reference_ops_on_known_values():
    """The restatement itself on values worked by hand."""
    f = torch.tensor([0, 100, 127, 128, 178, 179, 255], dtype=torch.uint8).view(1, 1, 7, 1).expand(1, 1, 7, 3).contiguous()
    assert R.posterize(f, 7)[0, 0, :, 0].tolist() == [0, 100, 126, 128, 178, 178, 254]
    assert R.solarize(f, 178.5)[0, 0, :, 0].tolist() == [0, 100, 127, 128, 178, 76, 0]
    ramp = torch.arange(100, 111, dtype=torch.uint8).view(1, 1, 11, 1).expand(1, 3, 11, 3).contiguous()
    ac = R.autocontrast(ramp)
    assert ac[0, 0, :, 0].tolist() == [int(np.float32(i) * (np.float32(255.0) / np.float32(10.0))) for i in range(11)]
    flat = torch.full((1, 4, 5, 3), 9, dtype=torch.uint8)
    assert torch.equal(R.autocontrast(flat), flat) and torch.equal(R.equalize(flat), flat)
    assert torch.equal(R.sharpness(flat[:, :2], 0.73), flat[:, :2])                    # two rows: returned as it is
    # equalize of 256 values, 255 pixels behind the last bin's one: step 1, lut[i] = i
    allv = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()
    assert torch.equal(R.equalize(allv), allv)
    assert math.ceil(178.5) == 179
