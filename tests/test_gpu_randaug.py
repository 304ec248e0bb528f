"""RandAugment on the device (csrc/randaug.hip, vtx/aug.py) against torchvision's arithmetic restated on the CPU
(tests/randaug_ref.py): the warp equal to F.grid_sample outside rounding ties of the coordinate, every other op bit for bit.

Clips are [3,2,H,W,3] with planted frames (randaug_ref.planted_clip) at 40x56 (2240 pixels: the 32-bit path) and 33x47 (1551
pixels, odd rows: the byte path, and stencil / warp edges that are no multiple of anything)."""
import numpy as np
import pytest
import torch

import aug_ref as A
import randaug_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = ['40x56', '33x47']
_clips = {}


def _clip(hw):
    """The planted clip of a shape, built once and never written."""
    if hw not in _clips:
        _clips[hw] = R.planted_clip(hw, seed=41 + hw[0])
    return _clips[hw]


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _f32(x):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64).float().to(DEV)


SELS = [[1, 1, 0], [0, 1, 1], [1, 0, 1]]          # every clip is processed twice and left alone once, beside processed ones


@pytest.mark.parametrize('hw', R.SHAPES, ids=IDS)
def test_warp_equals_grid_sample_outside_ties(hw):
    """Every geometric op in both signs: equal to the reference outside near_tie, one of the candidate source pixels inside;
    the clip with sel == 0 (and a matrix that would empty it) is copied bit for bit in the same launch."""
    from vtx import ops
    clip = _clip(hw)
    dev = clip.to(DEV)
    far = [1.0, 0.0, 1e9, 0.0, 1.0, 0.0]
    for n, (op, mag) in enumerate(R.signed_cases(hw)):
        m = R.matrix_of(op, mag, hw)
        sel = SELS[n % 3]
        got = ops.clip_warp_nearest_u8(dev, _f32([m if s else far for s in sel]), _i32(sel))
        torch.cuda.synchronize()
        assert got.data_ptr() != dev.data_ptr() and got.shape == dev.shape and got.dtype == torch.uint8
        got = got.cpu()
        tie = R.near_tie(*R.warp_coords64(m, hw))
        print(f'{R.OPS[op]} {mag:+.4f} on {hw}: tie share {tie.mean():.4f}')
        assert tie.mean() <= R.TIE_SHARE
        for b, s in enumerate(sel):
            if not s:
                assert torch.equal(got[b], clip[b])
                continue
            want = R.warp_grid_sample(clip[b], m).numpy()
            same = np.all(got[b].numpy() == want, axis=(0, 3))
            print(f'  clip {b}: {int((~same).sum())} pixels differ from grid_sample, {int((~same & ~tie).sum())} of them outside ties')
            assert np.all(same | tie)
            assert np.all(R.warp_matches(got[b].numpy(), clip[b], m))


@pytest.mark.parametrize('hw', R.SHAPES, ids=IDS)
def test_warp_identity_and_far_translation(hw):
    """An identity theta reproduces the clip bit for bit, and so does sel == 0; a translation far out of the frame gives zeros."""
    from vtx import ops
    clip = _clip(hw)
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    got = ops.clip_warp_nearest_u8(clip.to(DEV), _f32([ident, [1.0, 0.0, -3e9, 0.0, 1.0, 3e9], ident]), _i32([1, 1, 0])).cpu()
    assert torch.equal(got[0], clip[0]) and torch.equal(got[2], clip[2])
    assert int(got[1].max()) == 0
    out = torch.empty_like(clip, device=DEV)
    assert ops.clip_warp_nearest_u8(clip.to(DEV), _f32([ident] * 3), _i32([0, 0, 0]), out=out) is out
    assert torch.equal(out.cpu(), clip)


@pytest.mark.parametrize('hw', R.SHAPES, ids=IDS)
def test_sharpness_is_bit_identical(hw):
    """Both signs of the magnitude on every frame (flat 0 / 255 frames and the one-pixel border included), beside a clip that
    is copied."""
    from vtx import ops
    clip = _clip(hw)
    dev = clip.to(DEV)
    m = R.magnitudes(hw)[9]
    for n, sel in enumerate(SELS):
        fac = [1.0 + m, 1.0 - m, 1.0 + m] if n % 2 == 0 else [1.0 - m, 1.0 + m, 1.0 - m]
        got = ops.clip_sharpness_u8(dev, _f32([[r, 1.0 - r] for r in fac]), _i32(sel)).cpu()
        for b, s in enumerate(sel):
            want = R.sharpness(clip[b], fac[b]) if s else clip[b]
            assert torch.equal(got[b], want), f'sel {sel} clip {b} factor {fac[b]}: {int((got[b] != want).sum())} bytes differ'
    # the blend is computed on the border too: some border byte moves, as it does in the restatement
    want = R.sharpness(clip[2], 1.0 + m)
    assert (want[:, 0] != clip[2][:, 0]).any()
    # frames of two rows are returned as they are
    thin = clip[:, :, :2].contiguous()
    got = ops.clip_sharpness_u8(thin.to(DEV), _f32([[1.0 + m, -m]] * 3), _i32([1, 1, 1])).cpu()
    assert torch.equal(got, thin)


@pytest.mark.parametrize('hw', R.SHAPES, ids=IDS)
def test_posterize_and_solarize_are_bit_identical(hw):
    from vtx import ops
    clip = _clip(hw)
    recs = [[1, 7], [2, 179], [0, 0]]
    for shift in range(3):
        rec = recs[shift:] + recs[:shift]
        dev = clip.to(DEV)
        got = ops.clip_pointwise_u8_(dev, _i32(rec))
        assert got.data_ptr() == dev.data_ptr()
        got = got.cpu()
        for b, (op, arg) in enumerate(rec):
            want = clip[b] if op == 0 else R.posterize(clip[b], arg) if op == 1 else R.solarize(clip[b], 178.5)
            assert torch.equal(got[b], want), f'clip {b} op {op}'
    # other arguments: 4 bits, 0 bits, 8 bits; thresholds 0 (all inverted) and 256 (none)
    dev = clip.to(DEV)
    got = ops.clip_pointwise_u8_(dev, _i32([[1, 4], [1, 8], [2, 0]])).cpu()
    assert torch.equal(got[0], clip[0] & 0xF0) and torch.equal(got[1], clip[1]) and torch.equal(got[2], 255 - clip[2])
    got = ops.clip_pointwise_u8_(clip.to(DEV), _i32([[2, 256], [1, 0], [3, 5]])).cpu()
    assert torch.equal(got[0], clip[0]) and int(got[1].max()) == 0 and torch.equal(got[2], clip[2])


@pytest.mark.parametrize('hw', R.SHAPES, ids=IDS)
def test_autocontrast_is_bit_identical(hw):
    """Planted: flat frames (every channel hi == lo), values 100 .. 110 only, one constant channel beside two that stretch."""
    from vtx import ops
    clip = _clip(hw)
    want = [R.autocontrast(clip[b]) for b in range(3)]
    assert torch.equal(want[2][0, :, :, 1], clip[2, 0, :, :, 1]) and not torch.equal(want[0][1], clip[0, 1])
    assert int(want[0][1].min()) == 0 and int(want[0][1].max()) == 255
    for sel in SELS:
        got = ops.clip_autocontrast_u8_(clip.to(DEV), _i32(sel)).cpu()
        for b, s in enumerate(sel):
            assert torch.equal(got[b], want[b] if s else clip[b]), f'sel {sel} clip {b}'


@pytest.mark.parametrize('hw', R.SHAPES, ids=IDS)
def test_equalize_is_bit_identical(hw):
    """Planted: flat frames and the frame that is 255 but for 200 pixels (step == 0: unchanged), values 100 .. 110 only."""
    from vtx import ops
    clip = _clip(hw)
    want = [R.equalize(clip[b]) for b in range(3)]
    assert torch.equal(want[1][0], clip[1, 0]) and not torch.equal(want[0][1], clip[0, 1]) and not torch.equal(want[2][1], clip[2, 1])
    for sel in SELS:
        got = ops.clip_equalize_u8_(clip.to(DEV), _i32(sel)).cpu()
        for b, s in enumerate(sel):
            assert torch.equal(got[b], want[b] if s else clip[b]), f'sel {sel} clip {b}'


def _chain(base, rec, hw):
    """Reference op -> op on uint8 [T,H,W,3]; -> (expected, the input of the last op if that op is geometric else None)."""
    x, before = base, None
    for i, (op, mag) in enumerate(rec):
        before = x if op in R.GEOMETRIC and i == len(rec) - 1 else None
        x = R.apply_op(x, op, mag)
    return x, before


def test_clip_augment_with_auto_augment_end_to_end():
    """ClipAugment(img_size=32, auto_augment=...) with hand-built params: all 14 ops across the two slots, the same op twice in
    one clip, a one-op and an empty record.  Expected = the resampler's reference (identity-sized crop boxes with and without
    flip, which resample exactly) -> op -> op; exact, except where a geometric op comes last: there the tie rule of the warp
    applies.  Geometric ops in the first slot are shears and translations, whose 32x32 coordinates have no near tie."""
    from vtx import aug
    hw, out = A.SRC_HW, (32, 32)
    mag = R.magnitudes(out)
    recs = [((0, 0.0), (13, 0.0)),
            ((1, mag[1]), (9, -mag[9])),
            ((6, mag[6]), (2, -mag[2])),
            ((3, -mag[3]), (7, -mag[7])),
            ((8, mag[8]), (4, mag[4])),
            ((10, mag[10]), (5, mag[5])),
            ((11, mag[11]), (12, 0.0)),
            ((9, mag[9]), (9, mag[9])),
            ((2, mag[2]), (5, -mag[5])),
            ((7, mag[7]), (8, -mag[8])),
            ((4, -mag[4]), (1, -mag[1])),
            ((6, -mag[6]),),
            ()]
    assert {op for r in recs for op, _ in r} == set(range(14))
    B = len(recs)
    clip = A.source_clip(B, 2, hw, seed=51)
    boxes = [(b % 9, (3 * b) % 25, 32, 32) for b in range(B)]
    params = [aug.ClipDraw(t, l, h, w, b % 2 == 1, (), (), recs[b]) for b, (t, l, h, w) in enumerate(boxes)]
    a = aug.ClipAugment(img_size=32, auto_augment='rand-m9-mstd0.5-inc1')
    got = a(clip.to(DEV), params=params)
    torch.cuda.synchronize()
    assert got.shape == (B, 2, 32, 32, 3) and got.dtype == torch.uint8 and got.is_cuda
    got = got.cpu()
    for b, rec in enumerate(recs):
        base = A.torch_resized_crop(clip[b], boxes[b], out, 'bicubic', False, flip=params[b].flip)
        for i, (op, m) in enumerate(rec[:-1]):
            if op in R.GEOMETRIC:
                assert op != 5 and not R.near_tie(*R.warp_coords64(R.matrix_of(op, m, out), out)).any()
        want, before = _chain(base, rec, out)
        if before is None:
            assert torch.equal(got[b], want), f'clip {b} {rec}: {int((got[b] != want).sum())} bytes differ'
        else:
            op, m = rec[-1]
            mat = R.matrix_of(op, m, out)
            tie = R.near_tie(*R.warp_coords64(mat, out))
            assert tie.mean() <= R.TIE_SHARE
            same = np.all(got[b].numpy() == want.numpy(), axis=(0, 3))
            assert np.all(same | tie) and np.all(R.warp_matches(got[b].numpy(), before, mat)), f'clip {b} {rec}'
    # a crop that does resample: the device resampler's own output -> op -> op
    params2 = [params[b]._replace(top=2, left=5, height=30, width=41) for b in (1, 6, 7)]
    sub = clip[[1, 6, 7]].to(DEV)
    plain = a(sub, params=[p._replace(randaug=()) for p in params2]).cpu()
    got2 = a(sub, params=params2).cpu()
    for i, p in enumerate(params2):
        assert torch.equal(got2[i], _chain(plain[i], p.randaug, out)[0])


def test_clip_augment_draws_under_a_generator():
    """params=None: the draws are sample_params(auto_augment=..., out_hw=...) under the generator; reproducible; the colour jitter
    is not applied beside RandAugment."""
    from vtx import aug
    clip = A.source_clip(6, 2, A.SRC_HW, seed=52).to(DEV)
    a = aug.ClipAugment(img_size=32, auto_augment=True)
    x = a(clip, generator=torch.Generator().manual_seed(13))
    y = a(clip, generator=torch.Generator().manual_seed(13))
    z = a(clip, generator=torch.Generator().manual_seed(14))
    assert x.shape == (6, 2, 32, 32, 3) and x.dtype == torch.uint8 and x.is_cuda
    assert torch.equal(x, y) and not torch.equal(x, z)
    draws = aug.sample_params(6, A.SRC_HW, generator=torch.Generator().manual_seed(13), auto_augment=True, out_hw=(32, 32))
    assert all(len(d.randaug) == 2 and d.ops == () for d in draws)
    assert torch.equal(x, a(clip, params=draws))
    # without auto_augment the call is what it was: the colour-jitter draws
    j = aug.ClipAugment(img_size=32)
    jd = aug.sample_params(6, A.SRC_HW, generator=torch.Generator().manual_seed(13))
    assert all(len(d.ops) == 3 and d.randaug == () for d in jd)
    assert torch.equal(j(clip, generator=torch.Generator().manual_seed(13)), j(clip, params=jd))


def test_bad_arguments_raise_before_any_launch():
    from vtx import aug, ops
    classes = ('clip_resample', 'clip_jitter', 'clip_warp', 'clip_sharpness', 'clip_pointwise', 'clip_autocontrast', 'clip_equalize')
    cpu = torch.zeros(2, 2, 8, 8, 3, dtype=torch.uint8)
    dev = cpu.to(DEV)
    theta, fac, sel, pw = _f32([[1, 0, 0, 0, 1, 0]] * 2), _f32([[1.0, 0.0]] * 2), _i32([1, 1]), _i32([[1, 7], [2, 179]])
    a = aug.ClipAugment(img_size=8, auto_augment=True)
    box = aug.ClipDraw(0, 0, 8, 8, False, (), ())
    ops.profile_start(classes)
    try:
        for call in (lambda: ops.clip_warp_nearest_u8(cpu, theta, sel), lambda: ops.clip_sharpness_u8(cpu, fac, sel),
                     lambda: ops.clip_pointwise_u8_(cpu, pw), lambda: ops.clip_autocontrast_u8_(cpu, sel),
                     lambda: ops.clip_equalize_u8_(cpu, sel), lambda: a(cpu),
                     lambda: ops.clip_warp_nearest_u8(dev, theta.cpu(), sel), lambda: ops.clip_equalize_u8_(dev, sel.cpu())):
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                call()
        for call in (lambda: ops.clip_warp_nearest_u8(dev.float(), theta, sel), lambda: ops.clip_sharpness_u8(dev.float(), fac, sel),
                     lambda: ops.clip_pointwise_u8_(dev.int(), pw), lambda: ops.clip_autocontrast_u8_(dev.float(), sel),
                     lambda: ops.clip_equalize_u8_(dev[..., :2], sel), lambda: a(dev.float()),
                     lambda: ops.clip_warp_nearest_u8(dev, theta.double(), sel), lambda: ops.clip_warp_nearest_u8(dev, theta, sel.long()),
                     lambda: ops.clip_warp_nearest_u8(dev, theta[:1], sel), lambda: ops.clip_sharpness_u8(dev, theta, sel),
                     lambda: ops.clip_pointwise_u8_(dev, sel), lambda: ops.clip_autocontrast_u8_(dev, fac),
                     lambda: ops.clip_equalize_u8_(dev, pw), lambda: ops.clip_warp_nearest_u8(dev, theta, sel, out=dev.float())):
            with pytest.raises(TypeError):
                call()
        for call in (lambda: ops.clip_warp_nearest_u8(dev, theta, sel, out=dev), lambda: ops.clip_sharpness_u8(dev, fac, sel, out=dev),
                     lambda: a(dev, params=[box._replace(randaug=((14, 0.0),)), box]),
                     lambda: a(dev, params=[box, box._replace(randaug=((1, float('nan')),))]),
                     lambda: a(dev, params=[box._replace(randaug=((1, 0.1), (2, 0.1), (3, 1.0))), box])):
            with pytest.raises(ValueError):
                call()
        torch.cuda.synchronize()
    finally:
        launched = ops.profile_stop()
    assert launched == {c: {} for c in classes}
