"""Clip augmentation on the device (csrc/aug.hip, vtx/aug.py): the resampler against a float64 evaluation of its own tables,
the colour jitter bit for bit against torchvision's arithmetic restated on the CPU, and the path into the models."""
import itertools

import numpy as np
import pytest
import torch

import aug_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _stack_tables(specs, mode, antialias):
    """specs: per clip (src_len, start, length, out_len, flip) -> host tables per clip and the stacked device triple.  One spare
    column of NaN behind the widest window: a kernel that read past a count would show it."""
    from vtx import ops
    taps = max(ops.resample_max_taps(s[2], s[3], mode, antialias) for s in specs) + 1
    host = []
    for s in specs:
        f, c, w = ops.resample_table(s[0], s[1], s[2], s[3], mode, antialias, flip=s[4], max_taps=taps)
        for o in range(len(f)):
            w[o, c[o]:] = np.nan
        host.append((f, c, w))
    dev = tuple(torch.from_numpy(np.stack([h[i] for h in host])).to(DEV) for i in range(3))
    return host, dev


def _check_resample(src, boxes, flips, out_hw, mode, antialias):
    """Every byte = rint(clip(float64 table evaluation)); +-1 only within R.TIE of a rounding tie, and such pixels are at most
    R.TIE_SHARE of the case.  -> (device result, float64 values)."""
    from vtx import ops
    B, T, Hs, Ws, _ = src.shape
    xhost, xdev = _stack_tables([(Ws, b[1], b[3], out_hw[1], f) for b, f in zip(boxes, flips)], mode, antialias)
    yhost, ydev = _stack_tables([(Hs, b[0], b[2], out_hw[0], False) for b in boxes], mode, antialias)
    got = ops.clip_resample_u8(src.to(DEV), out_hw, xdev, ydev)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == (B, T, out_hw[0], out_hw[1], 3) and got.dtype == np.uint8
    v64 = np.stack([R.table_eval(src[b].numpy(), yhost[b], xhost[b]) for b in range(B)])
    want = np.rint(np.clip(v64, 0.0, 255.0))
    tie = R.near_tie(v64)
    diff = np.abs(got.astype(np.float64) - want)
    print(f'{mode} antialias={antialias} {Hs}x{Ws}->{out_hw}: tie share {tie.mean():.4f}, bytes off {int((diff > 0).sum())}, max diff {diff.max():.0f}')
    assert tie.mean() <= R.TIE_SHARE
    assert np.all((diff == 0) | (tie & (diff <= 1)))
    return got, v64


@pytest.mark.parametrize('mode,antialias', R.MODES)
def test_resample_matches_float64_tables(mode, antialias):
    src = R.source_clip(3, 2, R.SRC_HW, seed=3)
    got, _ = _check_resample(src, R.BOXES, [False, True, False], R.OUT_HW, mode, antialias)
    top, left, h, w = R.BOXES[2]
    assert np.array_equal(got[2], src[2, :, top:top + h, left:left + w].numpy())      # identity: the crop, bit for bit
    assert np.all(got[0, 0] == 0) and np.all(got[1, 1] == 255)                        # clamp / bicubic overshoot on flat frames


@pytest.mark.parametrize('mode,antialias', R.MODES)
def test_resample_other_shapes(mode, antialias):
    """A row length that is no multiple of 4 bytes or pixels with one-frame clips and a last row band that is not full; a frame
    wider than one column tile of the kernel."""
    src = R.source_clip(2, 1, (40, 57), seed=4)
    got, _ = _check_resample(src, [(0, 0, 40, 57), (2, 3, 31, 50)], [False, True], (29, 33), mode, antialias)
    assert np.all(got[0, 0] == 0)
    src = R.source_clip(1, 1, (12, 301), seed=5)
    _check_resample(src, [(1, 2, 10, 297)], [True], (10, 270), mode, antialias)


def _stacked(tabs):
    return tuple(torch.from_numpy(np.stack([t[i] for t in tabs])).to(DEV) for i in range(3))


def test_resample_edges_of_the_band_byte_for_byte():
    """40x300 -> 13x260, bicubic with antialias, tables bent per clip (aug_ref.edge_table): the last band holds 5 rows, the second
    column tile 4 live lanes (two of them with bent windows), the y windows hold up to 15 taps -- longer than a band --, windows
    run past the source edge or start in front of it, counts exceed the table's taps, and a row and a column of count 0 come
    out 0.  Against the float32 restatement of the kernel's operation order (aug_ref.resample_f32): every byte equal."""
    from vtx import ops
    B, T, (Hs, Ws), (H, W) = 2, 2, (40, 300), (13, 260)
    src = R.source_clip(B, T, (Hs, Ws), seed=8)
    ytabs, xtabs = [R.edge_table(Hs, H, shift=b) for b in range(B)], [R.edge_table(Ws, W, shift=b) for b in range(B)]
    assert ytabs[0][2].shape[1] == 16 and max(int(R.kernel_windows(t, Hs)[1].max()) for t in ytabs) > 8
    got = ops.clip_resample_u8(src.to(DEV), (H, W), _stacked(xtabs), _stacked(ytabs))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = np.stack([R.resample_f32(src[b].numpy(), ytabs[b], xtabs[b]) for b in range(B)])
    assert np.array_equal(got, want), f'{int((got != want).sum())} bytes differ'
    for b in range(B):
        assert not got[b, :, 6 + b].any() and not got[b, :, :, 6 + b].any() and got[b, 1, 5].any()
    # on well-formed tables the restatement is the float64 evaluation up to rounding ties: it is a reference, not a copy
    plain = [ops.resample_table(n, 0, n, m, 'bicubic', True) for n, m in ((Hs, H), (Ws, W))]
    v64 = R.table_eval(src[1].numpy(), *plain)
    diff = np.abs(R.resample_f32(src[1].numpy(), *plain).astype(np.float64) - np.rint(np.clip(v64, 0.0, 255.0)))
    assert np.all((diff == 0) | (R.near_tie(v64) & (diff <= 1)))


def _jit_records(recs):
    jo = np.zeros((len(recs), 4), dtype=np.int32)
    jf = np.zeros((len(recs), 6), dtype=np.float32)
    for b, (jops, fac) in enumerate(recs):
        jo[b, 0] = len(jops)
        jo[b, 1:1 + len(jops)] = jops
        jf[b, :len(jops)] = fac
        jf[b, 3:3 + len(jops)] = [1.0 - float(f) for f in fac]
    return torch.from_numpy(jo).to(DEV), torch.from_numpy(jf).to(DEV)


def test_jitter_is_bit_identical_to_torchvision_arithmetic():
    """All six orders of the three ops over two calls, factors 0.6 / 1.0 / 1.4 and saturating ones, a clip without ops, a clip with
    two ops; then frames whose pixel count is no multiple of four (the one-pixel-per-thread kernels)."""
    from vtx import ops
    perms = list(itertools.permutations((0, 1, 2)))
    calls = [
        ((4, 2, 32, 32), [(perms[0], (0.6, 1.0, 1.4)), (perms[1], (1.4, 0.6, 1.0)), (), (perms[2], (3.0, 1.4, 0.6))]),
        ((4, 2, 32, 32), [(perms[3], (1.0, 1.4, 0.6)), (perms[4], (0.0, 2.5, 1.4)), (perms[5], (0.731, 1.289, 0.0)), ((1, 0), (1.4, 1.3))]),
        ((3, 2, 5, 7), [(perms[5], (1.4, 0.6, 1.3)), (), (perms[2], (0.6, 1.4, 1.4))]),
    ]
    for n, (shape, recs) in enumerate(calls):
        recs = [r if r else ((), ()) for r in recs]
        g = torch.Generator().manual_seed(20 + n)
        clip = torch.randint(0, 256, shape + (3,), generator=g, dtype=torch.uint8)
        jo, jf = _jit_records(recs)
        dev = clip.to(DEV)
        out = ops.clip_jitter_u8_(dev, jo, jf)
        torch.cuda.synchronize()
        assert out.data_ptr() == dev.data_ptr()
        out = out.cpu()
        for b, (jops, fac) in enumerate(recs):
            want = R.jitter_ref(clip[b], jops, fac)
            assert torch.equal(out[b], want), f'call {n} clip {b}: ops {jops} factors {fac}: {int((out[b] != want).sum())} bytes differ'
            if not jops:
                assert torch.equal(out[b], clip[b])


def test_clip_augment_feeds_the_models():
    """ClipAugment = the resampler, then the jitter of its output; its uint8 clip under set_input_normalization gives the model
    output of the float clip (aug_u8 / 255 - mean) / std; the mim branch's output goes through hog_fwd."""
    import vtx
    import video_transformer as V
    from model_common import _build
    from vtx import aug
    clip = R.source_clip(2, 4, R.SRC_HW, seed=6)
    a = aug.ClipAugment(img_size=32)
    draws = aug.sample_params(2, R.SRC_HW, generator=torch.Generator().manual_seed(9))
    out = a(clip.to(DEV), generator=torch.Generator().manual_seed(9))
    assert out.shape == (2, 4, 32, 32, 3) and out.dtype == torch.uint8 and out.is_cuda
    assert torch.equal(out, a(clip.to(DEV), params=draws))                     # the generator's draws = sample_params' draws
    plain = a(clip.to(DEV), params=[d._replace(ops=(), factors=()) for d in draws]).cpu()
    for b, d in enumerate(draws):
        assert len(d.ops) == 3
        assert torch.equal(out[b].cpu(), R.jitter_ref(plain[b], d.ops, d.factors))
    mean, std = [0.45, 0.45, 0.45], [0.225, 0.225, 0.225]
    xf = out.cpu().permute(0, 1, 4, 2, 3).float().div(255)
    xf = xf.sub(torch.tensor(mean).view(1, 1, 3, 1, 1)).div(torch.tensor(std).view(1, 1, 3, 1, 1))
    vtx.set_precision('fp32')
    try:
        m, _ = _build(V.TimeSformer, 5, num_frames=4, img_size=32, patch_size=16, embed_dims=128, num_heads=2, num_transformer_layers=2)
        m.eval()
        vtx.set_input_normalization(mean, std)
        with torch.no_grad():
            y8 = m(out)
            yf = m(xf.to(DEV))
    finally:
        vtx.set_input_normalization(None, None)
        vtx.set_precision('auto')
    assert torch.equal(y8, yf)
    mim = aug.ClipAugment(img_size=32, scale=(0.5, 1.0), color_jitter=None)(clip.to(DEV), generator=torch.Generator().manual_seed(2))
    feats = vtx.ops.hog_fwd(mim.view(-1, 32, 32, 3))
    torch.cuda.synchronize()
    assert feats.shape == (8, 2, 2, 108) and bool(torch.isfinite(feats).all())


@pytest.mark.parametrize('mode,antialias', [('bicubic', False), ('bilinear', True)])
def test_clip_eval_is_resize_then_centre_crop(mode, antialias):
    """ClipEval(32): short side 40 -> floor(32 / 0.875) = 36, long side 56 -> int(36 * 56 / 40) = 50, centre 32 x 32."""
    from vtx import aug, ops
    clip = R.source_clip(2, 2, R.SRC_HW, seed=7)
    e = aug.ClipEval(img_size=32, interpolation=mode, antialias=antialias)
    assert e.resized_hw(*R.SRC_HW) == (36, 50)
    got = e(clip.to(DEV)).cpu().numpy()
    ytab = ops.resample_table(40, 0, 40, 36, mode, antialias)
    xtab = ops.resample_table(56, 0, 56, 50, mode, antialias)
    v64 = R.table_eval(clip.numpy(), ytab, xtab)[:, :, 2:34, 9:41]
    diff = np.abs(got.astype(np.float64) - np.rint(np.clip(v64, 0, 255)))
    tie = R.near_tie(v64)
    assert tie.mean() <= R.TIE_SHARE
    assert np.all((diff == 0) | (tie & (diff <= 1)))


def test_bad_arguments_raise_and_launch_nothing():
    from vtx import aug, ops
    a = aug.ClipAugment(img_size=32)
    good = torch.zeros(1, 2, 40, 56, 3, dtype=torch.uint8)
    box = aug.ClipDraw(0, 0, 40, 56, False, (), ())
    ops.profile_start(('clip_resample', 'clip_jitter'))
    try:
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            a(good)
        with pytest.raises(TypeError):
            a(torch.zeros(1, 2, 40, 56, 4, dtype=torch.uint8, device=DEV))
        with pytest.raises(TypeError):
            a(good.to(DEV).float())
        for bad in (box._replace(top=9), box._replace(left=-1), box._replace(width=57), box._replace(height=0)):
            with pytest.raises(ValueError, match='outside'):
                a(good.to(DEV), params=[bad])
        with pytest.raises(ValueError):
            a(good.to(DEV), params=[box, box])
        with pytest.raises(ValueError):
            a(good.to(DEV), params=[box._replace(ops=(1, 1), factors=(1.0, 1.0))])
        torch.cuda.synchronize()
    finally:
        launched = ops.profile_stop()
    assert launched == {'clip_resample': {}, 'clip_jitter': {}}
