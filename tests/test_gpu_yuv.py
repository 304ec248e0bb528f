"""Decoded 4:2:0 clips into the resampler (csrc/yuv.hip, vtx.YUVClip, ops.yuv420_to_rgb_u8, ops.clips_views_yuv, a list of YUVClip
given to vtx.aug.ClipAugment / ClipEval / ClipTest).  The conversion is held against tests/yuv_ref.py, the NumPy restatement of
include/vtx_yuv.h, over every (Y, U, V) triple; the fused kernel against the existing resampler (ops.clips_views_u8, which
tests/test_gpu_ragged.py pins) on the restatement's RGB clips and on the plain conversion's.  Every comparison is torch.equal."""
import functools

import numpy as np
import pytest
import torch

import yuv_ref as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CUSTOM = (7, 301, -333, 90, 4096, 500)                # a matrix of no standard: a negative and a largest coefficient


def _planes(rs, Ts, Hs, Ws, nv12, pad, sentinel=0xEE):
    """Random planes of one clip -> (tight NumPy y, u, v; host tensors y, u[, v] as a decoder with padded lines would hand them
    over: views of wider buffers filled with ``sentinel`` when ``pad``)."""
    Hc, Wc = (Hs + 1) // 2, (Ws + 1) // 2
    y, u, v = (rs.randint(0, 256, s).astype(np.uint8) for s in ((Ts, Hs, Ws), (Ts, Hc, Wc), (Ts, Hc, Wc)))
    if not pad:
        t = (torch.from_numpy(y), torch.from_numpy(np.stack([u, v], axis=-1))) if nv12 else tuple(torch.from_numpy(a) for a in (y, u, v))
        return (y, u, v), t
    yb = torch.full((Ts + 1, Hs + 3, Ws + 9), sentinel, dtype=torch.uint8)         # a frame, rows and columns that belong to nobody
    yv = yb[:Ts, 1:1 + Hs, 5:5 + Ws]
    yv.copy_(torch.from_numpy(y))
    if nv12:
        cb = torch.full((Ts + 1, Hc + 2, Wc + 3, 2), sentinel, dtype=torch.uint8)
        cv = cb[1:, 2:, 1:1 + Wc]
        cv.copy_(torch.from_numpy(np.stack([u, v], axis=-1)))
        return (y, u, v), (yv, cv)
    cb = torch.full((2, Ts, Hc + 1, Wc + 5), sentinel, dtype=torch.uint8)           # U and V in one buffer: the same pitch and frame stride
    uv, vv = cb[0, :, :Hc, 2:2 + Wc], cb[1, :, :Hc, 2:2 + Wc]
    uv.copy_(torch.from_numpy(u))
    vv.copy_(torch.from_numpy(v))
    return (y, u, v), (yv, uv, vv)


def _on_device(t):
    """A strided host view -> the same view of a device copy of its whole buffer (``.to`` alone would pack it)."""
    base = t._base if t._base is not None else t
    return torch.as_strided(base.to(DEV), t.shape, t.stride(), t.storage_offset())


def _clip(rs, shape, nv12, pad, matrix='bt601', full_range=False, sentinel=0xEE):
    """-> (vtx.YUVClip on the device, the restatement's uint8 [Ts,Hs,Ws,3] as a host tensor)."""
    import vtx
    (y, u, v), host = _planes(rs, *shape, nv12, pad, sentinel)
    clip = vtx.YUVClip(*[_on_device(t) for t in host], matrix=matrix, full_range=full_range)
    m = Y.PRESETS[(matrix, full_range)] if isinstance(matrix, str) else matrix
    assert clip.matrix == tuple(m) and clip.nv12 == nv12 and clip.shape == tuple(shape)
    return clip, torch.from_numpy(Y.clip_to_rgb(y, u, v, m))


# ---- the conversion over every triple ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _every_triple():
    """One 4096x4096 frame: chroma sample c = row * 2048 + column holds the pair (U, V) = (c % 65536 >> 8, c % 256), so the
    2048x2048 samples run through all 65536 pairs 64 times; the four luma bytes under a sample of run g = c // 65536 are
    4g .. 4g+3.  -> NumPy y [1,4096,4096], u, v [1,2048,2048]."""
    c = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    u, v, g = ((c & 65535) >> 8).astype(np.uint8), (c & 255).astype(np.uint8), (c >> 16).astype(np.uint8)
    y = np.empty((4096, 4096), dtype=np.uint8)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        y[dy::2, dx::2] = 4 * g + k
    triples = (y.astype(np.int64) << 16) | (np.repeat(np.repeat(u, 2, 0), 2, 1).astype(np.int64) << 8) | np.repeat(np.repeat(v, 2, 0), 2, 1)
    assert np.array_equal(np.unique(triples), np.arange(1 << 24))                  # every triple, once
    return y[None], u[None], v[None]


@functools.lru_cache(maxsize=None)
def _every_triple_on_device():
    y, u, v = _every_triple()
    return tuple(torch.from_numpy(a).to(DEV) for a in (y, u, v, np.stack([u, v], axis=-1)))


@functools.lru_cache(maxsize=None)
def _every_triple_rgb(matrix, full):
    return torch.from_numpy(Y.clip_to_rgb(*_every_triple(), Y.PRESETS[(matrix, full)])).to(DEV)


@pytest.mark.parametrize('nv12', [True, False], ids=['NV12', 'I420'])
@pytest.mark.parametrize('matrix,full', sorted(Y.PRESETS))
def test_conversion_over_every_triple(matrix, full, nv12):
    import vtx
    from vtx import ops
    y, u, v, uv = _every_triple_on_device()
    clip = vtx.YUVClip(y, uv, matrix=matrix, full_range=full) if nv12 else vtx.YUVClip(y, u, v, matrix=matrix, full_range=full)
    got = ops.yuv420_to_rgb_u8(clip)
    want = _every_triple_rgb(matrix, full)
    assert got.shape == (1, 4096, 4096, 3) and got.dtype == torch.uint8 and got.is_contiguous()
    assert torch.equal(got, want), f'{int((got != want).any(-1).sum())} of 2^24 triples differ'


# ---- the fused views against the existing resampler on converted clips ----------------------------------------------------
#: (Ts, Hs, Ws), NV12?, padded lines?, matrix, full range, flip, columns Wr of the resized row, rows Hr of the resized frame and
#: the first of the H = 13 rows taken.  5x7 and 9x6: the last chroma row / column serves one luma row / column (9x6: the last row
#: only); 36x300 -> 60 columns: 5:1, with antialias more than 20 taps; 40x600 -> 280 columns: two column tiles; NV12 and
#: I420, padded and tight, five matrices in one launch
CASES = [((3, 5, 7), True, True, 'bt601', False, False, 20, 13, 0),
         ((2, 9, 6), False, False, 'bt709', True, True, 16, 20, 3),
         ((4, 36, 300), False, True, CUSTOM, False, False, 60, 13, 0),
         ((5, 33, 47), True, False, 'bt709', False, True, 40, 16, 2),
         ((2, 40, 600), True, True, 'bt601', True, False, 280, 13, 0)]
FRAMES = [[2, 0, 2], [1, 1, 0], [3, 0, 1], [4, 4, 0], [1, 0, 1]]
LEFTS = [[0, 8, 4], [4, 0, 2], [48, 0, 17], [0, 28, 13], [268, 250, 0]]          # V = 3 windows of W = 12 columns
H, W = 13, 12                                                                      # 13 rows: the second band holds 5


@functools.lru_cache(maxsize=None)
def _batch(sentinel=0xEE):
    rs = np.random.RandomState(17)
    made = [_clip(rs, shape, nv12, pad, matrix, full, sentinel) for shape, nv12, pad, matrix, full, *_ in CASES]
    return [c for c, _ in made], [r for _, r in made]


def _tables(mode, antialias):
    from vtx import aug
    xs = [(s[2], 0, s[2], Wr, flip, 0, Wr) for s, _, _, _, _, flip, Wr, _, _ in CASES]
    ys = [(s[1], 0, s[1], Hr, False, top, H) for s, _, _, _, _, _, _, Hr, top in CASES]
    up = lambda specs: tuple(torch.from_numpy(a).to(DEV) for a in aug._tables(specs, mode, antialias))
    return up(xs), up(ys), [c[6] for c in CASES]


@pytest.mark.parametrize('mode,antialias', [('bilinear', False), ('bilinear', True), ('bicubic', False), ('bicubic', True)])
def test_views_equal_the_resampler_on_converted_clips(mode, antialias):
    from vtx import ops
    clips, ref_rgb = _batch()
    xtab, ytab, widths = _tables(mode, antialias)
    if antialias and mode == 'bicubic':
        assert xtab[2].shape[2] > 20                                                # many taps
    got = ops.clips_views_yuv(clips, FRAMES, LEFTS, W, xtab, ytab, widths=widths)
    converted = [ops.yuv420_to_rgb_u8(c) for c in clips]
    for a, b in zip(converted, ref_rgb):
        assert torch.equal(a.cpu(), b)                                              # the plain conversion = the restatement, odd sizes and pitches
    want_ref = ops.clips_views_u8([r.to(DEV) for r in ref_rgb], FRAMES, LEFTS, W, xtab, ytab, widths=widths)
    want_dev = ops.clips_views_u8(converted, FRAMES, LEFTS, W, xtab, ytab, widths=widths)
    assert got.shape == (5, 3, 3, H, W, 3) and got.dtype == torch.uint8 and got.is_contiguous()
    assert torch.equal(want_ref, want_dev)
    assert torch.equal(got, want_ref), f'{int((got != want_ref).sum())} bytes differ'
    assert len({bytes(got[b].cpu().numpy().tobytes()) for b in range(5)}) == 5          # five different clips came out


def test_every_frame_and_device_indices():
    """frames=None (clips cut to a common length) and int32 device tensors for frames / left."""
    from vtx import ops
    clips, ref_rgb = _batch()
    xtab, ytab, widths = _tables('bilinear', False)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    want = ops.clips_views_u8([r.to(DEV) for r in ref_rgb], FRAMES, LEFTS, W, xtab, ytab, widths=widths)
    assert torch.equal(ops.clips_views_yuv(clips, i32(FRAMES), i32(LEFTS), W, xtab, ytab, widths=widths), want)
    import vtx
    cut = [vtx.YUVClip(*[p[:2] for p in c.planes], matrix=c.matrix) for c in clips]
    want = ops.clips_views_u8([r[:2].to(DEV) for r in ref_rgb], None, LEFTS, W, xtab, ytab, widths=widths)
    assert torch.equal(ops.clips_views_yuv(cut, None, LEFTS, W, xtab, ytab, widths=widths), want)


def test_guard_bytes():
    """The planes lie in larger buffers: whatever fills the rest -- 0xEE, 0x00 -- the views are the same bytes (only the
    record's extents reach the output), and around out= nothing is written."""
    from vtx import ops
    (clips_a, ref_rgb), (clips_b, _) = _batch(), _batch(0x00)
    assert any(bool((p._base == 0xEE).any()) for c in clips_a for p in c.planes if p._base is not None)
    xtab, ytab, widths = _tables('bicubic', True)
    want = ops.clips_views_u8([r.to(DEV) for r in ref_rgb], FRAMES, LEFTS, W, xtab, ytab, widths=widths)
    n, pad = want.numel(), 4099
    buf = torch.full((pad + n + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    out = buf[pad:pad + n].view(want.shape)
    ret = ops.clips_views_yuv(clips_a, FRAMES, LEFTS, W, xtab, ytab, out=out, widths=widths)
    torch.cuda.synchronize()
    assert ret.data_ptr() == out.data_ptr() and torch.equal(out, want)
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n:] == 0xA5).all())
    assert torch.equal(ops.clips_views_yuv(clips_b, FRAMES, LEFTS, W, xtab, ytab, widths=widths), want)
    # the plain conversion, likewise
    c = clips_a[2]
    rgb = torch.full((pad + c.y.numel() * 3 + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    o = rgb[pad:-pad].view(c.shape + (3,))
    ops.yuv420_to_rgb_u8(c, out=o)
    torch.cuda.synchronize()
    assert torch.equal(o.cpu(), ref_rgb[2]) and bool((rgb[:pad] == 0xA5).all()) and bool((rgb[-pad:] == 0xA5).all())
    assert torch.equal(ops.yuv420_to_rgb_u8(clips_b[2]), o)


# ---- the pipelines ------------------------------------------------------------------------------------------------------
PIPE_SHAPES = [((5, 40, 56), True, True, 'bt601', False), ((3, 36, 300), False, True, 'bt709', False),
               ((4, 56, 40), False, False, 'bt601', True), ((6, 33, 47), True, False, CUSTOM, False)]
PIPE_FRAMES = [[4, 0, 4], [2, 2, 1], [0, 3, 3], [5, 0, 2]]
CLASSES = ('clips_views_yuv', 'clips_views', 'clip_views', 'clip_resample', 'yuv420_to_rgb')


@functools.lru_cache(maxsize=None)
def _pipe_batch():
    from vtx import ops
    rs = np.random.RandomState(29)
    clips = [_clip(rs, *c)[0] for c in PIPE_SHAPES]
    return clips, [ops.yuv420_to_rgb_u8(c) for c in clips]


def _launches(fn):
    from vtx import ops
    ops.profile_start(CLASSES)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        prof = ops.profile_stop()
    return out, {c: sum(v[0] for v in d.values()) for c, d in prof.items() if d}


def _pipes():
    from vtx import aug
    draws = [aug.ClipDraw(37, 51, 3, 5, True, (), ()),
             aug.ClipDraw(0, 0, 36, 300, False, (0, 1, 2), (1.2, 0.7, 1.3)),
             aug.ClipDraw(10, 4, 30, 33, False, (2,), (0.6,)),
             aug.ClipDraw(1, 2, 31, 44, True, (), (), ((5, 8.7), (11, 178.5)))]
    return [(aug.ClipAugment(img_size=24), {'params': draws}), (aug.ClipAugment(img_size=24, antialias=True), {'params': draws}),
            (aug.ClipEval(img_size=20), {}), (aug.ClipTest(32, short_side=36), {}), (aug.ClipTest(32, short_side=36, antialias=True), {})]


@pytest.mark.parametrize('k', range(5), ids=['augment', 'augment-antialias', 'eval', 'test', 'test-antialias'])
def test_pipelines_on_yuv_clips_equal_the_converted_rgb_route(k):
    pipe, kw = _pipes()[k]
    clips, rgb = _pipe_batch()
    got, n_yuv = _launches(lambda: pipe(clips, frames=PIPE_FRAMES, **kw))
    want, n_rgb = _launches(lambda: pipe(rgb, frames=PIPE_FRAMES, **kw))
    assert n_yuv == {'clips_views_yuv': 1} and n_rgb == {'clips_views': 1}           # one launch, and not the RGB kernel
    assert got.dtype == torch.uint8 and got.is_contiguous() and got.shape == want.shape and got.shape[0] == 4 * getattr(pipe, 'n_crops', 1)
    assert torch.equal(got, want), f'{int((got != want).sum())} bytes differ'
    assert torch.equal(pipe(tuple(clips), frames=PIPE_FRAMES, **kw), want)           # a tuple is a list


def test_drawn_params_come_from_the_shapes():
    """sample_params' src_hw comes from .shape: the draws of the YUV list are those of the RGB list on the same generator."""
    from vtx import aug
    clips, rgb = _pipe_batch()
    a = aug.ClipAugment(img_size=24)
    g, h = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    assert torch.equal(a(clips, generator=g, frames=PIPE_FRAMES), a(rgb, generator=h, frames=PIPE_FRAMES))
    assert torch.equal(g.get_state(), h.get_state())


def test_a_mixed_list_is_refused_and_nothing_is_launched():
    from vtx import aug, ops
    clips, rgb = _pipe_batch()
    xs, ys, lefts = aug.ClipTest(32, short_side=36).specs([c.shape[1:] for c in clips])
    tabs = [tuple(torch.from_numpy(a).to(DEV) for a in aug._tables(s, 'bilinear', False)) for s in (xs, ys)]

    def bad():
        for pipe, kw in _pipes()[::2]:
            with pytest.raises(TypeError, match='clip 1 is a Tensor beside YUVClip'):
                pipe([clips[0], rgb[1], clips[2], clips[3]], frames=PIPE_FRAMES, **kw)
            with pytest.raises(TypeError, match='clip 3 is a Tensor beside YUVClip'):
                pipe(clips[:3] + [rgb[3]], frames=PIPE_FRAMES, **kw)
            with pytest.raises(ValueError, match='of clip 1 outside its 3 decoded frames'):
                pipe(clips, frames=[[4, 0, 4], [2, 3, 1], [0, 3, 3], [5, 0, 2]], **kw)
            with pytest.raises(ValueError, match='lengths must agree'):
                pipe(clips, **kw)
        with pytest.raises(TypeError, match='uint8 tensors is expected, got YUVClip'):
            ops.clips_views_u8(clips, PIPE_FRAMES, lefts, 32, *tabs, widths=[s[6] for s in xs])
        with pytest.raises(TypeError, match='YUVClip is expected, got tensors'):
            ops.clips_views_yuv(rgb, PIPE_FRAMES, lefts, 32, *tabs, widths=[s[6] for s in xs])
        with pytest.raises(TypeError, match='table must be the int32 \\[88\\]'):
            ops.clips_views_yuv(ops.clips_table(clips, [s[6] for s in xs]), PIPE_FRAMES, lefts, 32, *tabs,
                                table=torch.zeros(24, dtype=torch.int32, device=DEV))
    _, launched = _launches(bad)
    assert launched == {}


def test_timesformer_forward_on_both_routes():
    """The model sees the same uint8 batch from either route, so its output is the same bits."""
    import vtx
    import video_transformer as V
    from oracle import synth
    from vtx import aug
    clips, rgb = _pipe_batch()
    ev = aug.ClipEval(img_size=32)
    frames = [f[:2] for f in PIPE_FRAMES]
    m = V.TimeSformer(num_frames=2, img_size=32, patch_size=16, embed_dims=128, num_heads=2, num_transformer_layers=1)
    m.load_state_dict(synth.synth_state_dict(synth.shapes_of(m), 3))
    m.to(DEV).eval()
    vtx.set_precision('fp32')
    vtx.set_input_normalization([0.45, 0.45, 0.45], [0.225, 0.225, 0.225])
    try:
        with torch.no_grad():
            a, b = m(ev(clips, frames=frames)), m(ev(rgb, frames=frames))
    finally:
        vtx.set_input_normalization(None, None)
        vtx.set_precision('auto')
    assert a.shape[0] == 4 and bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_tensors_launch_what_they_launched_before():
    """A 5-D tensor and a list of tensors: exactly the classes of the parent, and nothing of libvtx_yuv.so."""
    from vtx import aug
    _, rgb = _pipe_batch()
    five = torch.stack([r[:3, :33, :40] for r in rgb])
    for pipe, kw in _pipes()[2:4]:
        _, n = _launches(lambda: pipe(rgb, frames=PIPE_FRAMES, **kw))
        assert n == {'clips_views': 1}
        _, n = _launches(lambda: pipe(five, frames=[[2, 0]] * 4, **kw))
        assert n == {'clip_views': 1}
    _, n = _launches(lambda: aug.ClipEval(img_size=20)(five))
    assert n == {'clip_resample': 1}
    _, n = _launches(lambda: aug.ClipTest(32, short_side=36)(five))
    assert n == {'clip_views': 1}
