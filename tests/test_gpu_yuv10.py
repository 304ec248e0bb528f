"""Decoded 10-bit 4:2:0 clips into the resampler (csrc/yuv10.hip, vtx.YUVClip(depth=10), ops.yuv420_to_rgb_u8 and
ops.clips_views_yuv on them, lists of 10-bit or mixed YUVClip given to vtx.aug.ClipAugment / ClipEval / ClipTest).  The conversion
is held against tests/yuv10_ref.py, the NumPy restatement of include/vtx_yuv10.h, over the sample set S; the fused kernel
against the existing resampler (ops.clips_views_u8, which tests/test_gpu_ragged.py pins) on the restatement's RGB clips and on
the plain conversion's; 8-bit clips in a mixed list against libvtx_yuv.so.  Every comparison is torch.equal."""
import functools

import numpy as np
import pytest
import torch

import yuv10_ref as Y10
import yuv_ref as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CUSTOM10 = (29, 1203, -1333, 360, 16384, 2000)        # a matrix of no standard: a negative and a largest coefficient
CUSTOM8 = (7, 301, -333, 90, 4096, 500)


def _i16(a):
    """uint16 NumPy words -> an int16 host tensor of the same bits (what a reader hands over where uint16 is not at hand)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16))


def _on_device(t):
    """A strided host view -> the same view of a device copy of its whole buffer (``.to`` alone would pack it)."""
    base = t._base if t._base is not None else t
    return torch.as_strided(base.to(DEV), t.shape, t.stride(), t.storage_offset())


def _planes10(rs, Ts, Hs, Ws, inter, shift, pad, sentinel=0xEEEE):
    """Random 10-bit planes of one clip -> (tight NumPy words y, u, v: the samples moved left by ``shift``; host int16 tensors
    y, u[, v] as a decoder with padded lines would hand them over: views of wider buffers filled with ``sentinel`` when
    ``pad``, the interleaved chroma view then starting at an address that is 2 but not 4 bytes aligned)."""
    Hc, Wc = (Hs + 1) // 2, (Ws + 1) // 2
    y, u, v = ((rs.randint(0, 1024, s) << shift).astype(np.uint16) for s in ((Ts, Hs, Ws), (Ts, Hc, Wc), (Ts, Hc, Wc)))
    if not pad:
        return (y, u, v), ((_i16(y), _i16(np.stack([u, v], axis=-1))) if inter else tuple(_i16(a) for a in (y, u, v)))
    fill = lambda *s: _i16(np.full(s, sentinel, dtype=np.uint16))
    yv = fill(Ts + 1, Hs + 3, Ws + 9)[:Ts, 1:1 + Hs, 5:5 + Ws]                     # a frame, rows and columns that belong to nobody
    yv.copy_(_i16(y))
    if inter:
        n = (Ts + 1) * (Hc + 2) * (Wc + 3) * 2
        cv = fill(n + 1)[1:].view(Ts + 1, Hc + 2, Wc + 3, 2)[1:, 2:, 1:1 + Wc]      # one word into the buffer: the pairs are not 4-byte aligned
        cv.copy_(_i16(np.stack([u, v], axis=-1)))
        return (y, u, v), (yv, cv)
    cb = fill(2, Ts, Hc + 1, Wc + 5)                                               # U and V in one buffer: the same pitch and frame stride
    uv, vv = cb[0, :, :Hc, 2:2 + Wc], cb[1, :, :Hc, 2:2 + Wc]
    uv.copy_(_i16(u))
    vv.copy_(_i16(v))
    return (y, u, v), (yv, uv, vv)


def _clip10(rs, shape, inter, msb, pad, matrix='bt601', full_range=False, sentinel=0xEEEE):
    """-> (vtx.YUVClip(depth=10) on the device, the restatement's uint8 [Ts,Hs,Ws,3] as a host tensor).  ``msb`` None: what the
    layout says."""
    import vtx
    shift = 6 if (inter if msb is None else msb) else 0
    (y, u, v), host = _planes10(rs, *shape, inter, shift, pad, sentinel)
    clip = vtx.YUVClip(*[_on_device(t) for t in host], matrix=matrix, full_range=full_range, depth=10, msb_aligned=msb)
    m = Y10.PRESETS[(matrix, full_range)] if isinstance(matrix, str) else matrix
    assert clip.matrix == tuple(m) and clip.nv12 == inter and clip.shape == tuple(shape) and clip.depth == 10 and clip.shift == shift
    if pad and inter:
        assert clip.u.data_ptr() % 4 == 2
    return clip, torch.from_numpy(Y10.clip_to_rgb(y, np.stack([u, v], axis=-1) if inter else u, None if inter else v, m, shift=shift))


def _clip8(rs, shape, nv12, matrix='bt601', full_range=False):
    """A tight 8-bit clip -> (vtx.YUVClip on the device, the 8-bit restatement's RGB as a host tensor)."""
    import vtx
    Ts, Hs, Ws = shape
    Hc, Wc = (Hs + 1) // 2, (Ws + 1) // 2
    y, u, v = (rs.randint(0, 256, s).astype(np.uint8) for s in ((Ts, Hs, Ws), (Ts, Hc, Wc), (Ts, Hc, Wc)))
    host = (y, np.stack([u, v], axis=-1)) if nv12 else (y, u, v)
    clip = vtx.YUVClip(*[torch.from_numpy(a).to(DEV) for a in host], matrix=matrix, full_range=full_range)
    assert clip.depth == 8 and clip.shift == 0
    m = Y.PRESETS[(matrix, full_range)] if isinstance(matrix, str) else matrix
    return clip, torch.from_numpy(Y.clip_to_rgb(y, u, v, m))


CLASSES = ('clips_views_yuv10', 'yuv10_to_rgb', 'clips_views_yuv', 'clips_views', 'clip_views', 'clip_resample', 'yuv420_to_rgb')


def _launches(fn):
    from vtx import ops
    ops.profile_start(CLASSES)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        prof = ops.profile_stop()
    return out, {c: sum(v[0] for v in d.values()) for c, d in prof.items() if d}


# ---- the conversion over the sample set S ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _s_frame():
    """One frame of 4096 columns that realises every triple of S under 4:2:0 sharing, after tests/test_gpu_yuv.py's
    _every_triple: the triples sorted by chroma pair, each pair's run filled to a multiple of four with its last triple, four
    consecutive triples under one chroma sample at (0,0), (0,1), (1,0), (1,1).  -> NumPy int32 samples y [1,2Hc,4096],
    u, v [1,Hc,2048]."""
    yy, uu, vv = Y10.sample_set()
    key = np.unique((uu << 20) | (vv << 10) | yy)                                   # sorted: the triples of one pair are adjacent
    start = np.r_[0, np.flatnonzero(np.diff(key >> 10)) + 1]
    count = np.diff(np.r_[start, key.size])
    idx = np.sort(np.concatenate([np.arange(key.size), np.repeat(start + count - 1, (-count) % 4)]))
    Hc = -(-(idx.size // 4) // 2048)
    idx = np.concatenate([idx, np.full(4 * 2048 * Hc - idx.size, key.size - 1)])     # the last chroma row filled with the last triple
    seen = np.zeros(key.size, dtype=bool)
    seen[idx] = True
    assert seen.all()                                                              # every triple of S is somewhere
    k = key[idx].reshape(Hc, 2048, 2, 2)                                            # chroma row, chroma column, dy, dx
    y = (k & 1023).transpose(0, 2, 1, 3).reshape(2 * Hc, 4096)
    u, v = k[:, :, 0, 0] >> 20, (k[:, :, 0, 0] >> 10) & 1023
    up = lambda c: np.repeat(np.repeat(c, 2, 0), 2, 1)
    assert np.array_equal(((up(u) << 20) | (up(v) << 10) | y).reshape(Hc, 2, 2048, 2).transpose(0, 2, 1, 3), k)      # and what the planes realise is it
    return y[None].astype(np.int32), u[None].astype(np.int32), v[None].astype(np.int32)


@functools.lru_cache(maxsize=None)
def _s_frame_on_device(p010):
    """-> (y, uv) P010 words or (y, u, v) yuv420p10le words, int16 device tensors."""
    y, u, v = _s_frame()
    if p010:
        return tuple(_i16(a << 6).to(DEV) for a in (y, np.stack([u, v], axis=-1)))
    return tuple(_i16(a).to(DEV) for a in (y, u, v))


@functools.lru_cache(maxsize=None)
def _s_frame_rgb(matrix, full):
    y, u, v = _s_frame()
    up = lambda c: np.repeat(np.repeat(c, 2, 1), 2, 2)
    return torch.from_numpy(Y10.convert(y, up(u), up(v), Y10.PRESETS[(matrix, full)])).to(DEV)


@pytest.mark.parametrize('matrix,full,p010', [(m, f, True) for m, f in sorted(Y10.PRESETS)] + [('bt709', False, False)],
                         ids=lambda v: {True: 'y', False: 'n'}.get(v, v))
def test_conversion_over_the_sample_set(matrix, full, p010):
    import vtx
    from vtx import ops
    clip = vtx.YUVClip(*_s_frame_on_device(p010), matrix=matrix, full_range=full, depth=10)
    assert clip.shift == (6 if p010 else 0)
    got, n = _launches(lambda: ops.yuv420_to_rgb_u8(clip))
    want = _s_frame_rgb(matrix, full)
    assert n == {'yuv10_to_rgb': 1}
    assert got.shape == want.shape and got.shape[2:] == (4096, 3) and got.dtype == torch.uint8 and got.is_contiguous()
    assert torch.equal(got, want), f'{int((got != want).any(-1).sum())} pixels differ'


def test_stray_bits_do_not_reach_the_bytes():
    """Random low 6 bits in P010 words, random upper 6 bits in LSB-aligned words: the same bytes as the clean words'."""
    import vtx
    from vtx import ops
    rs = np.random.RandomState(5)
    y, u, v = (a[:, :r] for a, r in zip(_s_frame(), (512, 256, 256)))
    uv = np.stack([u, v], axis=-1)
    want = _s_frame_rgb('bt601', False)[:, :512]
    low, high = (lambda a: rs.randint(0, 64, a.shape)), (lambda a: rs.randint(0, 64, a.shape) << 10)
    dirty = vtx.YUVClip(_i16((y << 6) | low(y)).to(DEV), _i16((uv << 6) | low(uv)).to(DEV), depth=10)
    assert bool((dirty.y & 63).any()) and bool((dirty.u & 63).any()) and torch.equal(ops.yuv420_to_rgb_u8(dirty), want)
    dirty = vtx.YUVClip(*(_i16(a | high(a)).to(DEV) for a in (y, u, v)), depth=10)
    assert all(bool((p.view(torch.uint8)[..., 1::2] > 3).any()) for p in dirty.planes) and torch.equal(ops.yuv420_to_rgb_u8(dirty), want)
    # uint16 planes are the same bits
    clean = vtx.YUVClip(*(_i16(a).to(DEV).view(torch.uint16) for a in (y, u, v)), depth=10)
    assert clean.y.dtype == torch.uint16 and torch.equal(ops.yuv420_to_rgb_u8(clean), want)


def test_times_four_identity_on_the_device():
    """A 10-bit clip that is 4 x an 8-bit clip, with the matrix x 4, gives the bytes of the 8-bit route (libvtx_yuv.so); so does
    the 8-bit clip's own record through libvtx_yuv10.so."""
    import vtx
    from vtx import _lib, ops
    rs = np.random.RandomState(11)
    for shape, nv12, m in (((2, 33, 47), True, 'bt601'), ((3, 9, 6), False, CUSTOM8), ((1, 64, 300), True, (255, 4096, -4096, 4096, -4096, 4096))):
        c8, ref = _clip8(rs, shape, nv12, m)
        want, n = _launches(lambda: ops.yuv420_to_rgb_u8(c8))
        assert n == {'yuv420_to_rgb': 1} and torch.equal(want.cpu(), ref)
        for msb in (True, False):
            words = [torch.from_numpy(((p.cpu().numpy().astype(np.uint16) * 4) << (6 if msb else 0)).view(np.int16)).to(DEV) for p in c8.planes]
            c10 = vtx.YUVClip(*words, matrix=tuple(4 * c for c in c8.matrix), depth=10, msb_aligned=msb)
            got, n = _launches(lambda: ops.yuv420_to_rgb_u8(c10))
            assert n == {'yuv10_to_rgb': 1} and torch.equal(got, want), (shape, msb)
        rec, out = ops.upload_i32(c8.record10(), DEV), torch.empty_like(want)
        _lib.yuv10_call('vtx_yuv10_to_rgb_u8', ops.ptr(rec), *shape, ops.ptr(out), ops.stream())
        assert torch.equal(out, want)


# ---- the fused views against the existing resampler on converted clips ----------------------------------------------------
#: (Ts, Hs, Ws), interleaved chroma?, msb_aligned (None: what the layout says), padded lines?, matrix, full range, flip, columns Wr
#: of the resized row, rows Hr of the resized frame and the first of the H = 13 rows taken.  5x7 and 9x6: the last chroma row /
#: column serves one luma row / column; 36x300 -> 60 columns: 5:1, with antialias more than 20 taps; 40x600 -> 280 columns: two
#: column tiles; P010 and yuv420p10le, an interleaved plane with LSB samples and planar ones with MSB samples, padded and tight
CASES = [((3, 5, 7), True, None, True, 'bt601', False, False, 20, 13, 0),
         ((2, 9, 6), False, None, False, 'bt709', True, True, 16, 20, 3),
         ((4, 36, 300), False, True, True, CUSTOM10, False, False, 60, 13, 0),
         ((5, 33, 47), True, False, False, 'bt709', False, True, 40, 16, 2),
         ((2, 40, 600), True, None, True, 'bt601', True, False, 280, 13, 0)]
FRAMES = [[2, 0, 2], [1, 1, 0], [3, 0, 1], [4, 4, 0], [1, 0, 1]]
LEFTS = [[0, 8, 4], [4, 0, 2], [48, 0, 17], [0, 28, 13], [268, 250, 0]]          # V = 3 windows of W = 12 columns
H, W = 13, 12                                                                      # 13 rows: the second band holds 5


@functools.lru_cache(maxsize=None)
def _batch(sentinel=0xEEEE):
    rs = np.random.RandomState(17)
    made = [_clip10(rs, shape, inter, msb, pad, matrix, full, sentinel) for shape, inter, msb, pad, matrix, full, *_ in CASES]
    return [c for c, _ in made], [r for _, r in made]


def _tables(mode, antialias, cases=CASES):
    from vtx import aug
    xs = [(c[0][2], 0, c[0][2], c[-3], c[-4], 0, c[-3]) for c in cases]
    ys = [(c[0][1], 0, c[0][1], c[-2], False, c[-1], H) for c in cases]
    up = lambda specs: tuple(torch.from_numpy(a).to(DEV) for a in aug._tables(specs, mode, antialias))
    return up(xs), up(ys), [c[-3] for c in cases]


@pytest.mark.parametrize('mode,antialias', [('bilinear', False), ('bilinear', True), ('bicubic', False), ('bicubic', True)])
def test_views_equal_the_resampler_on_converted_clips(mode, antialias):
    from vtx import ops
    clips, ref_rgb = _batch()
    xtab, ytab, widths = _tables(mode, antialias)
    if antialias and mode == 'bicubic':
        assert xtab[2].shape[2] > 20                                                # many taps
    got, n = _launches(lambda: ops.clips_views_yuv(clips, FRAMES, LEFTS, W, xtab, ytab, widths=widths))
    assert n == {'clips_views_yuv10': 1}
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
    import vtx
    from vtx import ops
    clips, ref_rgb = _batch()
    xtab, ytab, widths = _tables('bilinear', False)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    want = ops.clips_views_u8([r.to(DEV) for r in ref_rgb], FRAMES, LEFTS, W, xtab, ytab, widths=widths)
    assert torch.equal(ops.clips_views_yuv(clips, i32(FRAMES), i32(LEFTS), W, xtab, ytab, widths=widths), want)
    cut = [vtx.YUVClip(*[p[:2] for p in c.planes], matrix=c.matrix, depth=10, msb_aligned=bool(c.shift)) for c in clips]
    want = ops.clips_views_u8([r[:2].to(DEV) for r in ref_rgb], None, LEFTS, W, xtab, ytab, widths=widths)
    assert torch.equal(ops.clips_views_yuv(cut, None, LEFTS, W, xtab, ytab, widths=widths), want)


def test_a_mixed_list_is_one_launch():
    """8-bit NV12, P010, I420, yuv420p10le in one list: one launch of the new class; each clip's views are those of the call on
    that clip alone; the 8-bit clips' bytes are those of the all-8-bit route through vtx_clips_views_yuv420."""
    from vtx import ops
    rs = np.random.RandomState(23)
    cases = [((3, 33, 47), 'nv12', 'bt601', False, False, 40, 16, 2), ((4, 36, 300), 'p010', 'bt709', False, True, 60, 13, 0),
             ((2, 9, 6), 'i420', CUSTOM8, False, False, 16, 20, 3), ((5, 40, 56), 'p10le', 'bt601', True, False, 24, 14, 1)]
    made = [_clip8(rs, c[0], c[1] == 'nv12', c[2], c[3]) if c[1] in ('nv12', 'i420') else
            _clip10(rs, c[0], c[1] == 'p010', None, True, c[2], c[3]) for c in cases]
    clips, ref_rgb = [c for c, _ in made], [r.to(DEV) for _, r in made]
    assert [c.depth for c in clips] == [8, 10, 8, 10]
    frames, lefts = [[2, 0, 2], [3, 0, 1], [1, 1, 0], [4, 4, 0]], [[0, 28, 13], [48, 0, 17], [4, 0, 2], [12, 5, 0]]
    for mode, antialias in (('bilinear', False), ('bicubic', True)):
        xtab, ytab, widths = _tables(mode, antialias, cases)
        got, n = _launches(lambda: ops.clips_views_yuv(clips, frames, lefts, W, xtab, ytab, widths=widths))
        assert n == {'clips_views_yuv10': 1}
        assert torch.equal(got, ops.clips_views_u8(ref_rgb, frames, lefts, W, xtab, ytab, widths=widths))
        row = lambda tab, bs: tuple(torch.stack([a[b] for b in bs]) for a in tab)
        for b in range(4):
            one, n = _launches(lambda: ops.clips_views_yuv([clips[b]], [frames[b]], [lefts[b]], W, row(xtab, [b]), row(ytab, [b]), widths=[widths[b]]))
            assert n == ({'clips_views_yuv10': 1} if clips[b].depth == 10 else {'clips_views_yuv': 1})
            assert torch.equal(got[b], one[0]), b
        eight, n = _launches(lambda: ops.clips_views_yuv([clips[0], clips[2]], [frames[0], frames[2]], [lefts[0], lefts[2]], W,
                                                         row(xtab, [0, 2]), row(ytab, [0, 2]), widths=[widths[0], widths[2]]))
        assert n == {'clips_views_yuv': 1} and torch.equal(got[[0, 2]], eight)


def test_guard_bytes():
    """The planes lie in larger buffers: whatever fills the rest -- 0xEEEE, 0x0000 -- the views are the same bytes (only the
    record's extents reach the output), and around out= nothing is written."""
    from vtx import ops
    (clips_a, ref_rgb), (clips_b, _) = _batch(), _batch(0x0000)
    assert any(bool((p._base.view(torch.uint8) == 0xEE).any()) for c in clips_a for p in c.planes if p._base is not None)
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
PIPE_SHAPES = [((5, 40, 56), True, None, True, 'bt601', False), ((3, 36, 300), False, None, True, 'bt709', False),
               ((4, 56, 40), False, True, False, 'bt601', True), ((6, 33, 47), True, False, False, CUSTOM10, False)]
PIPE_FRAMES = [[4, 0, 4], [2, 2, 1], [0, 3, 3], [5, 0, 2]]


@functools.lru_cache(maxsize=None)
def _pipe_batch():
    from vtx import ops
    rs = np.random.RandomState(29)
    clips = [_clip10(rs, *c)[0] for c in PIPE_SHAPES]
    return clips, [ops.yuv420_to_rgb_u8(c) for c in clips]


def _pipes():
    from vtx import aug
    draws = [aug.ClipDraw(37, 51, 3, 5, True, (), ()),
             aug.ClipDraw(0, 0, 36, 300, False, (0, 1, 2), (1.2, 0.7, 1.3)),
             aug.ClipDraw(10, 4, 30, 33, False, (2,), (0.6,)),
             aug.ClipDraw(1, 2, 31, 44, True, (), (), ((5, 8.7), (11, 178.5)))]
    return [(aug.ClipAugment(img_size=24), {'params': draws}), (aug.ClipAugment(img_size=24, antialias=True), {'params': draws}),
            (aug.ClipEval(img_size=20), {}), (aug.ClipTest(32, short_side=36), {}), (aug.ClipTest(32, short_side=36, antialias=True), {})]


@pytest.mark.parametrize('k', range(5), ids=['augment', 'augment-antialias', 'eval', 'test', 'test-antialias'])
def test_pipelines_on_10bit_clips_equal_the_converted_rgb_route(k):
    pipe, kw = _pipes()[k]
    clips, rgb = _pipe_batch()
    got, n_yuv = _launches(lambda: pipe(clips, frames=PIPE_FRAMES, **kw))
    want, n_rgb = _launches(lambda: pipe(rgb, frames=PIPE_FRAMES, **kw))
    assert n_yuv == {'clips_views_yuv10': 1} and n_rgb == {'clips_views': 1}         # one launch, and not the RGB kernel
    assert got.dtype == torch.uint8 and got.is_contiguous() and got.shape == want.shape and got.shape[0] == 4 * getattr(pipe, 'n_crops', 1)
    assert torch.equal(got, want), f'{int((got != want).sum())} bytes differ'
    assert torch.equal(pipe(tuple(clips), frames=PIPE_FRAMES, **kw), want)           # a tuple is a list


def test_drawn_params_come_from_the_luma_shapes():
    """sample_params' src_hw comes from .shape, the luma's: the draws of the 10-bit list are those of the RGB list on the same
    generator."""
    from vtx import aug
    clips, rgb = _pipe_batch()
    a = aug.ClipAugment(img_size=24)
    g, h = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    assert torch.equal(a(clips, generator=g, frames=PIPE_FRAMES), a(rgb, generator=h, frames=PIPE_FRAMES))
    assert torch.equal(g.get_state(), h.get_state())


def test_other_lists_launch_what_they_launched_before():
    """A list of 8-bit YUVClip, a list of tensors and a 5-D tensor: exactly the classes of the parent, nothing of libvtx_yuv10.so."""
    from vtx import aug
    rs = np.random.RandomState(31)
    eight = [_clip8(rs, c[0], c[1], 'bt601')[0] for c in PIPE_SHAPES]
    _, rgb = _pipe_batch()
    five = torch.stack([r[:3, :33, :40] for r in rgb])
    for pipe, kw in _pipes()[::2]:
        _, n = _launches(lambda: pipe(eight, frames=PIPE_FRAMES, **kw))
        assert n == {'clips_views_yuv': 1}
        _, n = _launches(lambda: pipe(rgb, frames=PIPE_FRAMES, **kw))
        assert n == {'clips_views': 1}
    for pipe, kw in _pipes()[2:4]:
        _, n = _launches(lambda: pipe(five, frames=[[2, 0]] * 4, **kw))
        assert n == {'clip_views': 1}
    _, n = _launches(lambda: aug.ClipEval(img_size=20)(five))
    assert n == {'clip_resample': 1}


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
