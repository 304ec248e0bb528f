"""Clips of differing source size in one launch (csrc/ragged.hip, vtx.ops.clips_views_u8, a list given to vtx.aug.ClipAugment /
ClipEval / ClipTest).  The oracle is always the existing path run clip by clip and concatenated -- pipe(c[None], params=[p],
frames=f[None]) -- which tests/test_gpu_aug.py and tests/test_gpu_views.py pin against torch; every comparison is torch.equal."""
import functools

import numpy as np
import pytest
import torch

import aug_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 11

#: (Ts, Hs, Ws): a landscape clip; a row longer than one 256-column tile beside three clips for which that tile is dead; a
#: portrait clip; odd sizes with an unaligned row length
SHAPES = [(5, 40, 56), (3, 36, 300), (4, 56, 40), (6, 33, 47)]
#: the last frame of every clip, repeats and reversed order: a stride taken from another clip's Ts / Hs / Ws shows up
FRAMES = [[4, 0, 4], [2, 2, 1], [0, 3, 3], [5, 0, 2]]


@functools.lru_cache(maxsize=None)
def _clips():
    """The four source clips on the device (random bytes; frame 0 all 0 and the last frame all 255, as aug_ref.source_clip)."""
    return tuple(R.source_clip(1, Ts, (Hs, Ws), seed=SEED + b)[0].to(DEV) for b, (Ts, Hs, Ws) in enumerate(SHAPES))


def _one_by_one(pipe, clips, frames, params=None):
    """The parent's only route: one call per clip, concatenated."""
    outs = []
    for b, c in enumerate(clips):
        kw = {} if params is None else {'params': [params[b]]}
        outs.append(pipe(c[None], frames=None if frames is None else [frames[b]], **kw))
    return torch.cat(outs)


@pytest.mark.parametrize('antialias', [False, True])
def test_clip_test_on_a_list_equals_the_clips_one_by_one(antialias):
    """ClipTest(32, short_side=36), bilinear: resized rows of 50, 300, 36 and 51 columns, all 12 views byte-equal."""
    from vtx import aug
    t = aug.ClipTest(32, short_side=36, antialias=antialias)
    clips = list(_clips())
    got = t(clips, frames=FRAMES)
    want = _one_by_one(t, clips, FRAMES)
    assert got.shape == (12, 3, 32, 32, 3) and got.dtype == torch.uint8 and got.is_cuda and got.is_contiguous()
    assert torch.equal(got, want), f'{int((got != want).sum())} bytes differ'
    assert bool((got[0, 1] == 0).all()) and bool((got[0, 0] == 255).all())          # clip 0: frame 0 is all 0, frame 4 all 255
    assert bool((got[3, 0] == 255).all()) and bool((got[9, 0] == 255).all())        # clips 1 and 3: their own last frames
    assert torch.equal(t(tuple(clips), frames=FRAMES), got)                          # a tuple is a list
    # one row [T] for every clip alike
    assert torch.equal(t(clips, frames=[2, 0]), _one_by_one(t, clips, [[2, 0]] * 4))


@pytest.mark.parametrize('antialias', [False, True])
def test_clip_eval_on_a_list_equals_the_clips_one_by_one(antialias):
    """ClipEval(img_size=20), bicubic: the last 8-row band holds 4 rows; with antialias the tap counts differ between the clips
    and the tables are padded to the largest."""
    from vtx import aug, ops
    e = aug.ClipEval(img_size=20, antialias=antialias)
    clips = list(_clips())
    if antialias:
        taps = {ops.resample_max_taps(Hs, e.resized_hw(Hs, Ws)[0], 'bicubic', True) for _, Hs, Ws in SHAPES}
        assert taps == {7, 9}                                                        # the y tables: 33 -> 22 rows needs 7, the others 9
    got = e(clips, frames=FRAMES)
    want = _one_by_one(e, clips, FRAMES)
    assert got.shape == (4, 3, 20, 20, 3) and got.dtype == torch.uint8
    assert torch.equal(got, want), f'{int((got != want).sum())} bytes differ'


def _augment_case():
    """Clips and explicit draws for ClipAugment(24): a 3x5 corner crop with flip; a full-frame crop with all three jitter ops,
    contrast in the middle; a RandAugment record (Rotate, then Solarize); a 24x24 source of 4 frames with a full-frame crop --
    the identity: one tap of weight 1."""
    from vtx import aug
    c = _clips()
    clips = [c[0], c[1], c[2], c[3][:4, :24, :24].contiguous()]
    draws = [aug.ClipDraw(37, 51, 3, 5, True, (), ()),
             aug.ClipDraw(0, 0, 36, 300, False, (0, 1, 2), (1.2, 0.7, 1.3)),
             aug.ClipDraw(10, 4, 30, 33, False, (), (), ((5, 8.7), (11, 178.5))),
             aug.ClipDraw(0, 0, 24, 24, False, (), ())]
    return clips, draws


@pytest.mark.parametrize('antialias', [True, False])
def test_clip_augment_on_a_list_equals_the_clips_one_by_one(antialias):
    from vtx import aug
    a = aug.ClipAugment(img_size=24, antialias=antialias)
    clips, draws = _augment_case()
    frames = [[4, 0, 4], [2, 2, 1], [0, 3, 3], [3, 0, 2]]
    got = a(clips, params=draws, frames=frames)
    want = _one_by_one(a, clips, frames, draws)
    assert got.shape == (4, 3, 24, 24, 3) and torch.equal(got, want), f'{int((got != want).sum())} bytes differ'
    assert torch.equal(got[3], clips[3][frames[3]])                                 # the identity
    # every frame: clips cut to a common Ts = 3
    cut = [c[:3] for c in clips]
    got = a(cut, params=draws)
    want = _one_by_one(a, cut, None, draws)
    assert got.shape == (4, 3, 24, 24, 3) and torch.equal(got, want), f'{int((got != want).sum())} bytes differ'
    assert torch.equal(got[3], cut[3])
    # drawn here: the draws of one-clip calls on the same generator, clip by clip
    g, h = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    got = a(clips, generator=g, frames=frames)
    want = torch.cat([a(c[None], generator=h, frames=[frames[b]]) for b, c in enumerate(clips)])
    assert torch.equal(got, want)


def test_a_list_of_equal_shapes_is_the_stacked_tensor():
    from vtx import aug
    src = R.source_clip(3, 5, R.SRC_HW, seed=SEED).to(DEV)
    frames = [[0, 2, 4], [1, 1, 3], [4, 3, 0]]
    draws = aug.sample_params(3, R.SRC_HW, generator=torch.Generator().manual_seed(9))
    for pipe, kw in ((aug.ClipTest(32, short_side=36), {}), (aug.ClipEval(32), {}), (aug.ClipAugment(32), {'params': draws})):
        one = {'params': draws[1:2]} if kw else {}
        for fr in (frames, None):
            assert torch.equal(pipe(list(src), frames=fr, **kw), pipe(src, frames=fr, **kw)), (type(pipe).__name__, fr)
            assert torch.equal(pipe([src[1]], frames=fr and [fr[1]], **one), pipe(src[1][None], frames=fr and [fr[1]], **one))


def test_a_non_contiguous_entry_is_copied():
    from vtx import aug
    clips = list(_clips())
    t = aug.ClipTest(16, short_side=18)
    sliced = [clips[0][:, ::2], clips[1][:, :, 3:259], clips[2][::2], clips[3][1:]]         # rows, columns, frames; a contiguous tail
    assert not any(c.is_contiguous() for c in sliced[:3]) and sliced[3].is_contiguous()
    frames = [[4, 0], [2, 1], [0, 1], [4, 2]]
    got = t(sliced, frames=frames)
    assert torch.equal(got, t([c.contiguous() for c in sliced], frames=frames))
    assert torch.equal(got, _one_by_one(t, sliced, frames))


def test_two_calls_in_a_row_keep_their_own_tables():
    """Different geometry in consecutive calls, nothing waited for in between: each equals its own oracle."""
    from vtx import aug
    clips = list(_clips())
    t, e = aug.ClipTest(32, short_side=36), aug.ClipEval(img_size=20)
    first = t(clips, frames=FRAMES)
    second = e(clips[::-1], frames=FRAMES[::-1])
    third = t(clips[1:3], frames=FRAMES[1:3])
    torch.cuda.synchronize()
    assert torch.equal(first, _one_by_one(t, clips, FRAMES))
    assert torch.equal(second, _one_by_one(e, clips[::-1], FRAMES[::-1]))
    assert torch.equal(third, _one_by_one(t, clips[1:3], FRAMES[1:3]))


def _tables_on_device(specs, mode='bilinear', antialias=False):
    from vtx import aug
    return tuple(torch.from_numpy(a).to(DEV) for a in aug._tables(specs, mode, antialias))


def test_binding_with_host_and_device_indices_and_out():
    """vtx.ops.clips_views_u8 itself: host frames / left (validated and uploaded with the descriptor), int32 device tensors (taken
    as they are), out= with guard bytes around it; what lies behind a clip's Wr_b columns of the x table is never read."""
    from vtx import aug, ops
    clips = list(_clips())
    t = aug.ClipTest(32, short_side=36)
    xs, ys, lefts = t.specs([s[1:] for s in SHAPES])
    widths = [s[6] for s in xs]
    xf, xc, xw = aug._tables(xs, 'bilinear', False)
    for b, w in enumerate(widths):                                                   # poison behind every row's own columns
        xf[b, w:], xc[b, w:], xw[b, w:] = 10 ** 6, 2, np.nan
    xtab = tuple(torch.from_numpy(a).to(DEV) for a in (xf, xc, xw))
    ytab = _tables_on_device(ys)
    want = torch.stack([ops.clip_views_u8(c[None], [FRAMES[b]], [lefts[b].tolist()], 32,
                                          tuple(a[b:b + 1, :widths[b]].contiguous() for a in xtab), tuple(a[b:b + 1] for a in ytab))[0]
                        for b, c in enumerate(clips)])
    got = ops.clips_views_u8(clips, FRAMES, lefts, 32, xtab, ytab, widths=widths)
    assert got.shape == (4, 3, 3, 32, 32, 3) and torch.equal(got, want)
    i32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.int32, device=DEV)
    assert torch.equal(ops.clips_views_u8(clips, i32(FRAMES), i32(lefts), 32, xtab, ytab, widths=widths), want)
    n, pad = want.numel(), 4099
    buf = torch.full((pad + n + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    out = buf[pad:pad + n].view(want.shape)
    ret = ops.clips_views_u8(clips, FRAMES, lefts, 32, xtab, ytab, out=out, widths=widths)
    torch.cuda.synchronize()
    assert ret.data_ptr() == out.data_ptr() and torch.equal(out, want)
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n:] == 0xA5).all())
    # V = 1, left = 0, Wr_b = W, every frame: the plain resampler, clip by clip
    a_x, a_y = [(Ws, 0, Ws, 24, False, 0, 24) for _, _, Ws in SHAPES], [(Hs, 0, Hs, 24, False, 0, 24) for _, Hs, _ in SHAPES]
    xt, yt = _tables_on_device(a_x, 'bicubic'), _tables_on_device(a_y, 'bicubic')
    cut = [c[:3] for c in clips]
    got = ops.clips_views_u8(cut, None, [[0]] * 4, 24, xt, yt)
    for b, c in enumerate(cut):
        assert torch.equal(got[b, 0], ops.clip_resample_u8(c[None], (24, 24), tuple(a[b:b + 1] for a in xt), tuple(a[b:b + 1] for a in yt))[0])


def test_ragged_edges_of_the_band_byte_for_byte():
    """Two clips of different Ts / Hs / Ws / Wr in one launch -- 3 x 40x300 -> rows of 772 columns, 4 x 19x23 -> rows of 61 -- 13
    output rows (the last band holds 5), views of 60 columns, bicubic with antialias (clip 0: y windows of up to 15 taps), tables
    bent per clip (aug_ref.edge_table) and poisoned behind clip 1's 61 columns.  Clip 0: columns 30 .. 59 in two views, the tile
    256 .. 511 in none, 4 live lanes in the last tile; clip 1: every tile but the first is dead.  Against the float32
    restatement of the kernel (aug_ref.resample_f32) clip by clip, sliced: every byte equal."""
    from vtx import ops
    shapes, widths, H, W = [(3, 40, 300), (4, 19, 23)], [772, 61], 13, 60
    frames, lefts = [[1, 2], [2, 1]], [[0, 30, 712], [0, 1, 1]]
    clips = [R.source_clip(1, Ts, (Hs, Ws), seed=SEED + 7 + b)[0] for b, (Ts, Hs, Ws) in enumerate(shapes)]
    ytabs = [R.edge_table(Hs, H, max_taps=16, shift=b) for b, (_, Hs, _) in enumerate(shapes)]
    xtabs = [R.edge_table(Ws, widths[b], max_taps=6, shift=b) for b, (_, _, Ws) in enumerate(shapes)]
    assert int(R.kernel_windows(ytabs[0], 40)[1].max()) > 8
    xf, xc, xw = np.full((2, 772), 10 ** 6, np.int32), np.full((2, 772), 2, np.int32), np.full((2, 772, 6), np.nan, np.float32)
    for b, t in enumerate(xtabs):
        xf[b, :widths[b]], xc[b, :widths[b]], xw[b, :widths[b]] = t
    xdev = tuple(torch.from_numpy(a).to(DEV) for a in (xf, xc, xw))
    ydev = tuple(torch.from_numpy(np.stack([t[i] for t in ytabs])).to(DEV) for i in range(3))
    got = ops.clips_views_u8([c.to(DEV) for c in clips], frames, lefts, W, xdev, ydev, widths=widths)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == (2, 3, 2, H, W, 3)
    for b, c in enumerate(clips):
        whole = R.resample_f32(c[frames[b]].numpy(), ytabs[b], xtabs[b])
        want = np.stack([whole[:, :, l:l + W] for l in lefts[b]])
        assert np.array_equal(got[b], want), f'clip {b}: {int((got[b] != want).sum())} bytes differ'
        assert not got[b, :, :, 6 + b].any() and not got[b, 0, :, :, 6 + b].any() and got[b, 2, 0, 5].any()


def test_bad_lists_raise_before_any_launch_and_a_valid_call_still_works():
    from vtx import aug, ops
    clips = list(_clips())
    t = aug.ClipTest(32, short_side=36)
    xs, ys, lefts = t.specs([s[1:] for s in SHAPES])
    widths = [s[6] for s in xs]
    xtab, ytab = _tables_on_device(xs), _tables_on_device(ys)
    want = _one_by_one(t, clips, FRAMES)
    pipes = (t, aug.ClipEval(img_size=20), aug.ClipAugment(img_size=24))
    ops.profile_start(('clips_views', 'clip_views', 'clip_resample'))
    try:
        for pipe in pipes:
            with pytest.raises(TypeError, match='clip 2'):                                  # a wrong dtype inside the list
                pipe(clips[:2] + [clips[2].to(torch.int8)] + clips[3:], frames=FRAMES)
            with pytest.raises(RuntimeError, match='no CPU fallback'):                      # a CUDA / CPU mix
                pipe(clips[:3] + [clips[3].cpu()], frames=FRAMES)
            with pytest.raises(TypeError, match='host integers'):
                pipe(clips, frames=torch.tensor(FRAMES, dtype=torch.int32, device=DEV))
            with pytest.raises(ValueError, match='of clip 1 outside its 3 decoded frames'):
                pipe(clips, frames=[[4, 0, 4], [2, 3, 1], [0, 3, 3], [5, 0, 2]])
        call = lambda **kw: ops.clips_views_u8(**{**dict(clips=clips, frames=FRAMES, left=lefts, width=32, xtab=xtab, ytab=ytab, widths=widths), **kw})
        with pytest.raises(TypeError, match='clip 0'):
            call(clips=[clips[0].float()] + clips[1:])
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call(clips=[clips[0].cpu()] + clips[1:])
        with pytest.raises(TypeError, match='out must be'):                                 # an out= of the wrong shape
            call(out=torch.empty(4, 3, 3, 32, 31, 3, dtype=torch.uint8, device=DEV))
        with pytest.raises(TypeError, match='out must be'):
            call(out=torch.empty(4, 3, 3, 32, 32, 3, device=DEV))
        with pytest.raises(TypeError, match='left'):                                        # left with B - 1 rows
            call(left=lefts[:3])
        with pytest.raises(TypeError, match='left'):
            call(left=torch.tensor(lefts[:3], dtype=torch.int32, device=DEV))
        with pytest.raises(ValueError, match='left'):                                       # in range for clip 1's row, not for clip 0's
            call(left=[[0, 19, 9]] + lefts[1:].tolist())
        with pytest.raises(ValueError, match='frame indices'):
            call(frames=[[5, 0, 4]] + FRAMES[1:])
        with pytest.raises(ValueError, match='agree in length'):
            call(frames=None)
        with pytest.raises(ValueError, match='do not fit'):
            call(widths=[50, 301, 36, 51])
        with pytest.raises(ValueError, match='do not fit'):
            call(widths=[50, 300, 31, 51])
        with pytest.raises(ValueError, match='row widths'):
            call(widths=[50, 300, 36])
        with pytest.raises(ValueError, match='at most 8'):
            call(left=[[0] * 9] * 4)
        with pytest.raises(TypeError, match='a table is'):
            call(xtab=tuple(a[:3] for a in xtab))
        with pytest.raises(TypeError, match='goes with the ClipTable'):                    # a table for a list nobody checked
            call(table=torch.zeros(24, dtype=torch.int32, device=DEV))
        ct = ops.clips_table(clips, widths)
        assert ct.host.dtype == np.int32 and ct.host[8:].reshape(4, 4).tolist() == [list(s) + [w] for s, w in zip(SHAPES, widths)]
        assert ct.host[:8].view(np.uint64).tolist() == [c.data_ptr() for c in clips]
        with pytest.raises(TypeError, match='table must be'):
            call(clips=ct, widths=None, table=torch.zeros(23, dtype=torch.int32, device=DEV))
        with pytest.raises(TypeError, match='device tensors'):                             # host indices beside an uploaded table
            call(clips=ct, widths=None, table=torch.zeros(24, dtype=torch.int32, device=DEV))
        with pytest.raises(TypeError, match='carries its row widths'):
            call(clips=ct)
        torch.cuda.synchronize()
    finally:
        launched = ops.profile_stop()
    assert launched == {'clips_views': {}, 'clip_views': {}, 'clip_resample': {}}
    got = t(clips, frames=FRAMES)
    assert torch.equal(got, want)
    assert torch.equal(call().view(got.shape), want)
    assert torch.equal(call(clips=ct, widths=None).view(got.shape), want)                  # a checked list, uploaded by the binding
