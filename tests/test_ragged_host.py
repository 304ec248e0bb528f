"""Clips of differing source size, host side (no GPU): the C ABI of libvtx_ragged.so (include/vtx_ragged.h), the draws of
vtx.aug.sample_params for per-clip frame sizes, ClipTest's padded x tables and the host checks of a list of clips."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

#: (Ts, Hs, Ws) of tests/test_gpu_ragged.py: landscape, a row longer than one 256-column tile, portrait, odd sizes
SHAPES = [(5, 40, 56), (3, 36, 300), (4, 56, 40), (6, 33, 47)]
SIZES = [s[1:] for s in SHAPES]


def test_ragged_library_header_and_binding_agree():
    """include/vtx_ragged.h, vtx/_lib.py RAGGED_SIGNATURES and the export list of libvtx_ragged.so name the same 3 symbols; none
    of them is declared in the other six headers; the header compiles as C99."""
    import __graft_entry__ as ge
    from helpers import ROOT
    from vtx import _lib
    ge.ensure_built()

    def declared(header):
        src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        return sorted(set(re.findall(r'\b(vtx_[a-z0-9_]+)\s*\(', src)))
    names = declared('vtx_ragged.h')
    assert names == sorted(_lib.RAGGED_SIGNATURES) and names == ['vtx_clips_views_u8', 'vtx_ragged_last_error_string', 'vtx_ragged_version']
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.RAGGED_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('vtx_')) == names
    for other in ('vtx.h', 'vtx_aug.h', 'vtx_randaug.h', 'vtx_views.h', 'vtx_mix.h', 'vtx_stem.h'):
        assert not set(names) & set(declared(other))
    assert _lib.load_ragged().vtx_ragged_version() >= 100
    subprocess.run(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', os.path.join(ROOT, 'include', 'vtx_ragged.h')], check=True)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Null pointers, non-positive sizes, more than 8 views, a view wider than the widest resized row, more than 65535 frames and a
    pointer table that is not 8-byte aligned: VTX_EINVAL (-1) / VTX_EALIGN (-2) with a reason, on a machine without a GPU --
    nothing was launched."""
    from vtx import _lib
    lib = _lib.load_ragged()
    p = 4096                                                   # never dereferenced on the host

    def call(B=4, T=3, H=32, V=3, W=32, Wr_max=300, src=p, geom=p, dst=2 * p, frames=p, left=p, tab=p, xt=2, yt=2):
        return lib.vtx_clips_views_u8(B, T, H, V, W, Wr_max, src, geom, dst, frames, left, tab, tab, tab, xt, tab, tab, tab, yt, None)
    err = lib.vtx_ragged_last_error_string
    for name in ('src', 'geom', 'dst', 'left', 'tab'):
        assert call(**{name: None}) == -1 and b'null pointer' in err(), name
    assert call(B=0) == -1 and b'positive' in err()
    assert call(W=-1) == -1 and call(xt=0) == -1 and call(T=0) == -1 and call(H=0) == -1 and call(Wr_max=0) == -1
    assert call(V=9) == -1 and b'at most 8' in err()
    assert call(W=301) == -1 and b'does not fit' in err()
    assert call(B=21846, T=3) == -1 and b'grid' in err()
    assert call(src=p + 4) == -2 and b'8-byte aligned' in err()


@pytest.mark.parametrize('kw', [dict(color_jitter=0.4), dict(auto_augment=True, out_hw=(24, 24))], ids=['jitter', 'randaug'])
def test_draws_for_per_clip_sizes_are_those_of_successive_one_clip_calls(kw):
    from vtx import aug
    g, h = torch.Generator().manual_seed(23), torch.Generator().manual_seed(23)
    got = aug.sample_params(4, SIZES, generator=g, **kw)
    want = [d for hw in SIZES for d in aug.sample_params(1, hw, generator=h, **kw)]
    assert len(got) == 4 and got == want
    assert torch.equal(g.get_state(), h.get_state())
    for d, (Hs, Ws) in zip(got, SIZES):                        # each box lies in its own clip's frame
        assert 0 <= d.top and d.top + d.height <= Hs and 0 <= d.left and d.left + d.width <= Ws
    assert all(len(d.randaug) == 2 and not d.ops for d in got) if 'auto_augment' in kw else all(len(d.ops) == 3 for d in got)
    # a single size still means: every clip alike
    g, h = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    assert aug.sample_params(3, (40, 56), generator=g, **kw) == aug.sample_params(3, [(40, 56)] * 3, generator=h, **kw)
    with pytest.raises(ValueError, match='sizes'):
        aug.sample_params(3, SIZES, **kw)


@pytest.mark.parametrize('mode,antialias', [('bilinear', False), ('bilinear', True)])
def test_clip_test_pads_each_x_table_to_the_widest_row(mode, antialias):
    """ClipTest(32, short_side=36): the resized rows hold 50, 300, 36 and 51 columns.  Row b of the stacked x table is
    ops.resample_table of clip b alone on its first Wr_b entries (weights zero behind that table's own tap count) and has
    count 0 behind them."""
    from vtx import aug, ops
    t = aug.ClipTest(32, short_side=36, interpolation=mode, antialias=antialias)
    xs, ys, lefts = t.specs(SIZES)
    widths = [s[6] for s in xs]
    assert widths == [50, 300, 36, 51] == [t.resized_hw(*hw)[1] for hw in SIZES]
    assert lefts.dtype == np.int32 and lefts.tolist() == [[0, w - 32, (w - 32) // 2] for w in widths]
    first, count, weights = aug._tables(xs, mode, antialias)
    taps = max(ops.resample_max_taps(Ws, Wr, mode, antialias) for (_, Ws), Wr in zip(SIZES, widths))
    assert first.shape == count.shape == (4, 300) and weights.shape == (4, 300, taps)
    for b, ((_, Ws), Wr) in enumerate(zip(SIZES, widths)):
        f, c, w = ops.resample_table(Ws, 0, Ws, Wr, mode, antialias)
        assert np.array_equal(first[b, :Wr], f) and np.array_equal(count[b, :Wr], c) and np.all(c > 0)
        assert np.array_equal(weights[b, :Wr, :w.shape[1]], w) and not weights[b, :Wr, w.shape[1]:].any()
        assert not count[b, Wr:].any() and not first[b, Wr:].any() and not weights[b, Wr:].any()
    yf, yc, yw = aug._tables(ys, mode, antialias)
    assert yf.shape == (4, 32) and np.all(yc > 0)              # the y tables: 32 rows for every clip, none padded
    for b, (Hs, _) in enumerate(SIZES):
        Hr = t.resized_hw(*SIZES[b])[0]
        f, c, w = ops.resample_table(Hs, 0, Hs, Hr, mode, antialias)
        top = (Hr - 32) // 2
        assert np.array_equal(yf[b], f[top:top + 32]) and np.array_equal(yw[b, :, :w.shape[1]], w[top:top + 32])
    with pytest.raises(ValueError, match=r'bigger than input size \(36, 50\) \(clip 0, 40x56\)'):
        aug.ClipTest(40, short_side=36).specs([(40, 56), (80, 100)])


def test_a_list_is_checked_on_the_host():
    from vtx import aug, ops
    clips = [torch.zeros(s + (3,), dtype=torch.uint8) for s in SHAPES]
    frames = [[4, 0, 4], [2, 2, 1], [0, 3, 3], [5, 0, 2]]
    pipes = (aug.ClipTest(32, short_side=36), aug.ClipEval(20), aug.ClipAugment(24))
    assert ops.clip_list_shapes(clips, 't') == SHAPES
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.clips_table(clips, [50, 300, 36, 51])
    for pipe in pipes:
        with pytest.raises(RuntimeError, match='no CPU fallback'):                 # valid in every other respect
            pipe(clips, frames=frames)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            pipe(tuple(c[:3] for c in clips))
        with pytest.raises((TypeError, ValueError), match='empty'):
            pipe([])
        with pytest.raises((TypeError, ValueError), match='clip 1'):               # a 5-D element
            pipe([clips[0], clips[1][None]], frames=[0, 1])
        with pytest.raises((TypeError, ValueError), match='clip 2'):               # a float element
            pipe(clips[:2] + [clips[2].float()] + clips[3:], frames=frames)
        with pytest.raises((TypeError, ValueError), match='clip 0'):               # not a tensor
            pipe([clips[0].numpy()], frames=[0])
        with pytest.raises((TypeError, ValueError), match='clip 1'):               # two channels
            pipe([clips[0], clips[1][..., :2]], frames=[0])
        for bad in ([[4, 0, 4], [2, 3, 1], [0, 3, 3], [5, 0, 2]], [[4, 0, 4], [2, 2, 1], [0, 3, -1], [5, 0, 2]]):
            with pytest.raises((TypeError, ValueError), match='of clip [12] outside its [34] decoded frames'):
                pipe(clips, frames=bad)                                            # in range for its neighbours, not for its own clip
        with pytest.raises((TypeError, ValueError), match='outside its 3 decoded frames'):
            pipe(clips, frames=[0, 3])                                             # one row for all: checked against every clip
        with pytest.raises((TypeError, ValueError), match='lengths must agree'):
            pipe(clips)                                                            # differing Ts_b without frames
        with pytest.raises((TypeError, ValueError), match='rows'):
            pipe(clips, frames=frames[:3])
        with pytest.raises(TypeError):
            pipe(clips, frames=[[4, 0, 4], [2, 2], [0, 3, 3], [5, 0, 2]])          # rows of different length
        with pytest.raises(TypeError):
            pipe(clips, frames=[[0.0, 1.0]] * 4)
    with pytest.raises(ValueError, match=r'of clip 0 \(40x56\) is smaller than the 20x20 crop'):
        aug.ClipEval(20, crop_pct=1.25)(clips, frames=frames)                      # Resize(16), then a 20x20 crop
    with pytest.raises(ValueError, match='bigger than input size'):
        aug.ClipTest(40, short_side=36)(clips, frames=frames)
    with pytest.raises(ValueError, match='outside the 36x300 frame'):              # a box that fits clip 0's frame, given to clip 1
        aug.ClipAugment(24)(clips, frames=frames, params=[aug.ClipDraw(0, 0, 40, 56, False, (), ())] * 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.clips_views_u8(clips, frames, [[0, 18, 9]] * 4, 32, None, None)
    for bad in ([], clips[0], [clips[0][None]], [clips[0].int()]):
        with pytest.raises((TypeError, ValueError)):
            ops.clips_views_u8(bad, None, [[0]], 32, None, None)
    assert aug._check_frames_ragged([1, 2], [3, 5]).tolist() == [[1, 2], [1, 2]]
    assert aug._check_frames_ragged(torch.tensor([[2], [4]]), [3, 5]).dtype == np.int32
    assert aug._check_frames_ragged(None, [4, 4, 4]) is None
