"""Test-time views, host side (no GPU): the C ABI of libvtx_views.so (include/vtx_views.h), the frame sampling of
vtx.aug.sample_frames against a by-hand restatement of TemporalRandomCrop + np.linspace, and the geometry of vtx.aug.ClipTest
(Resize(short side) + ThreeCrop)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch


def test_views_library_header_and_binding_agree():
    """include/vtx_views.h, vtx/_lib.py VIEWS_SIGNATURES and the export list of libvtx_views.so name the same 3 symbols; none of
    them is declared in the other three headers; the header compiles as C99."""
    import __graft_entry__ as ge
    from helpers import ROOT
    from vtx import _lib
    ge.ensure_built()

    def declared(header):
        src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        return sorted(set(re.findall(r'\b(vtx_[a-z0-9_]+)\s*\(', src)))
    names = declared('vtx_views.h')
    assert names == sorted(_lib.VIEWS_SIGNATURES) and names == ['vtx_clip_views_u8', 'vtx_views_last_error_string', 'vtx_views_version']
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.VIEWS_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('vtx_')) == names
    for other in ('vtx.h', 'vtx_aug.h', 'vtx_randaug.h'):
        assert not set(names) & set(declared(other))
    assert _lib.load_views().vtx_views_version() >= 100
    subprocess.run(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', os.path.join(ROOT, 'include', 'vtx_views.h')], check=True)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Null pointers, non-positive sizes, more than 8 views, a view wider than the resized row, a missing frame list with T != Ts
    and src == dst: VTX_EINVAL (-1) with a reason, on a machine without a GPU -- nothing was launched."""
    from vtx import _lib
    lib = _lib.load_views()
    p = 4096                                                   # never dereferenced on the host

    def call(B=1, Ts=5, T=3, Hs=40, Ws=56, H=32, Wr=50, V=3, W=32, src=p, dst=2 * p, frames=p, left=p, tab=p, xt=2, yt=2):
        return lib.vtx_clip_views_u8(B, Ts, T, Hs, Ws, H, Wr, V, W, src, dst, frames, left, tab, tab, tab, xt, tab, tab, tab, yt, None)
    err = lib.vtx_views_last_error_string
    assert call(src=None) == -1 and b'null pointer' in err()
    assert call(left=None) == -1 and b'null pointer' in err()
    assert call(tab=None) == -1 and b'null pointer' in err()
    assert call(B=0) == -1 and b'positive' in err()
    assert call(W=-1) == -1 and call(xt=0) == -1 and call(T=0) == -1
    assert call(V=9) == -1 and b'at most 8' in err()
    assert call(W=51) == -1 and b'does not fit' in err()
    assert call(frames=None) == -1 and b'T=3, Ts=5' in err()
    assert call(dst=p) == -1 and b'in place' in err()
    assert call(B=70000, T=1, Ts=1) == -1 and b'grid' in err()


def _by_hand(total, num_frames, interval, g):
    """data_transform.py:485-489 and dataset.py:160-162, with the draw taken from a torch.Generator."""
    size = num_frames * interval
    rand_end = max(0, total - size - 1)
    begin = int(torch.randint(0, rand_end + 1, (1,), generator=g))
    end = min(begin + size, total)
    assert end - begin >= num_frames
    return begin, end, np.linspace(begin, end - 1, num_frames, dtype=int)


@pytest.mark.parametrize('total,n,interval', [(100, 8, 4), (32, 8, 4), (20, 8, 4), (8, 8, 4), (35, 8, 4)],
                         ids=['long', 'total=span', 'below-span', 'total=num_frames', 'span+3'])
def test_sample_frames_restates_temporal_random_crop(total, n, interval):
    from vtx import aug
    g, h = torch.Generator().manual_seed(17), torch.Generator().manual_seed(17)
    begins = set()
    for _ in range(64):
        got = aug.sample_frames(total, n, interval, generator=g)
        begin, end, want = _by_hand(total, n, interval, h)
        begins.add(begin)
        assert isinstance(got, np.ndarray) and got.dtype.kind == 'i' and np.array_equal(got, want)
        assert got[0] == begin and got[-1] == end - 1 and len(got) == n          # first and last index
        assert np.all(np.diff(got) >= 0) and got.min() >= 0 and got.max() < total
    assert torch.equal(g.get_state(), h.get_state())                               # one draw per call, nothing else
    rand_end = max(0, total - n * interval - 1)
    assert begins == set(range(rand_end + 1)) if rand_end <= 2 else (min(begins) >= 0 and max(begins) <= rand_end and len(begins) > 20)
    if total <= n * interval:
        assert np.array_equal(got, np.linspace(0, total - 1, n, dtype=int))        # the whole video, evenly


def test_sample_frames_raises_where_the_reference_asserts():
    from vtx import aug
    with pytest.raises(ValueError, match='shorter'):
        aug.sample_frames(7, 8, 4)
    with pytest.raises(ValueError):
        aug.sample_frames(100, 0, 4)
    with pytest.raises(ValueError):
        aug.sample_frames(100, 8, 0)


def test_clip_test_geometry_is_resize_then_three_crop():
    from vtx import aug
    t = aug.ClipTest()
    assert (t.img_size, t.short_side, t.interpolation, t.antialias, t.n_crops) == (224, 256, 'bilinear', False, 3)
    assert t.resized_hw(240, 320) == (256, 341) and t.offsets(240, 320) == (16, (0, 117, 58))
    assert t.resized_hw(320, 240) == (341, 256) and t.offsets(320, 240) == (58, (0, 32, 16))
    assert t.resized_hw(256, 340) == (256, 340) and t.offsets(256, 340) == (16, (0, 116, 58))
    s = aug.ClipTest(32, short_side=36)
    assert s.resized_hw(40, 56) == (36, 50) == aug.ClipEval(32).resized_hw(40, 56) and s.offsets(40, 56) == (2, (0, 18, 9))
    with pytest.raises(ValueError, match=r'Requested crop size 300 is bigger than input size \(256, 341\)'):
        aug.ClipTest(300).offsets(240, 320)
    with pytest.raises(ValueError, match='bigger than input size'):
        aug.ClipTest(224, short_side=200).offsets(240, 320)
    with pytest.raises(ValueError, match='interpolation'):
        aug.ClipTest(interpolation='nearest')


def test_cpu_clips_and_bad_frames_raise():
    from vtx import aug, ops
    clip = torch.zeros(1, 5, 40, 56, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        aug.ClipTest(32, short_side=36)(clip)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        aug.ClipEval(32)(clip, frames=[[0, 1]])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        aug.ClipAugment(32)(clip, frames=[[0, 1]])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.clip_views_u8(clip, None, [[0]], 32, None, None)
    # the frame list is checked on the host, before anything is uploaded
    assert aug._check_frames([0, 4], 2, 5).tolist() == [[0, 4], [0, 4]] and aug._check_frames(torch.tensor([[1], [2]]), 2, 5).dtype == np.int32
    assert np.array_equal(aug._check_frames(aug.sample_frames(5, 3, 2), 1, 5), [[0, 2, 4]])
    for bad in ([[0, 5]], [[-1, 0]]):
        with pytest.raises(ValueError, match='outside the 5 decoded frames'):
            aug._check_frames(bad, 1, 5)
    with pytest.raises(ValueError, match='rows'):
        aug._check_frames([[0], [1]], 3, 5)
    for bad in ([[0.0, 1.0]], [], [[[0]]]):
        with pytest.raises(TypeError):
            aug._check_frames(bad, 1, 5)
