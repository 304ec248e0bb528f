"""4:2:0 YUV clips, host side (no GPU): the C ABI of libvtx_yuv.so (include/vtx_yuv.h), vtx.YUVClip's refusals, and the premises
of tests/yuv_ref.py -- the NumPy restatement the GPU tests compare against -- over all 2^24 (Y, U, V) triples."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import yuv_ref as Y


def test_yuv_library_header_and_binding_agree():
    """include/vtx_yuv.h, vtx/_lib.py YUV_SIGNATURES and the export list of libvtx_yuv.so name the same 4 symbols; none of them is
    declared in the other eight headers; the header compiles as C99 and its record is the 22 int32 the binding packs."""
    import __graft_entry__ as ge
    from helpers import ROOT
    from vtx import _lib
    ge.ensure_built()

    def declared(header):
        src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        return sorted(set(re.findall(r'\b(vtx_[a-z0-9_]+)\s*\(', src)))
    names = declared('vtx_yuv.h')
    assert names == sorted(_lib.YUV_SIGNATURES)
    assert names == ['vtx_clips_views_yuv420', 'vtx_yuv420_to_rgb_u8', 'vtx_yuv_last_error_string', 'vtx_yuv_version']
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.YUV_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('vtx_')) == names
    for other in ('vtx.h', 'vtx_aug.h', 'vtx_randaug.h', 'vtx_views.h', 'vtx_mix.h', 'vtx_stem.h', 'vtx_ragged.h', 'vtx_dropout.h'):
        assert not set(names) & set(declared(other))
    assert _lib.load_yuv().vtx_yuv_version() >= 100
    hdr = os.path.join(ROOT, 'include', 'vtx_yuv.h')
    subprocess.run(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', hdr], check=True)
    size = ('#include "%s"\n_Static_assert(sizeof(vtx_yuv420_clip) == 4 * %d && _Alignof(vtx_yuv420_clip) == 8, "record");\n'
            % (hdr, _lib.YUV_CLIP_I32))
    subprocess.run(['gcc', '-std=c11', '-fsyntax-only', '-x', 'c', '-'], input=size, text=True, check=True)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Null pointers, non-positive sizes, more than 8 views, a view wider than the widest resized row, more than 65535 frames and
    records that are not 8-byte aligned: VTX_EINVAL (-1) / VTX_EALIGN (-2) with a reason, on a machine without a GPU -- nothing
    was launched."""
    from vtx import _lib
    lib = _lib.load_yuv()
    p = 4096                                                   # never dereferenced on the host
    err = lib.vtx_yuv_last_error_string

    def views(B=4, T=3, H=32, V=3, W=32, Wr_max=300, clips=p, dst=2 * p, frames=p, left=p, tab=p, xt=2, yt=2):
        return lib.vtx_clips_views_yuv420(B, T, H, V, W, Wr_max, clips, dst, frames, left, tab, tab, tab, xt, tab, tab, tab, yt, None)
    for name in ('clips', 'dst', 'left', 'tab'):
        assert views(**{name: None}) == -1 and b'null pointer' in err(), name
    assert views(B=0) == -1 and b'positive' in err()
    assert views(W=-1) == -1 and views(xt=0) == -1 and views(yt=0) == -1 and views(T=0) == -1 and views(H=0) == -1 and views(Wr_max=0) == -1
    assert views(V=9) == -1 and b'at most 8' in err()
    assert views(W=301) == -1 and b'does not fit' in err()
    assert views(B=21846, T=3) == -1 and b'grid' in err()
    assert views(H=8 * 65535 + 1) == -1 and b'grid' in err()
    assert views(clips=p + 4) == -2 and b'8-byte aligned' in err()

    def rgb(clip=p, Ts=2, Hs=5, Ws=7, dst=2 * p):
        return lib.vtx_yuv420_to_rgb_u8(clip, Ts, Hs, Ws, dst, None)
    assert rgb(clip=None) == -1 and b'null pointer' in err()
    assert rgb(dst=None) == -1 and b'null pointer' in err()
    assert rgb(Ts=0) == -1 and b'positive' in err()
    assert rgb(Hs=-3) == -1 and rgb(Ws=0) == -1
    assert rgb(Ts=1 << 16, Hs=1 << 15) == -1 and b'2^31' in err()
    assert rgb(clip=p + 2) == -2 and b'8-byte aligned' in err()


def test_yuvclip_refusals():
    """Types, shapes, strides and matrices are refused on the host in MixedClip's style; the planes of a clip that passed all of
    them must live on the device (there is no CPU fallback)."""
    import vtx
    from vtx import aug, ops
    z = lambda *s: torch.zeros(s, dtype=torch.uint8)
    y, u, v, uv = z(2, 5, 7), z(2, 3, 4), z(2, 3, 4), z(2, 3, 4, 2)
    C = vtx.YUVClip
    with pytest.raises(TypeError, match='y must be a uint8 tensor'):
        C(y.float(), u, v)
    with pytest.raises(TypeError, match='u must be a uint8 tensor'):
        C(y, u.numpy(), v)
    with pytest.raises(TypeError, match='v must be a uint8 tensor'):
        C(y, u, v.int())
    with pytest.raises(ValueError, match=r'y must be a non-empty \[Ts,Hs,Ws\]'):
        C(z(2, 5, 7, 1), u, v)
    with pytest.raises(ValueError, match='y must be a non-empty'):
        C(z(0, 5, 7), z(0, 3, 4), z(0, 3, 4))
    with pytest.raises(ValueError, match=r'u must be \(2, 3, 4\)'):
        C(y, z(2, 2, 3), v)                                    # floor, not ceil, of the odd sizes
    with pytest.raises(ValueError, match=r'v must be \(2, 3, 4\)'):
        C(y, u, z(1, 3, 4))
    with pytest.raises(ValueError, match=r'u must be \(2, 3, 4, 2\).*NV12'):
        C(y, u)                                                # a planar U given as NV12
    with pytest.raises(ValueError, match='innermost stride of y'):
        C(z(2, 5, 14)[:, :, ::2], u, v)
    with pytest.raises(ValueError, match='innermost stride of v'):
        C(y, u, z(2, 3, 8)[:, :, ::2])
    with pytest.raises(ValueError, match='NV12 plane must have U and V adjacent'):
        C(y, z(2, 3, 2, 4).permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match='NV12 plane must have U and V adjacent'):
        C(y, z(2, 3, 4, 4)[..., ::2])
    with pytest.raises(ValueError, match='share their row pitch'):
        C(y, u, z(2, 3, 6)[:, :, :4])
    with pytest.raises(ValueError, match='row pitch'):
        C(torch.as_strided(z(100), (2, 5, 7), (35, 1, 1)), u, v)            # rows that overlap: a pitch of 1 under rows of 7 bytes
    with pytest.raises(ValueError, match="'bt601', 'bt709' or six integers"):
        C(y, u, v, matrix='bt2020')
    with pytest.raises(TypeError, match='six integers'):
        C(y, u, v, matrix=(16, 298, 409, 100, 208))
    with pytest.raises(TypeError, match='six integers'):
        C(y, u, v, matrix=(16, 298.0, 409, 100, 208, 516))
    with pytest.raises(TypeError, match='six integers'):
        C(y, u, v, matrix=7)
    with pytest.raises(ValueError, match='y_off'):
        C(y, u, v, matrix=(256, 298, 409, 100, 208, 516))
    with pytest.raises(ValueError, match='4096'):
        C(y, u, v, matrix=(16, 298, 4097, 100, 208, 516))
    for planes in ((y, u, v), (y, uv), (z(2, 5, 16)[:, :, :7], z(2, 3, 9)[:, :, 1:5], z(2, 3, 9)[:, :, 2:6])):
        with pytest.raises(RuntimeError, match='no CPU fallback'):                  # valid in every other respect
            C(*planes)
    # what takes a YUVClip says so when it gets something else, and the pipelines refuse a stray object in a list as before
    with pytest.raises(TypeError, match='a YUVClip is expected'):
        ops.yuv420_to_rgb_u8(torch.zeros(2, 5, 7, 3, dtype=torch.uint8))
    with pytest.raises(TypeError, match='YUVClip is expected, got tensors'):
        ops.clips_views_yuv([torch.zeros(2, 5, 7, 3, dtype=torch.uint8)], None, [[0]], 4, None, None)
    with pytest.raises((TypeError, ValueError)):
        ops.clips_views_yuv([], None, [[0]], 4, None, None)
    with pytest.raises(TypeError, match='clip 0'):
        aug.ClipEval(4)([object()])
    assert ops.YUV_MATRICES == Y.PRESETS


def test_record_layout_matches_the_header():
    """YUVClip.record() without a device: a carrier filled by hand (the constructor insists on device planes) packs 22 int32 --
    three pointers as little-endian pairs, Ts Hs Ws Wr, luma pitch and frame stride, chroma pitch, frame stride and step, the
    matrix, a zero -- with NV12's V one byte behind U and pitches taken from the strides of padded planes."""
    from vtx import ops
    ybuf, cbuf = torch.zeros(3, 6, 16, dtype=torch.uint8), torch.zeros(3, 4, 10, 2, dtype=torch.uint8)
    c = object.__new__(ops.YUVClip)
    c.y, c.u, c.v, c.matrix = ybuf[:, :5, 2:9], cbuf[:2][:, :3, 1:5], None, Y.PRESETS[('bt709', True)]
    c.y = c.y[:2]
    rec = c.record(61)
    assert rec.dtype == np.int32 and rec.shape == (22,)
    assert rec[:6].view(np.uint64).tolist() == [c.y.data_ptr(), c.u.data_ptr(), c.u.data_ptr() + 1]
    assert rec[6:].tolist() == [2, 5, 7, 61, 16, 96, 20, 80, 2, 0, 256, 403, 48, 120, 475, 0]
    c.u, c.v = cbuf[:2, :3, :4, 0], cbuf[:2, :3, :4, 1]          # not a valid I420 pair (stride 2): record() only reads bases and strides
    assert c.record()[:6].view(np.uint64).tolist() == [c.y.data_ptr(), c.u.data_ptr(), c.v.data_ptr()] and c.record()[9] == 0 and c.record()[14] == 1


# ---- premises of the restatement, over all 2^24 triples --------------------------------------------------------------------
def _report(name, got, want):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    differ = float((d.max(axis=-1) > 0).mean())
    print(f'{name}: max deviation {int(d.max())} step(s), {100 * differ:.3f} % of the 2^24 triples differ in some channel')
    return int(d.max())


@pytest.mark.parametrize('matrix,full', sorted(Y.PRESETS))
def test_grey_axis(matrix, full):
    """U = V = 128: R = G = B; limited range maps 16 -> 0 and 235 -> 255 (and clamps outside), full range is the identity."""
    g = np.arange(256)
    rgb = Y.convert(g, np.full(256, 128), np.full(256, 128), Y.PRESETS[(matrix, full)])
    assert np.array_equal(rgb[:, 0], rgb[:, 1]) and np.array_equal(rgb[:, 1], rgb[:, 2])
    if full:
        assert np.array_equal(rgb[:, 0], g)
    else:
        assert rgb[16, 0] == 0 and rgb[235, 0] == 255 and not rgb[:16].any() and (rgb[235:] == 255).all()
        assert np.all(np.diff(rgb[16:236, 0].astype(int)) >= 1)                   # 220 codes onto 256: strictly rising


@pytest.mark.parametrize('matrix,full', sorted(Y.PRESETS))
def test_preset_is_within_one_step_of_the_float64_matrix(matrix, full):
    yy, uu, vv = Y.all_triples()
    got, want = Y.convert(yy, uu, vv, Y.PRESETS[(matrix, full)]), Y.convert_f64(yy, uu, vv, matrix, full)
    assert _report(f'{matrix} {"full" if full else "limited"} range against float64', got, want) <= 1


def test_full_range_601_is_within_one_step_of_pillow():
    from PIL import Image
    yy, uu, vv = Y.all_triples()
    ycc = np.stack([yy, uu, vv], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    want = np.asarray(Image.frombytes('YCbCr', (4096, 4096), ycc.tobytes()).convert('RGB')).reshape(-1, 3)
    got = Y.convert(yy, uu, vv, Y.PRESETS[('bt601', True)])
    assert _report('bt601 full range against Pillow YCbCr -> RGB', got, want) <= 1


def test_planes_with_pitches_and_odd_sizes():
    """The addressing of the restatement itself: NV12 and I420 of one 5x7 clip give the same RGB, padded planes read what the
    tight ones read, and the last chroma row / column serves one luma row / column."""
    rs = np.random.RandomState(3)
    y, u, v = rs.randint(0, 256, (2, 5, 7)), rs.randint(0, 256, (2, 3, 4)), rs.randint(0, 256, (2, 3, 4))
    y, u, v = (a.astype(np.uint8) for a in (y, u, v))
    m = Y.PRESETS[('bt709', False)]
    want = Y.clip_to_rgb(y, u, v, m)
    assert want.shape == (2, 5, 7, 3)
    assert np.array_equal(Y.clip_to_rgb(y, np.stack([u, v], axis=-1), None, m), want)
    for t, s, x in ((0, 0, 0), (1, 4, 6), (0, 3, 5), (1, 2, 1)):
        assert np.array_equal(want[t, s, x], Y.convert(y[t, s, x], u[t, s >> 1, x >> 1], v[t, s >> 1, x >> 1], m))
    yb, cb = np.full((3, 6, 16), 0xEE, np.uint8), np.full((3, 4, 11, 2), 0xEE, np.uint8)
    yb[:2, :5, 2:9], cb[:2, :3, 1:5, 0], cb[:2, :3, 1:5, 1] = y, u, v
    got = Y.planes_to_rgb(yb, cb, cb, (2, 5, 7), 16, 96, 22, 88, 2, m, y0=2, u0=2, v0=3)
    assert np.array_equal(got, want)
