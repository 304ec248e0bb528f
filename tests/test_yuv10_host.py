"""10-bit 4:2:0 YUV clips, host side (no GPU): the C ABI of libvtx_yuv10.so (include/vtx_yuv10.h), vtx.YUVClip(depth=10)'s
refusals, the record packer, and the premises of tests/yuv10_ref.py -- the NumPy restatement the GPU tests compare against --:
the presets against their float64 matrices over the sample set S, the x4 identity with the 8-bit contract over all 2^24
8-bit triples."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import yuv10_ref as Y10
import yuv_ref as Y

OTHERS = ('vtx.h', 'vtx_aug.h', 'vtx_randaug.h', 'vtx_views.h', 'vtx_mix.h', 'vtx_stem.h', 'vtx_ragged.h', 'vtx_dropout.h', 'vtx_yuv.h')
FIELDS = ('y', 'u', 'v', 'Ts', 'Hs', 'Ws', 'Wr', 'y_pitch', 'y_frame', 'c_pitch', 'c_frame', 'c_step', 'depth', 'shift', 'matrix', 'reserved')


def _header():
    from helpers import ROOT
    return os.path.join(ROOT, 'include', 'vtx_yuv10.h')


def test_yuv10_library_header_and_binding_agree():
    """include/vtx_yuv10.h, vtx/_lib.py YUV10_SIGNATURES and the export list of libvtx_yuv10.so name the same 4 symbols; none of
    them is declared in the other nine headers; the header compiles as C99 and its record is the 24 int32 the binding packs."""
    import __graft_entry__ as ge
    from helpers import ROOT
    from vtx import _lib
    ge.ensure_built()

    def declared(header):
        src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        return sorted(set(re.findall(r'\b(vtx_[a-z0-9_]+)\s*\(', src)))
    names = declared('vtx_yuv10.h')
    assert names == sorted(_lib.YUV10_SIGNATURES)
    assert names == ['vtx_clips_views_yuv10', 'vtx_yuv10_last_error_string', 'vtx_yuv10_to_rgb_u8', 'vtx_yuv10_version']
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.YUV10_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('vtx_')) == names
    for other in OTHERS:
        assert not set(names) & set(declared(other)), other
    assert _lib.load_yuv10().vtx_yuv10_version() >= 100
    subprocess.run(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', _header()], check=True)
    size = ('#include "%s"\n_Static_assert(sizeof(vtx_yuv10_clip) == 4 * %d && _Alignof(vtx_yuv10_clip) == 8, "record");\n'
            % (_header(), _lib.YUV10_CLIP_I32))
    subprocess.run(['gcc', '-std=c11', '-fsyntax-only', '-x', 'c', '-'], input=size, text=True, check=True)
    assert _lib.YUV10_CLIP_I32 == 24 and _lib.YUV_CLIP_I32 == 22                    # the 8-bit record stays what it was


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Null pointers, non-positive sizes, more than 8 views, a view wider than the widest resized row, more than 65535 frames and
    records that are not 8-byte aligned: VTX_EINVAL (-1) / VTX_EALIGN (-2) with the reasons vtx_clips_views_yuv420 gives, on a
    machine without a GPU -- nothing was launched, nothing dereferenced."""
    from vtx import _lib
    lib = _lib.load_yuv10()
    p = 4096                                                   # never dereferenced on the host
    err = lib.vtx_yuv10_last_error_string

    def views(B=4, T=3, H=32, V=3, W=32, Wr_max=300, clips=p, dst=2 * p, frames=p, left=p, tab=p, xt=2, yt=2):
        return lib.vtx_clips_views_yuv10(B, T, H, V, W, Wr_max, clips, dst, frames, left, tab, tab, tab, xt, tab, tab, tab, yt, None)
    for name in ('clips', 'dst', 'left', 'tab'):
        assert views(**{name: None}) == -1 and b'null pointer' in err(), name
    assert views(B=0) == -1 and b'positive' in err()
    assert views(W=-1) == -1 and views(xt=0) == -1 and views(yt=0) == -1 and views(T=0) == -1 and views(H=0) == -1 and views(Wr_max=0) == -1
    assert views(V=0) == -1 and b'positive' in err()
    assert views(V=9) == -1 and b'at most 8' in err()
    assert views(W=301) == -1 and b'does not fit' in err()
    assert views(B=21846, T=3) == -1 and b'grid' in err()
    assert views(H=8 * 65535 + 1) == -1 and b'grid' in err()
    assert views(clips=p + 4) == -2 and b'8-byte aligned' in err()
    assert err().startswith(b'clips_views_yuv10:')

    def rgb(clip=p, Ts=2, Hs=5, Ws=7, dst=2 * p):
        return lib.vtx_yuv10_to_rgb_u8(clip, Ts, Hs, Ws, dst, None)
    assert rgb(clip=None) == -1 and b'null pointer' in err()
    assert rgb(dst=None) == -1 and b'null pointer' in err()
    assert rgb(Ts=0) == -1 and b'positive' in err()
    assert rgb(Hs=-3) == -1 and rgb(Ws=0) == -1
    assert rgb(Ts=1 << 16, Hs=1 << 15) == -1 and b'2^31' in err()
    assert rgb(clip=p + 2) == -2 and b'8-byte aligned' in err()
    assert err().startswith(b'yuv10_to_rgb_u8:')


def test_yuvclip_depth10_refusals():
    """depth=10 takes int16 / uint16 planes of the 8-bit shapes; types, shapes, strides, matrices, depth and msb_aligned are
    refused on the host with the 8-bit messages where they apply; the planes of a clip that passed all of them must live on
    the device (there is no CPU fallback)."""
    import vtx
    z = lambda *s: torch.zeros(s, dtype=torch.int16)
    y, u, v, uv = z(2, 5, 7), z(2, 3, 4), z(2, 3, 4), z(2, 3, 4, 2)
    C = lambda *a, **k: vtx.YUVClip(*a, depth=10, **k)
    with pytest.raises(TypeError, match='y must be an int16 or uint16 tensor at depth=10, got torch.uint8'):
        C(y.to(torch.uint8), u, v)                             # an 8-bit plane under depth=10
    with pytest.raises(TypeError, match='u must be an int16 or uint16 tensor at depth=10, got torch.int32'):
        C(y, uv.int())
    with pytest.raises(TypeError, match='v must be an int16 or uint16 tensor'):
        C(y, u, v.numpy())
    with pytest.raises(TypeError, match='y must be a uint8 tensor, got torch.int16'):
        vtx.YUVClip(y, u, v)                                   # and 16-bit planes without it
    with pytest.raises(ValueError, match=r'y must be a non-empty \[Ts,Hs,Ws\]'):
        C(z(2, 5, 7, 1), u, v)
    with pytest.raises(ValueError, match=r'u must be \(2, 3, 4\)'):
        C(y, z(2, 2, 3), v)                                    # floor, not ceil, of the odd sizes
    with pytest.raises(ValueError, match=r'v must be \(2, 3, 4\)'):
        C(y, u, z(1, 3, 4))
    with pytest.raises(ValueError, match=r'u must be \(2, 3, 4, 2\).*v=None'):
        C(y, u)                                                # a planar U given as P010
    with pytest.raises(ValueError, match='innermost stride of y'):
        C(z(2, 5, 14)[:, :, ::2], u, v)
    with pytest.raises(ValueError, match='U and V adjacent and chroma columns 2 samples apart'):
        C(y, z(2, 3, 4, 4)[..., ::2])
    with pytest.raises(ValueError, match='share their row pitch'):
        C(y, u, z(2, 3, 6)[:, :, :4])
    with pytest.raises(ValueError, match=r'row pitch of 2 \(rows of 14 bytes\)'):
        C(torch.as_strided(z(100), (2, 5, 7), (35, 1, 1)), u, v)
    with pytest.raises(ValueError, match="'bt601', 'bt709' or six integers"):
        C(y, u, v, matrix='bt2020')
    with pytest.raises(TypeError, match='six integers'):
        C(y, u, v, matrix=(64, 1192.0, 1634, 401, 832, 2066))
    with pytest.raises(ValueError, match='0 <= y_off <= 1023'):
        C(y, u, v, matrix=(1024, 1192, 1634, 401, 832, 2066))
    with pytest.raises(ValueError, match='y_off'):
        C(y, u, v, matrix=(-1, 1192, 1634, 401, 832, 2066))
    with pytest.raises(ValueError, match=r'\|c\| <= 16384'):
        C(y, u, v, matrix=(64, 1192, 16385, 401, 832, 2066))
    with pytest.raises(ValueError, match=r'\|c\| <= 16384'):
        C(y, u, v, matrix=(64, 1192, 1634, 401, 832, -16385))
    for depth in (12, 16, 0, '10', 10.5, True, None):
        with pytest.raises(ValueError, match='depth must be 8 or 10'):
            vtx.YUVClip(y, u, v, depth=depth)
    for msb in (1, 0, 'yes', 6):
        with pytest.raises(ValueError, match='msb_aligned must be True, False or None'):
            C(y, u, v, msb_aligned=msb)
    with pytest.raises(ValueError, match='msb_aligned goes with depth=10'):
        vtx.YUVClip(y.to(torch.uint8), u.to(torch.uint8), v.to(torch.uint8), msb_aligned=True)
    # valid in every other respect: both layouts, both alignments, both dtypes, the largest matrix, padded planes
    big = (1023, 16384, -16384, 16384, -16384, 16384)
    for planes, kw in (((y, u, v), {}), ((y, uv), {}), ((y, uv), {'msb_aligned': False}), ((y, u, v), {'msb_aligned': True, 'matrix': big}),
                       ((y.view(torch.uint16), uv.view(torch.uint16)), {'matrix': 'bt709', 'full_range': True}),
                       ((z(2, 5, 16)[:, :, :7], z(2, 3, 9)[:, :, 1:5], z(2, 3, 9)[:, :, 2:6]), {})):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            C(*planes, **kw)
    with pytest.raises(RuntimeError, match='no CPU fallback'):                      # depth=8 spelled out is the default
        vtx.YUVClip(*(p.to(torch.uint8) for p in (y, u, v)), depth=8, msb_aligned=False)


def test_presets_are_yuv10_matrix_of_the_two_standards():
    from vtx import ops
    assert ops.YUV10_MATRICES == Y10.PRESETS
    for (name, full), m in Y10.PRESETS.items():
        assert ops.yuv10_matrix(*Y10.LUMA[name], full_range=full) == m, (name, full)
        assert all(isinstance(c, int) for c in ops.yuv10_matrix(*Y10.LUMA[name], full))
    assert ops.yuv10_matrix(0.2627, 0.0593) == (64, 1192, 1719, 192, 666, 2193)       # BT.2020 limited range, by hand from 4096 * k
    with pytest.raises(ValueError, match='luma weights'):
        ops.yuv10_matrix(0.7, 0.4)
    assert ops.YUV_MATRICES == Y.PRESETS                                              # the 8-bit table is what it was


def _report(name, got, want):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    differ = float((d.max(axis=-1) > 0).mean())
    print(f'{name}: max deviation {int(d.max())} step(s), {100 * differ:.3f} % of the {len(d)} triples differ in some channel')
    return int(d.max())


def test_sample_set():
    """S: 2^24 random triples, then the grid; the grid holds the ends of both ranges and the chroma centre."""
    yy, uu, vv = Y10.sample_set()
    g = len(Y10.GRID)
    assert yy.size == uu.size == vv.size == (1 << 24) + g ** 3
    assert {0, 1023, 511, 512, 513, 63, 64, 65, 939, 940, 941, 959, 960, 961, 5, 1020} <= set(Y10.GRID.tolist())
    rs = np.random.RandomState(0)
    assert np.array_equal(yy[:1 << 24], rs.randint(0, 1024, 1 << 24)) and np.array_equal(uu[:5], rs.randint(0, 1024, 1 << 24)[:5])
    for a in (yy, uu, vv):
        assert a.min() == 0 and a.max() == 1023
    assert (yy[-1], uu[-1], vv[-1]) == (1023, 1023, 1023) and (yy[1 << 24], uu[1 << 24], vv[1 << 24]) == (0, 0, 0)


@pytest.mark.parametrize('matrix,full', sorted(Y10.PRESETS))
def test_grey_axis(matrix, full):
    """U = V = 512: R = G = B; limited range maps 64 -> 0 and 940 -> 255 (and clamps outside), full range 0 -> 0 and 1023 -> 255;
    never falling."""
    g = np.arange(1024)
    rgb = Y10.convert(g, np.full(1024, 512), np.full(1024, 512), Y10.PRESETS[(matrix, full)])
    assert np.array_equal(rgb[:, 0], rgb[:, 1]) and np.array_equal(rgb[:, 1], rgb[:, 2])
    assert np.all(np.diff(rgb[:, 0].astype(int)) >= 0)
    if full:
        assert rgb[0, 0] == 0 and rgb[1023, 0] == 255
    else:
        assert rgb[64, 0] == 0 and rgb[940, 0] == 255 and not rgb[:64].any() and (rgb[940:] == 255).all()


@pytest.mark.parametrize('matrix,full', sorted(Y10.PRESETS))
def test_preset_is_within_one_step_of_the_float64_matrix(matrix, full):
    yy, uu, vv = Y10.sample_set()
    got, want = Y10.convert(yy, uu, vv, Y10.PRESETS[(matrix, full)]), Y10.convert_f64(yy, uu, vv, matrix, full)
    assert _report(f'{matrix} {"full" if full else "limited"} range against float64', got, want) <= 1


def test_times_four_identity_over_every_8bit_triple():
    """A 10-bit clip whose samples are 4 x an 8-bit clip's, with the matrix (4 * y_off, 4 * c ...), converts to exactly the 8-bit
    clip's RGB: every preset of vtx_yuv.h and a matrix at its bounds, over all 2^24 triples."""
    yy, uu, vv = Y.all_triples()
    for m in list(Y.PRESETS.values()) + [(255, 4096, -4096, 4096, -4096, 4096), (7, 301, -333, 90, 4096, 500)]:
        m4 = tuple(4 * c for c in m)
        assert 0 <= m4[0] <= 1023 and all(abs(c) <= 16384 for c in m4[1:])
        assert np.array_equal(Y10.convert(4 * yy, 4 * uu, 4 * vv, m4), Y.convert(yy, uu, vv, m)), m


def test_planes_with_pitches_shift_and_mask():
    """The addressing of the restatement itself: P010 and yuv420p10le of one 5x7 clip give the same RGB, padded planes read what
    the tight ones read, the last chroma row / column serves one luma row / column, and bits outside the sample do not count."""
    rs = np.random.RandomState(3)
    y, u, v = (rs.randint(0, 1024, s).astype(np.uint16) for s in ((2, 5, 7), (2, 3, 4), (2, 3, 4)))
    m = Y10.PRESETS[('bt709', False)]
    want = Y10.clip_to_rgb(y, u, v, m)
    assert want.shape == (2, 5, 7, 3)
    for t, s, x in ((0, 0, 0), (1, 4, 6), (0, 3, 5), (1, 2, 1)):
        assert np.array_equal(want[t, s, x], Y10.convert(y[t, s, x], u[t, s >> 1, x >> 1], v[t, s >> 1, x >> 1], m))
    stray = lambda a, lo: (rs.randint(0, 64, a.shape) << (0 if lo else 10)).astype(np.uint16)
    assert np.array_equal(Y10.clip_to_rgb((y << 6) | stray(y, True), (np.stack([u, v], axis=-1) << 6) | stray(np.stack([u, v], axis=-1), True), None, m), want)
    assert np.array_equal(Y10.clip_to_rgb(y | stray(y, False), u | stray(u, False), v | stray(v, False), m), want)
    assert np.array_equal(Y10.clip_to_rgb(y << 6, u << 6, v << 6, m, shift=6), want)        # planar and MSB-aligned
    yb, cb = np.full((3, 6, 16), 0xEEEE, np.uint16), np.full((3, 4, 11, 2), 0xEEEE, np.uint16)
    yb[:2, :5, 2:9], cb[:2, :3, 1:5, 0], cb[:2, :3, 1:5, 1] = y, u, v
    got = Y10.planes_to_rgb(yb, cb, cb, (2, 5, 7), 32, 192, 44, 176, 2, 0, m, y0=4, u0=4, v0=6)
    assert np.array_equal(got, want)


def _offsets(tmp_path):
    """offsetof() of every field of vtx_yuv10_clip, in int32 words, from a C program compiled against the header."""
    src = '#include <stdio.h>\n#include "%s"\nint main(void) {\n' % _header()
    src += ''.join('  printf("%s %%zu\\n", offsetof(vtx_yuv10_clip, %s));\n' % (f, f) for f in FIELDS) + '  return 0;\n}\n'
    exe = os.path.join(str(tmp_path), 'offsets')
    subprocess.run(['gcc', '-std=c99', '-x', 'c', '-', '-o', exe], input=src, text=True, check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    at = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()}
    assert all(o % 4 == 0 for o in at.values())
    return {f: o // 4 for f, o in at.items()}


def test_record10_matches_the_headers_offsets(tmp_path):
    """YUVClip.record10() without a device: a carrier filled by hand (the constructor insists on device planes) packs 24 int32,
    each field where offsetof() of the header's struct puts it -- pitches in bytes, the chroma step in samples, P010's V one
    sample behind U --; an 8-bit carrier packs the same record with depth 8, and its record() stays the 22 int32 it was."""
    from vtx import ops
    at = _offsets(tmp_path)
    assert [at[f] for f in FIELDS] == [0, 2, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 23]
    m = Y10.PRESETS[('bt709', True)]
    ybuf, cbuf = torch.zeros(3, 6, 16, dtype=torch.int16), torch.zeros(3, 4, 10, 2, dtype=torch.int16)
    c = object.__new__(ops.YUVClip)
    c.y, c.u, c.v, c.matrix, c.depth, c.shift = ybuf[:2, :5, 2:9], cbuf[:2][:, :3, 1:5], None, m, 10, 6
    rec = c.record10(61)
    assert rec.dtype == np.int32 and rec.shape == (24,)
    word = lambda f: int(rec[at[f]])
    ptr = lambda f: int(rec[at[f]:at[f] + 2].view(np.uint64)[0])
    assert (ptr('y'), ptr('u'), ptr('v')) == (c.y.data_ptr(), c.u.data_ptr(), c.u.data_ptr() + 2)
    assert ptr('y') == ybuf.data_ptr() + 4 and ptr('u') == cbuf.data_ptr() + 4
    assert [word(f) for f in FIELDS[3:14]] == [2, 5, 7, 61, 32, 192, 40, 160, 2, 10, 6]
    assert rec[at['matrix']:at['matrix'] + 6].tolist() == list(m) and word('reserved') == 0
    c.u, c.v, c.shift = cbuf[:2, :3, :4, 0], cbuf[:2, :3, :4, 1], 0           # not a valid planar pair (stride 2): record10() only reads bases and strides
    rec = c.record10()
    ptr = lambda f: int(rec[at[f]:at[f] + 2].view(np.uint64)[0])
    assert (ptr('u'), ptr('v')) == (c.u.data_ptr(), c.v.data_ptr()) and rec[at['Wr']] == 0 and rec[at['c_step']] == 1 and rec[at['shift']] == 0
    # an 8-bit carrier: bytes are samples
    yb8, cb8 = torch.zeros(3, 6, 16, dtype=torch.uint8), torch.zeros(3, 4, 10, 2, dtype=torch.uint8)
    c8 = object.__new__(ops.YUVClip)
    c8.y, c8.u, c8.v, c8.matrix, c8.depth, c8.shift = yb8[:2, :5, 2:9], cb8[:2][:, :3, 1:5], None, Y.PRESETS[('bt709', True)], 8, 0
    r10, r8 = c8.record10(61), c8.record(61)
    assert r8.shape == (22,) and r10.shape == (24,)
    assert r10[:15].tolist() == r8[:15].tolist() and r10[15:17].tolist() == [8, 0] and r10[17:].tolist() == r8[15:].tolist()
    assert int(r10[4:6].view(np.uint64)[0]) == c8.u.data_ptr() + 1
