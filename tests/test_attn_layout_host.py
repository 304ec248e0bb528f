"""Host-side checks of vtx.functions._attn_layout (no GPU): the table AttnFn reads everything from -- attention mode and
shape fields, rows and row maps of its buffers, the cls policy -- held against the kernels' own shape rules (make_params,
csrc/attn.hip) and against itself, for every kind at small geometries, P = 1, T = 1 and the benchmark's shape."""
import ctypes

import numpy as np
import pytest

KINDS = ('self', 'space', 'time_cls', 'space_nocls')
BTP = [(2, 8, 5), (3, 8, 1), (2, 1, 4), (1, 1, 1), (8, 8, 196), (96, 8, 196)]      # (clips, frames, patches per frame)
D = 768


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.ensure_built()
    from vtx import _lib
    L = _lib.load()
    L.vtx_last_error_string.restype = ctypes.c_char_p
    return _lib, L


def _layout(kind, B, T, P):
    from vtx import functions as F_
    return F_, F_._attn_layout(kind, (B, 1 + P * T, D), 0 if kind == 'self' else T)


def _phys(rmap, m):
    """Physical row of logical row m (include/vtx.h: base + m + (m / grp) * skip, grp <= 0: base + m)."""
    return rmap.base + m + (m // rmap.grp * rmap.skip if rmap.grp > 0 else 0)


@pytest.mark.parametrize('B,T,P', BTP)
@pytest.mark.parametrize('kind', KINDS)
def test_shape_fields_pass_the_kernels_shape_rules(lib, kind, B, T, P):
    """vtx_attn_fwd accepts mode, S, L, B, T, P and stops at the next check, the null qkv pointer: nothing is launched."""
    _lib, L = lib
    _, lay = _layout(kind, B, T, P)
    d = _lib.AttnDesc()
    d.dtype, d.mode = _lib.VTX_BF16, lay.mode
    d.S, d.L, d.H, d.hd = lay.S, lay.L, D // 64, 64
    d.B, d.T, d.P = lay.B, lay.T, lay.P
    d.ld_qkv, d.ld_out, d.scale = 3 * D, D, 0.125
    assert L.vtx_attn_fwd(ctypes.byref(d), None) != 0
    assert 'qkv alignment' in L.vtx_last_error_string().decode()
    if kind == 'self':
        assert (lay.mode, lay.B, lay.T, lay.P) == (_lib.ATTN_CONTIG, 0, 0, 0)
    else:
        assert (lay.B, lay.T, lay.P) == (B, T, P)


@pytest.mark.parametrize('B,T,P', BTP)
@pytest.mark.parametrize('kind', KINDS)
def test_rows_of_every_buffer_agree(kind, B, T, P):
    F_, lay = _layout(kind, B, T, P)
    N1 = 1 + P * T
    stream_rows = B * N1
    tokens = stream_rows if kind == 'self' else B * P * T
    # o: one row per (sequence, position); the token rows first, then the split cls rows
    assert lay.S * lay.L == lay.Mo
    assert lay.tok + lay.ncls == lay.Mo and lay.tok == tokens
    per_clip = {'self': 0, 'space': T, 'time_cls': P, 'space_nocls': 0}[kind]
    assert (lay.ncls, lay.groups) == (B * per_clip, per_clip)
    assert (lay.ncls > 0) == (lay.cls == F_.CLS_MEAN)
    assert lay.cls == {'self': F_.CLS_NONE, 'space': F_.CLS_MEAN, 'time_cls': F_.CLS_MEAN, 'space_nocls': F_.CLS_PASS}[kind]
    assert lay.direct == (kind != 'self')
    # LayerNorm: every row the block attends over, read inside the stream; a 'pass' layout leaves exactly the cls rows out
    assert lay.rows == (tokens if lay.cls == F_.CLS_PASS else stream_rows)
    assert 0 <= _phys(lay.xmap, 0) and _phys(lay.xmap, lay.rows - 1) < stream_rows
    # qkv: the largest row qmap produces is inside the buffer; without a scatter the buffer is exactly the rows written
    assert _phys(lay.qmap, lay.rows - 1) < lay.qrows
    assert lay.qrows == (lay.rows if lay.qmap.grp <= 0 and lay.qmap.base == 0 else stream_rows)
    # proj output / residual: the token rows land inside the stream and never on a cls row of a layout that has cls rows
    assert _phys(lay.omap, lay.tok - 1) < stream_rows
    if kind != 'self':
        m = np.arange(lay.tok)
        phys = lay.omap.base + m + m // lay.omap.grp * lay.omap.skip
        assert (phys % N1 != 0).all() and len(np.unique(phys)) == lay.tok
    # DropPath: idx(m) = (m / d1) * m1 + (m % d2) * m2 over the token rows names every sequence and nothing beyond
    d1, m1, d2, m2 = lay.rs
    m = np.arange(lay.tok)
    idx = m // d1 * m1 + m % d2 * m2
    assert idx.min() == 0 and idx.max() == lay.S - 1 and len(np.unique(idx)) == lay.S


def test_unknown_kind_is_an_error():
    from vtx import functions as F_
    with pytest.raises(ValueError):
        F_._attn_layout('time', (2, 41, D), 8)
