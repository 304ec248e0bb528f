"""Exact parity of every kernel that takes a TABLE row map (include/vtx.h: physical row = base + m + tab[m // grp]) -- the C /
residual maps of vtx_gemm_nt, the LayerNorm kernels, vtx_row_scale_copy and the dropped-row fix-ups -- on tables no kernel can
ignore (helpers: tests/exact_tab.py, tests/exact_ln.py, tests/exact.py; premises: tests/test_exact_tab_premise.py).

The tables are the ones vtx/functions.py::_compaction_plan builds for the DropPath-compacted FFN: kept clips out of 9, irregular
steps (2, 0, 3 groups), a first entry != 0, a single group, an all-zero table, and their complements as drop tables; groups of 256
(boundaries on tile boundaries), 257 (a boundary drifting through the tile), 300 (boundaries inside 16-row passes) and 44 rows
(several boundaries per 256-row tile: map_row instead of the tile map).  Every comparison is equality against a float64 CPU
reference gathered / scattered through the index vector; outputs start as the NaN sentinel and every physical row outside the
map's image (the other clips' rows, rows before `base`, the tail) and the ld padding must stay bit-unchanged.  Buffers are large
enough for the closed form (grp, skip = max_step, base): a kernel that ignores the table fails by comparison, in bounds.
"""
import functools

import numpy as np
import pytest
import torch

import exact as X
import exact_ln as L
import exact_tab as T
from test_gpu_exact_arith import NT_FAMILIES
from test_gpu_exact_layernorm import check_bwd, check_fwd_outputs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16 = torch.bfloat16
F32 = torch.float32


def dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def bits(t):
    return t.contiguous().view(X._INT[t.dtype])


def same_bits(name, a, b):
    assert torch.equal(bits(a), bits(b)), f'{name}: differs from the identity-layout run of the same rows'


def lay_of(grp, kept):
    return T.layout(grp, kept, T.base_of(grp, kept))


def guards(buf, lay, D):
    """Sentinel regions of an output written through lay: the ld padding and every physical row outside the map's image."""
    return {'ld padding': buf[:, D:], 'unmapped rows': buf[lay.unmapped().to(buf.device), :D]}


# ------------------------------------------------------------------------------------------------------ vtx_gemm_nt
@functools.lru_cache(maxsize=None)
def _gemm_dev(grp, kept, epi, K, dtype):
    """Device operands and the expected output (CPU, in `dtype`) of one case."""
    c = T.gemm_case(grp, kept, epi, K)
    name = f'tab gemm {epi} grp={grp} kept={list(kept)} K={K}'
    if dtype == BF16:
        want = X.expect_bf16(name, c['expected'], c['kind'])
    else:
        X.assert_fp32_exact(name, c['expected'])
        want = c['expected'].float()
    N = c['N']
    d = dict(A=dev(c['A'], dtype), W=dev(c['W'], dtype), bias=dev(c['bias']), want=want, R=None, scale=None)
    if c['R'] is not None:
        d['R'] = dev(torch.cat([c['R'], T.junk((c['R'].shape[0], 8), 5)], 1), dtype)       # ldr = N + 8
    if c['scale'] is not None:
        d['scale'] = dev(c['scale'])
    return d


def run_gemm(tag, grp, kept, epi, K=T.GEMM_K, dtype=BF16):
    from vtx import ops
    c, d = T.gemm_case(grp, kept, epi, K), _gemm_dev(grp, kept, epi, K, dtype)
    M, N, clay = c['M'], c['N'], c['clay']
    kw = dict(bias=d['bias'], cmap=clay.rowmap(ops))
    if d['R'] is not None:
        kw.update(R=d['R'], ldr=N + 8, rmap=c['rlay'].rowmap(ops))
    if d['scale'] is not None:
        kw.update(row_scale=d['scale'], rs=(grp, 1, 1, 0))
    C = X.guarded((clay.phys, N), dtype, DEV)
    ops.gemm_nt(d['A'], d['W'], C, M, N, K, ldc=N + 8, **kw)
    X.check_exact(f'{tag} {epi} grp={grp} kept={list(kept)} {M}x{N}x{K}', C[clay.rows.to(DEV), :N], d['want'], guards(C, clay, N))


def run_gemm_group(tag, grp, dtype=BF16, k128=False):
    for g, kept, epi, K in T.gemm_cases((grp,)):
        if K == T.GEMM_K or k128:
            run_gemm(tag, g, kept, epi, K, dtype)


@pytest.mark.parametrize('grp', T.GROUPS)
@pytest.mark.parametrize('family', list(NT_FAMILIES))
def test_gemm_nt_table_family_exact(family, grp, vtx_opts):
    """Every bf16 family, every pattern and epilogue.  grp 44 goes through pp256 too: launch_pp sends residual maps with several
    boundaries per tile to the per-tile flow and the tile map of C falls back to map_row.  pp256 and auto (the persistent kernel
    at M >= 2048) also take K = 128, the persistent kernel's two-K-tile minimum; the rings fall back to dma2 there."""
    for k, v in NT_FAMILIES[family].items():
        vtx_opts(k, v)
    run_gemm_group(f'gemm_nt {family}', grp, k128=True)


@pytest.mark.parametrize('grp', T.GROUPS)
def test_gemm_nt_table_f32_exact(grp):
    run_gemm_group('gemm_nt f32', grp, dtype=F32, k128=True)


PP_OPTIONS = [dict(pp_grid=g, pp_cont=c, pp_epi=e) for g in ('256', '8') for c in ('0', '1') for e in ('0', '1', '4', '6')]


@pytest.mark.parametrize('grp', T.GROUPS)
@pytest.mark.parametrize('opts', PP_OPTIONS, ids=lambda o: '-'.join(f'{k}{v}' for k, v in o.items()))
def test_gemm_nt_table_pp256_options_exact(opts, grp, vtx_opts):
    """The persistent kernel under both grids, both flows (pp_cont 1: the residual-block prologue forms the tile's step from the
    table on its own) and the epilogue structures 0 (lean), 1 (per-pass), 4 (general), 6 (rolled: tables stay with the lean
    passes)."""
    vtx_opts('gemm_nt', 'pp256')
    for k, v in opts.items():
        vtx_opts(k, v)
    run_gemm_group('gemm_nt pp256 ' + ' '.join(f'{k}={v}' for k, v in opts.items()), grp, k128=True)


def test_gemm_table_rejections():
    """vtx_gemm_nt's A map and both maps of vtx_gemm_tn take the closed form only: VTX_EINVAL, nothing written."""
    from vtx import ops
    from vtx._lib import VtxError
    lay = lay_of(257, T.KEPT[0])
    M, N, K = lay.M, 64, 64
    tm = lay.rowmap(ops)
    A = dev(X.ints((lay.phys, K), -1, 1, 1.0, 1), BF16)
    W = dev(X.ints((N, K), -1, 1, 1.0, 2), BF16)
    C = X.guarded((M, N), BF16, DEV)
    with pytest.raises(VtxError, match=r'code -1'):
        ops.gemm_nt(A, W, C, M, N, K, ldc=N + 8, amap=tm)
    torch.cuda.synchronize()
    assert X.sentinel_touched(C) == 0, 'a rejected vtx_gemm_nt wrote to C'
    B2 = dev(X.ints((lay.phys, N), -1, 1, 1.0, 3), BF16)
    for kw in (dict(amap=tm), dict(bmap=tm), dict(amap=tm, bmap=tm)):
        out = X.sentinel_fill(torch.empty(K, N, dtype=F32, device=DEV))
        cs = X.sentinel_fill(torch.empty(K, dtype=F32, device=DEV))
        with pytest.raises(VtxError, match=r'code -1'):
            ops.gemm_tn(A, B2, M, K, N, out=out, colsum_out=cs, **kw)
        torch.cuda.synchronize()
        assert X.sentinel_touched(out) == 0 and X.sentinel_touched(cs) == 0, 'a rejected vtx_gemm_tn wrote to its outputs'


# -------------------------------------------------------------------------------------------------------- LayerNorm
def ident(rows):
    """The same logical rows in a compact buffer (one group, no skip, base 0)."""
    return L.Layout(rows, n=rows, skip=0, base=0)


@functools.lru_cache(maxsize=4)
def _fwd_case(rows, D, kind):
    return L.fwd_case(rows, D, kind, L.case_seed(rows, D))


@functools.lru_cache(maxsize=4)
def _bwd_case(rows, D, kind):
    return L.bwd_case(rows, D, kind, True, L.case_seed(rows, D))


def _stats_out(rows):
    return X.sentinel_fill(torch.empty(rows + 8, device=DEV)), X.sentinel_fill(torch.empty(rows + 8, device=DEV))


def _ln_fwd(c, lx, ly, dt):
    from vtx import ops
    rows, D = c['rows'], c['D']
    x = dev(lx.place(c['x'], dt, seed=2, pad=12))
    y = ly.out(D, dt, DEV)
    mean, rstd = _stats_out(rows)
    ops.layernorm_fwd(x, rows, D, D + 12, lx.rowmap(ops), dev(c['gamma']), dev(c['beta']), L.EPS, y, D + L.PAD, ly.rowmap(ops), mean, rstd)
    torch.cuda.synchronize()
    return y, mean, rstd


@pytest.mark.parametrize('grp', T.GROUPS)
@pytest.mark.parametrize('D', T.LN_D + T.LN_D_WIDE)
@pytest.mark.parametrize('kind', T.LN_FWD_KINDS)
def test_layernorm_fwd_table_exact(kind, D, grp, vtx_opts):
    """vtx_layernorm_fwd with a table xmap and a compact y (the compact FFN) and with the table on both maps, under ln_rows 1 .. 4:
    the exact_ln checks, and bit equality with the same rows in a compact buffer."""
    dt = F32 if kind == 'f32' else BF16
    for kept in T.KEPT:
        tl = lay_of(grp, kept)
        rows = tl.M
        c = _fwd_case(rows, D, kind)
        lt, li = L.Layout(rows, table=tl), ident(rows)
        y0, mean0, rstd0 = _ln_fwd(c, li, li, dt)
        for nr in ((1, 2, 3, 4) if D <= 1024 else (3,)):
            vtx_opts('ln_rows', str(nr))
            for ly in (li, lt):
                name = f"{c['name']} {tl} {'table y' if ly is lt else 'compact y'} ln_rows={nr}"
                y, mean, rstd = _ln_fwd(c, lt, ly, dt)
                check_fwd_outputs(name, c, ly, y, mean, rstd)
                same_bits(name + ' y', ly.got(y, D), li.got(y0, D))
                same_bits(name + ' mean', mean, mean0)
                same_bits(name + ' rstd', rstd, rstd0)


def _ln_acc(c, ls, ly, with_drop=None):
    """vtx_layernorm_acc_fwd with smap = omap = ls and y through ly; then, with_drop (a table layout of the dropped clips over
    the same buffers), the accumulate-only call (y = NULL) on those rows.  -> xo, y, mean, rstd, and the CPU d / xs buffers."""
    from vtx import ops
    rows, D = c['rows'], c['D']
    d = ls.place(c['d'], BF16, seed=4)
    xs = None if c['xs'] is None else ls.place(c['xs'], F32, seed=5)
    xo, y = ls.out(D, F32, DEV, pad=12), ly.out(D, BF16, DEV)
    mean, rstd = _stats_out(rows)
    dd, xsd = dev(d), None if xs is None else dev(xs)
    sm = ls.rowmap(ops)
    ops.layernorm_acc_fwd(xsd, dd, rows, D, D + L.PAD, sm, xo, D + 12, sm, dev(c['gamma']), dev(c['beta']), L.EPS, y, D + L.PAD,
                          ly.rowmap(ops), mean, rstd)
    if with_drop is not None:
        dm = with_drop.rowmap(ops)
        ops.layernorm_acc_fwd(xsd, dd, with_drop.M, D, D + L.PAD, dm, xo, D + 12, dm)
    torch.cuda.synchronize()
    return xo, y, mean, rstd, d, xs


@pytest.mark.parametrize('grp', T.GROUPS)
@pytest.mark.parametrize('D', T.LN_D)
@pytest.mark.parametrize('kind', T.LN_ACC_KINDS)
def test_layernorm_acc_fwd_table_exact(kind, D, grp):
    """vtx_layernorm_acc_fwd as FFNFn._forward_compact calls it: the kept clips through the keep table (stream in and out) with a
    compact y, with and without xs; the dropped clips through the drop table with y = NULL (accumulate only)."""
    for kept in T.KEPT:
        tl = lay_of(grp, kept)
        dl = tl.dropped()
        rows = tl.M
        c = _fwd_case(rows, D, kind)
        lt, li = L.Layout(rows, table=tl), ident(rows)
        xo0, y0, mean0, rstd0, _, _ = _ln_acc(c, li, li)
        xo, y, mean, rstd, d, xs = _ln_acc(c, lt, li, dl)
        name = f"{c['name']} {tl}"
        rest = lt.unmapped.clone()
        rest[dl.rows] = False
        X.check_exact(f'{name} xo', lt.got(xo, D), c['x'], lt.guards(xo, D, rest))
        want_drop = d[dl.rows, :D].float() + (0 if xs is None else xs[dl.rows, :D])
        X.check_exact(f'{name} xo dropped clips (y = NULL)', xo[dl.rows.to(DEV), :D], want_drop)
        check_fwd_outputs(name, c, li, y, mean, rstd)
        same_bits(name + ' xo', lt.got(xo, D), li.got(xo0, D))
        same_bits(name + ' y', y, y0)
        same_bits(name + ' mean', mean, mean0)
        same_bits(name + ' rstd', rstd, rstd0)


def _ln_bwd(c, lay):
    """One backward launch with x / dres / dx (/ dres32 / dx32) through lay and a compact dy (identity dymap)."""
    from vtx import ops
    rows, D, kind = c['rows'], c['D'], c['kind']
    tdt = F32 if kind == 'f32' else BF16
    xdt = BF16 if kind == 'bf16' else F32
    dy = dev(torch.cat([c['dy'], torch.full((rows, 4), 9.0)], 1), tdt)
    x = dev(lay.place(c['x'], xdt, seed=2, pad=12))
    junk = torch.full((3,), 77.0)
    mean, rstd = dev(torch.cat([c['mu'], junk])), dev(torch.cat([c['rs'], junk]))
    o = dict(lay=lay, dx=lay.out(D, tdt, DEV), dg=dev(c['dg0']), db=dev(c['db0']), dx32=None)
    dres = dres32 = None
    if kind == 'g32':
        dres32, o['dx32'] = dev(lay.place(c['dres'], F32, seed=3)), lay.out(D, F32, DEV)
    else:
        dres = dev(lay.place(c['dres'], tdt, seed=3))
    ops.layernorm_bwd(dy, D + 4, ops.IDENT, x, D + 12, lay.rowmap(ops), rows, D, mean, rstd, dev(c['gamma']), dres, o['dx'], D + L.PAD,
                      o['dg'], o['db'], dres32=dres32, dx32=o['dx32'])
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize('grp', T.GROUPS)
@pytest.mark.parametrize('D', T.LN_D)
@pytest.mark.parametrize('kind', T.LN_BWD_KINDS)
def test_layernorm_bwd_table_exact(kind, D, grp):
    """vtx_layernorm_bwd (F32, BF16, BF16_X32) and vtx_layernorm_bwd_g32 as FFNFn._backward_compact calls them: a table xmap
    (x, dres, dx share it), the residual gradient, a compact dy.  The exact_ln checks, and bit equality of dx, dgamma and dbeta
    with the same rows, in the same order and number, in a compact buffer."""
    for kept in T.KEPT:
        tl = lay_of(grp, kept)
        rows = tl.M
        c = _bwd_case(rows, D, kind)
        lt, li = L.Layout(rows, table=tl), ident(rows)
        o, o0 = _ln_bwd(c, lt), _ln_bwd(c, li)
        check_bwd(c, o, f' {tl}')
        name = f"{c['name']} {tl}"
        same_bits(name + ' dx', lt.got(o['dx'], D), li.got(o0['dx'], D))
        same_bits(name + ' dgamma', o['dg'], o0['dg'])
        same_bits(name + ' dbeta', o['db'], o0['db'])
        if kind == 'g32':
            same_bits(name + ' dx32', lt.got(o['dx32'], D), li.got(o0['dx32'], D))


# ----------------------------------------------------------------------------------------------- copies and fix-ups
def _out(t, dtype):
    X.assert_fp32_exact('expected', t)
    return X.rne_bf16(t) if dtype == BF16 else t.float()


@pytest.mark.parametrize('grp', T.GROUPS)
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_row_scale_copy_table_exact(dtype, grp):
    """vtx_row_scale_copy as FFNFn makes it: the gather of dout through the keep table with per-clip scales
    (_backward_compact), the pass-through copy of the dropped clips with the drop table on both sides (_copy_rows_res, and the
    forward's copy of x), and the zeroing of the dropped clips' rows (_zero_rows)."""
    from vtx import ops
    D = T.COPY_D
    for kept in T.KEPT:
        c = T.copy_case(grp, kept)
        lay = c['lay']
        dl = lay.dropped()
        e = T.copy_expected(c)
        src = dev(torch.cat([c['src'], T.junk((lay.phys, 8), 1)], 1), dtype)                  # lds = D + 8
        tag = f'row_scale_copy {lay} {dtype}'
        dz = X.guarded((lay.M + T.TAIL, D), dtype, DEV)
        ops.row_scale_copy(src, dz, lay.M, D, lds=D + 8, smap=lay.rowmap(ops), ldd=D + 8, s=dev(c['scale']), rs=(grp, 1, 1, 0))
        X.check_exact(f'{tag} gather', dz[:lay.M, :D], _out(e['gather'], dtype), {'ld padding': dz[:, D:], 'tail': dz[lay.M:, :D]})
        dm = dl.rowmap(ops)
        dst = X.guarded((lay.phys, D), dtype, DEV, pad_cols=16)
        ops.row_scale_copy(src, dst, dl.M, D, lds=D + 8, smap=dm, ldd=D + 16, dmap=dm)
        X.check_exact(f'{tag} dropped clips pass through', dst[dl.rows.to(DEV), :D], _out(c['src'].double()[dl.rows], dtype), guards(dst, dl, D))
        zero = dev(torch.zeros(1))
        dst = X.guarded((lay.phys, D), dtype, DEV, pad_cols=16)
        ops.row_scale_copy(src, dst, dl.M, D, lds=D + 8, smap=dm, ldd=D + 16, dmap=dm, s=zero, rs=(1, 0, 1, 0))
        X.check_exact(f'{tag} dropped clips zeroed', dst[dl.rows.to(DEV), :D], torch.zeros(dl.M, D, dtype=dtype), guards(dst, dl, D))


@pytest.mark.parametrize('grp', T.GROUPS)
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_dropped_rows_table_exact(dtype, grp):
    """vtx_dropped_rows_fix (out[omap(m)] = x[xmap(m)] + bias and zero[m] = 0 on the rows of the groups with s == 0) and
    vtx_dropped_rows_colsum with table maps; groups of 4 rows, the first and the last (ragged for grp 257) dropped."""
    from vtx import ops
    D = T.COPY_D
    for kept in T.KEPT:
        c = T.copy_case(grp, kept)
        lay = c['lay']
        e = T.copy_expected(c)
        drop = e['drop']
        tm = lay.rowmap(ops)
        src = dev(torch.cat([c['src'], T.junk((lay.phys, 8), 1)], 1), dtype)
        s = dev(c['s'])
        tag = f'dropped_rows {lay} {dtype}'
        out = X.guarded((lay.phys, D), dtype, DEV, pad_cols=16)
        z0 = X.ints((lay.M, D), 1, 8, 1.0, 3)
        zo = dev(z0, dtype)
        ops.dropped_rows_fix(s, lay.M, D, T.FIX_GROUP, x=src, xmap=tm, bias=dev(c['bias']), out=out, omap=tm, zero=zo, ldx=D + 8, ldo=D + 16)
        rows_d = lay.rows[drop]
        um = torch.ones(lay.phys, dtype=torch.bool)
        um[rows_d] = False
        X.check_exact(f'{tag} fix out', out[rows_d.to(DEV), :D], _out(e['fix'][drop], dtype),
                      {'ld padding': out[:, D:], 'rows of kept groups and unmapped rows': out[um.to(DEV), :D]})
        refz = z0.double().clone()
        refz[drop] = 0
        X.check_exact(f'{tag} fix zero', zo, _out(refz, dtype))
        for nparts in (1, 5):
            part = ops.dropped_rows_colsum(src, s, lay.M, D, T.FIX_GROUP, smap=tm, lds=D + 8, nparts=nparts)
            fold = ops.reduce_rows(part, 1, nparts, D, D, 0, 1, 0)
            X.check_exact(f'{tag} colsum nparts={nparts}', fold[0], _out(e['colsum'], F32))


# --------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize('grp', T.GROUPS)
def test_compaction_plan_builds_these_tables(grp):
    """_compaction_plan / _plan_maps for every pattern: the device buffer holds exactly the keep and drop tables of exact_tab
    (spare entries included) and the kept clips' scales; step_k / step_d are the largest steps; groups below 256 rows do not compact."""
    from vtx import functions as F_
    keep_scale = float(np.float32(1.0) / np.float32(0.9))
    for kept in T.KEPT:
        tl = T.layout(grp, kept, 0)
        dl = tl.dropped()
        host = torch.tensor([keep_scale * (1 + i) if i in kept else 0.0 for i in range(T.N_UNITS)], dtype=F32)
        sv = host.to(DEV)
        sv._vtx_host = host
        plan = F_._compaction_plan(sv, T.N_UNITS, grp, torch.device(DEV))
        if grp < 256:
            assert plan is None
            continue
        nk, nd, step_k, step_d, buf = plan
        assert (nk, nd, step_k, step_d) == (tl.n_groups, dl.n_groups, tl.max_step, dl.max_step)
        words = buf.cpu()
        assert words[:nk + nd + 2].view(torch.int32).tolist() == tl.tab + dl.tab
        assert torch.equal(words[nk + nd + 2:], host[list(kept)])
        kmap, dmap, sv_k = F_._plan_maps(plan, grp)
        for m, t, off in ((kmap, tl, 0), (dmap, dl, nk + 1)):
            assert (m.grp, m.skip, m.base, m.tab) == (grp, t.max_step, 0, buf.data_ptr() + 4 * off)
        assert torch.equal(sv_k.cpu(), host[list(kept)])
