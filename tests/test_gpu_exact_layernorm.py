"""Exact-arithmetic parity of the LayerNorm kernels and their partial reduce (csrc/ln.hip; helpers: tests/exact_ln.py).

Every operand lives in a [B, 1 + N, ld] buffer reached through ops.tokmap (ld = D + 8, x with D + 12: ldx != lddx), outputs are
sentinel-filled and the cls rows, the ld padding and the statistics beyond `rows` must stay bit-unchanged.  dgamma / dbeta
(non-zero on entry) are compared with equality at every D and row count; dx with equality wherever it is exact and against the
derived per-element bound elsewhere; mean_out with equality, rstd_out within 4 ulp of float64, y with equality given rstd_out.

Row counts (properties of the loops): backward and acc_fwd take two rows per wave and trip over a grid of 256 .. 1024 (backward)
or up to 2048 (acc_fwd) workgroups of 4 waves, so 20 487 and 24 581 rows give several trips whose last one has waves with two
rows, one row and none; 2032 / 2033 rows are 127 / 128 partial slabs: the 4-lane and the wide partial reduce.  The forward
kernels take ln_rows rows per trip over up to 2048 workgroups: 8193 and 32 773 rows.
Instantiations (2100 rows, the wide reduce): NCH 1 .. 4 FULL and ragged for every entry point, NCH 6 and 8 for
vtx_layernorm_fwd / vtx_layernorm_bwd; RES and no-RES for F32, BF16 and X32 (X32 up to D = 1024), G32; ln_fwd2_kernel
at NR 1 (ln_rows 1, and D > 1024) and NR 2 .. 4.  Not run: BF16_X32 at D > 1024 (ln_bwd_kernel<bf16, 6 / 8, .., float>).
"""
import functools

import pytest
import torch

import exact as X
import exact_ln as L

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16 = torch.bfloat16
F32 = torch.float32
BWD_TABLE, FWD_TABLE = frozenset(L.bwd_table()), frozenset(L.fwd_table())


def dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


@functools.lru_cache(maxsize=2)
def _bwd_case(rows, D, kind, res):
    assert (rows, D, kind, res) in BWD_TABLE, 'a case outside the table the premise test covers'
    return L.bwd_case(rows, D, kind, res, L.case_seed(rows, D))


@functools.lru_cache(maxsize=2)
def _fwd_case(rows, D, kind):
    assert (rows, D, kind) in FWD_TABLE, 'a case outside the table the premise test covers'
    return L.fwd_case(rows, D, kind, L.case_seed(rows, D))


def _stats_in(c, extra=3):
    """mean / rstd inputs of the backward with junk behind the last row."""
    junk = torch.full((extra,), 77.0)
    return dev(torch.cat([c['mu'], junk])), dev(torch.cat([c['rs'], junk]))


def launch_bwd(c, dy_mapped=False):
    """One backward launch on fresh buffers -> dict of the device outputs and the layout."""
    from vtx import ops
    rows, D, kind = c['rows'], c['D'], c['kind']
    tdt = F32 if kind == 'f32' else BF16
    xdt = BF16 if kind == 'bf16' else F32
    lay = L.Layout(rows)
    if dy_mapped:                                             # dy through a map of its own: groups of 53 rows, 2 skipped, from row 3
        lay_dy = L.Layout(rows, n=53, skip=2, base=3)
        dy, dymap = dev(lay_dy.place(c['dy'], tdt, seed=1, pad=4)), lay_dy.rowmap(ops)
    else:
        dy, dymap = dev(torch.cat([c['dy'], torch.full((rows, 4), 9.0)], 1), tdt), ops.IDENT
    x = dev(lay.place(c['x'], xdt, seed=2, pad=12))
    mean, rstd = _stats_in(c)
    o = dict(lay=lay, dx=lay.out(D, tdt, DEV), dg=dev(c['dg0']), db=dev(c['db0']), dx32=None)
    dres = dres32 = None
    if kind == 'g32':
        dres32, o['dx32'] = dev(lay.place(c['dres'], F32, seed=3)), lay.out(D, F32, DEV)
    elif c['dres'] is not None:
        dres = dev(lay.place(c['dres'], tdt, seed=3))
    ops.layernorm_bwd(dy, D + 4, dymap, x, D + 12, lay.rowmap(ops), rows, D, mean, rstd, dev(c['gamma']), dres, o['dx'], D + L.PAD,
                      o['dg'], o['db'], dres32=dres32, dx32=o['dx32'])
    torch.cuda.synchronize()
    return o


def check_bwd(c, o, tag=''):
    rows, D, kind = c['rows'], c['D'], c['kind']
    name = c['name'] + ('' if c['dres'] is not None else ' no-res') + tag
    lay, ex = o['lay'], c['exact_rows']
    X.check_exact(f'{name} dgamma', o['dg'], c['dgamma'].float())
    X.check_exact(f'{name} dbeta', o['db'], c['dbeta'].float())
    want32, want16 = L.bwd_expected_dx(c)
    ref, bound = c['dx'][~ex], c['bound'][~ex]
    dx = lay.got(o['dx'], D).cpu()
    if kind == 'g32':
        dx32 = lay.got(o['dx32'], D).cpu()
        X.check_exact(f'{name} dx32', dx32[ex], want32, lay.guards(o['dx32'], D))
        X.check_exact(f'{name} dx = rne(dx32)', dx, dx32.to(BF16), lay.guards(o['dx'], D))
        X.check_exact(f'{name} dx', dx[ex], want16)
        if ref.numel():
            L.check_bounded(f'{name} dx32 (unmirrored rows)', dx32[~ex], ref, bound)
        return
    X.check_exact(f'{name} dx', dx[ex], want32 if kind == 'f32' else want16, lay.guards(o['dx'], D))
    if ref.numel():
        L.check_bounded(f'{name} dx (unmirrored rows)', dx[~ex], ref, bound, None if kind == 'f32' else L.half_bf16_ulp(ref))


def run_bwd(rows, D, kind, res=True, dy_mapped=False):
    c = _bwd_case(rows, D, kind, res)
    check_bwd(c, launch_bwd(c, dy_mapped), ' dymap' if dy_mapped else '')


def _stats_out(rows):
    return X.sentinel_fill(torch.empty(rows + 8, device=DEV)), X.sentinel_fill(torch.empty(rows + 8, device=DEV))


def check_fwd_outputs(name, c, lay, y, mean, rstd):
    rows, D = c['rows'], c['D']
    X.check_exact(f'{name} mean', mean[:rows], c['mean'].float(), {'beyond rows': mean[rows:]})
    r = rstd[:rows].cpu()
    L.check_rstd(name, r, c['rstd'])
    X.check_exact(f'{name} y', lay.got(y, D), L.fwd_expected_y(c, r),
                  dict(lay.guards(y, D), **{'rstd beyond rows': rstd[rows:]}))


def run_fwd(rows, D, kind, ln_rows, vtx_opts):
    """vtx_layernorm_fwd under every given ln_rows, each against the reference."""
    from vtx import ops
    c = _fwd_case(rows, D, kind)
    dt = F32 if kind == 'f32' else BF16
    lay = L.Layout(rows)
    x, gamma, beta = dev(lay.place(c['x'], dt, seed=2, pad=12)), dev(c['gamma']), dev(c['beta'])
    for nr in ln_rows:
        vtx_opts('ln_rows', str(nr))
        y = lay.out(D, dt, DEV)
        mean, rstd = _stats_out(rows)
        ops.layernorm_fwd(x, rows, D, D + 12, lay.rowmap(ops), gamma, beta, L.EPS, y, D + L.PAD, lay.rowmap(ops), mean, rstd)
        torch.cuda.synchronize()
        check_fwd_outputs(f"{c['name']} ln_rows={nr}", c, lay, y, mean, rstd)


def run_acc(rows, D, kind):
    """vtx_layernorm_acc_fwd on the token rows (with y), then its accumulate-only form (y = None) on the cls rows."""
    from vtx import ops
    c = _fwd_case(rows, D, kind)
    lay = L.Layout(rows)
    d = lay.place(c['d'], BF16, seed=4)
    xs = None if c['xs'] is None else lay.place(c['xs'], F32, seed=5)
    cls = torch.arange(lay.clips) * (1 + L.TOK_N)
    xo_cls = d[cls, :D].float() + (0 if xs is None else xs[cls, :D])
    xo, y = lay.out(D, F32, DEV, pad=12), lay.out(D, BF16, DEV)
    mean, rstd = _stats_out(rows)
    tm, cm = lay.rowmap(ops), ops.clsmap(L.TOK_N)
    dd, xsd = dev(d), None if xs is None else dev(xs)
    ops.layernorm_acc_fwd(xsd, dd, rows, D, D + L.PAD, tm, xo, D + 12, tm, dev(c['gamma']), dev(c['beta']), L.EPS, y, D + L.PAD, tm,
                          mean, rstd)
    ops.layernorm_acc_fwd(xsd, dd, lay.clips, D, D + L.PAD, cm, xo, D + 12, cm)
    torch.cuda.synchronize()
    rest = lay.unmapped.clone()
    rest[cls] = False
    X.check_exact(f"{c['name']} xo", lay.got(xo, D), c['x'], lay.guards(xo, D, rest))
    X.check_exact(f"{c['name']} xo cls rows (y = None)", xo[cls.to(DEV), :D], xo_cls)
    check_fwd_outputs(c['name'], c, lay, y, mean, rstd)


# ----------------------------------------------------------------------------------------------- row-count edges
@pytest.mark.parametrize('rows', L.BWD_EDGE_ROWS)
@pytest.mark.parametrize('D', L.EDGE_D)
@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_layernorm_bwd_row_counts(kind, D, rows):
    """One trip with idle waves (1, 3, 5 rows), 127 / 128 partial slabs (the two partial reduces), several trips with a ragged
    last one.  5 and 24 581 rows read dy through a row map of its own."""
    run_bwd(rows, D, kind, dy_mapped=rows in (5, 24581))


@pytest.mark.parametrize('rows', L.BWD_EDGE_ROWS)
@pytest.mark.parametrize('D', L.EDGE_D)
def test_layernorm_acc_fwd_row_counts(D, rows):
    run_acc(rows, D, 'acc')


@pytest.mark.parametrize('rows', L.FWD_EDGE_ROWS)
@pytest.mark.parametrize('D', L.EDGE_D)
@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_layernorm_fwd_row_counts(kind, D, rows, vtx_opts):
    """ln_fwd2_kernel under ln_rows 1 (NR 1: a second trip from 8193 rows) and 2 .. 4 (32 773 rows give a second, ragged
    trip at every NR)."""
    run_fwd(rows, D, kind, (1, 2, 3, 4), vtx_opts)


@pytest.mark.parametrize('what', ['bwd bf16', 'bwd g32', 'acc_fwd'])
def test_layernorm_bench_width(what):
    """D = 768 bf16 at 24 581 rows: the width the benchmark runs, several trips."""
    if what == 'acc_fwd':
        run_acc(L.BENCH_ROWS, L.BENCH_D, 'acc')
    else:
        run_bwd(L.BENCH_ROWS, L.BENCH_D, what.split()[1])


def test_layernorm_bwd_deterministic():
    """Two launches of the 24 581-row backward: bit-identical dgamma, dbeta and dx."""
    c = _bwd_case(L.BENCH_ROWS, L.BENCH_D, 'bf16', True)
    a, b = launch_bwd(c), launch_bwd(c)
    for k, view in (('dg', torch.int32), ('db', torch.int32), ('dx', torch.int16)):
        assert torch.equal(a[k].view(view), b[k].view(view)), f'{k} differs between two launches'


# ------------------------------------------------------------------------------------------------ instantiations
@pytest.mark.parametrize('D', L.INST_D + L.INST_D_WIDE)
def test_layernorm_fwd_instantiations(D, vtx_opts):
    """NCH 1 .. 4 FULL / ragged under ln_rows 1 .. 4; D > 1024: ln_fwd2_kernel<NCH 6 / 8, NR 1> whatever ln_rows says."""
    for kind in ('f32', 'bf16'):
        run_fwd(L.INST_ROWS, D, kind, (1, 2, 3, 4) if D <= 1024 else (3,), vtx_opts)


@pytest.mark.parametrize('D', L.INST_D + L.INST_D_WIDE)
def test_layernorm_bwd_instantiations(D):
    """F32 and BF16 with and without the residual gradient at every NCH; up to D = 1024 also BF16_X32 with and without it (the
    final LayerNorm of a float32 stream has none) and G32, which always has one.  BF16_X32 at D > 1024 is not run: the
    float32 stream (vtx_layernorm_acc_fwd) ends at D = 1024."""
    for kind in ('f32', 'bf16') + (('x32',) if D <= 1024 else ()):
        for res in (True, False):
            run_bwd(L.INST_ROWS, D, kind, res)
    if D <= 1024:
        run_bwd(L.INST_ROWS, D, 'g32')


@pytest.mark.parametrize('D', L.INST_D)
def test_layernorm_acc_fwd_instantiations(D):
    """With the float32 stream and as the first sub-block (xs = None)."""
    run_acc(L.INST_ROWS, D, 'acc')
    run_acc(L.INST_ROWS, D, 'acc0')
