"""The LayerNorm kernels and the partial-sum reduction (csrc/ln.hip) against a build of the parent commit, bit for bit, on
ordinary random data.  tests/test_gpu_exact_layernorm.py holds the rounding-sensitive outputs (rstd, the inexact dx rows)
to bounds; here every output buffer -- y, the float32 stream, statistics, dx, dx32, dgamma, dbeta, with their
sentinel-filled padding, unmapped rows and tails -- equals what the library named by VTX_PARENT_LIB computes (the
child-process mechanism of tests/test_gpu_long_attention.py; skipped when the variable names no file).

Widths and rows are the tables of tests/exact_ln.py: INST_D + INST_D_WIDE at INST_ROWS (NCH 1 .. 4 full and ragged, NCH 6
and 8, 132 partial slabs: the wide reduce), EDGE_D at 1 and 7 rows and at the second-trip counts 8193 and 32 773.
  vtx_layernorm_fwd       f32 and bf16 under ln_rows 1 .. 4 (D > 1024: the default alone)
  vtx_layernorm_acc_fwd   D <= 1024: with xs, with xs = None, and the y = None form on the cls rows
  vtx_layernorm_bwd       F32, BF16 and BF16_X32 at every width, each with and without dres; vtx_layernorm_bwd_g32 (D <= 1024)
Reduction routes through the public entry points.  No entry point reports the route; the ones named here follow from the
conditions of launch_reduce_partials (csrc/ln.hip) and tn_plan (csrc/gemm_tn.hip) as they stand, and a change of either may
move a shape to another kernel: vtx_colsum 300 x 136 (2 slabs, 136 columns: the 4-lane kernel), vtx_gemm_tn with a column
sum at 1024 x 136 x 264 (the ring keeps cdiv(264, 128) = 3 column-sum copies per slab and 136 x 264 >= 4096 weight columns:
the 16-byte kernel, whose scalar tail blocks walk the folded copies), at 1024 x 8 x 264 (8 x 264 < 4096: the 4-lane kernel
itself walks them) and at 600 x 128 x 128 (M < 1024, one copy: the 16-byte kernel, no folds), and the 2100-row backward
launches above (132 slabs of 2 D <= 4096 columns: the wide kernel).
"""
import pytest
import torch

import exact as X
import exact_ln as L
from helpers import report
from test_gpu_long_attention import _bits, parent_build_cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16, F32 = torch.bfloat16, torch.float32
DT = {'f32': F32, 'bf16': BF16}

SPEC = dict(
    fwd=[(L.INST_ROWS, D) for D in L.INST_D + L.INST_D_WIDE] + [(r, D) for D in L.EDGE_D for r in L.FWD_EDGE_ROWS],
    acc=[(L.INST_ROWS, D) for D in L.INST_D] + [(r, D) for D in L.EDGE_D for r in L.FWD_EDGE_ROWS],
    bwd=[(L.INST_ROWS, D) for D in L.INST_D + L.INST_D_WIDE] + [(r, D) for D in L.EDGE_D for r in L.FWD_EDGE_ROWS],
    colsum=[(300, 136)],
    gemm_tn=[(1024, 136, 264), (1024, 8, 264), (600, 128, 128)])


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=X.gen(seed))


def dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _fwd(res, rows, D):
    from vtx import ops
    import vtx
    lay = L.Layout(rows)
    x, gamma, beta = rnd(rows, D, seed=rows + D) * 1.5 + 0.25, rnd(D, seed=1) * 0.5 + 1.0, rnd(D, seed=2) * 0.3
    tm = lay.rowmap(ops)
    for kind, dt in DT.items():
        xd = dev(lay.place(x, dt, seed=2, pad=12))
        for nr in ((1, 2, 3, 4) if D <= 1024 else (3,)):
            vtx.set_option('ln_rows', str(nr))
            y = lay.out(D, dt, DEV)
            mean, rstd = (X.sentinel_fill(torch.empty(rows + 8, device=DEV)) for _ in range(2))
            ops.layernorm_fwd(xd, rows, D, D + 12, tm, dev(gamma), dev(beta), L.EPS, y, D + L.PAD, tm, mean, rstd)
            res[f'fwd {kind} {rows}x{D} ln_rows={nr}'] = [y.cpu(), mean.cpu(), rstd.cpu()]
    vtx.set_option('ln_rows', '3')


def _acc(res, rows, D):
    from vtx import ops
    lay = L.Layout(rows)
    d = dev(lay.place(rnd(rows, D, seed=rows + D + 1), BF16, seed=4))
    xs = dev(lay.place(rnd(rows, D, seed=rows + D + 2) * 3.0, F32, seed=5))
    gamma, beta = dev(rnd(D, seed=3) * 0.5 + 1.0), dev(rnd(D, seed=4) * 0.3)
    tm, cm = lay.rowmap(ops), ops.clsmap(L.TOK_N)
    for name, xsd in (('xs', xs), ('xs=None', None)):
        xo, y = lay.out(D, F32, DEV, pad=12), lay.out(D, BF16, DEV)
        mean, rstd = (X.sentinel_fill(torch.empty(rows + 8, device=DEV)) for _ in range(2))
        ops.layernorm_acc_fwd(xsd, d, rows, D, D + L.PAD, tm, xo, D + 12, tm, gamma, beta, L.EPS, y, D + L.PAD, tm, mean, rstd)
        ops.layernorm_acc_fwd(xsd, d, lay.clips, D, D + L.PAD, cm, xo, D + 12, cm)          # y = None: the cls rows
        res[f'acc_fwd {name} {rows}x{D}'] = [xo.cpu(), y.cpu(), mean.cpu(), rstd.cpu()]


def _bwd(res, rows, D):
    from vtx import ops
    lay = L.Layout(rows)
    tm = lay.rowmap(ops)
    x, dy, dres = rnd(rows, D, seed=rows + D + 3) * 1.5 + 0.25, rnd(rows, D, seed=rows + D + 4), rnd(rows, D, seed=rows + D + 5)
    gamma = dev(rnd(D, seed=5) * 0.5 + 1.0)
    dg0, db0 = rnd(D, seed=6), rnd(D, seed=7)
    junk = torch.full((3,), 77.0)
    kinds = ('f32', 'bf16', 'x32') + (('g32',) if D <= 1024 else ())       # the ABI of vtx_layernorm_bwd_g32 ends at D = 1024
    for kind in kinds:
        tdt = F32 if kind == 'f32' else BF16
        xdt = BF16 if kind == 'bf16' else F32
        xq = x.to(xdt).float()                                   # statistics of the row the kernel reads
        mean = xq.mean(1)
        rstd = (xq.var(1, unbiased=False) + L.EPS).rsqrt()
        xd, dyd = dev(lay.place(x, xdt, seed=2, pad=12)), dev(torch.cat([dy, torch.full((rows, 4), 9.0)], 1), tdt)
        md, rd = dev(torch.cat([mean, junk])), dev(torch.cat([rstd, junk]))
        for res_on in ((True,) if kind == 'g32' else (True, False)):
            dx, dg, db = lay.out(D, tdt, DEV), dev(dg0), dev(db0)
            out = [dx, dg, db]
            if kind == 'g32':
                dx32 = lay.out(D, F32, DEV)
                ops.layernorm_bwd(dyd, D + 4, ops.IDENT, xd, D + 12, tm, rows, D, md, rd, gamma, None, dx, D + L.PAD, dg, db,
                                  dres32=dev(lay.place(dres, F32, seed=3)), dx32=dx32)
                out.append(dx32)
            else:
                dr = dev(lay.place(dres, tdt, seed=3)) if res_on else None
                ops.layernorm_bwd(dyd, D + 4, ops.IDENT, xd, D + 12, tm, rows, D, md, rd, gamma, dr, dx, D + L.PAD, dg, db)
            res[f"bwd {kind}{'' if res_on else ' no-res'} {rows}x{D}"] = [t.cpu() for t in out]


def _reduce_routes(res, spec):
    from vtx import ops
    import vtx
    vtx.set_option('gemm_tn', 'auto')
    for M, N in spec['colsum']:
        a = dev(rnd(M, N, seed=M + N), BF16)
        acc = dev(rnd(N, seed=8))
        ops.colsum(a, M, N, out=acc, accumulate=True)
        res[f'colsum {M}x{N}'] = [ops.colsum(a, M, N).cpu(), acc.cpu()]
    for M, N1, N2 in spec['gemm_tn']:
        a, b = dev(rnd(M, N1, seed=M + N1), BF16), dev(rnd(M, N2, seed=M + N2 + 1), BF16)
        C, cs = ops.gemm_tn(a, b, M, N1, N2, want_colsum=True)
        Cacc, csacc = dev(rnd(N1, N2, seed=9)), dev(rnd(N1, seed=10))
        ops.gemm_tn(a, b, M, N1, N2, out=Cacc, accumulate=True, colsum_out=csacc, colsum_accumulate=True)
        res[f'gemm_tn {M}x{N1}x{N2}'] = [C.cpu(), cs.cpu(), Cacc.cpu(), csacc.cpu(), ops.gemm_tn(a, b, M, N1, N2).cpu()]


def ln_cases(spec):
    """{case: [every output buffer, whole, on the CPU]} of this process's library."""
    res = {}
    for rows, D in spec['fwd']:
        _fwd(res, rows, D)
    for rows, D in spec['acc']:
        _acc(res, rows, D)
    for rows, D in spec['bwd']:
        _bwd(res, rows, D)
    _reduce_routes(res, spec)
    torch.cuda.synchronize()
    return res


def test_layernorm_and_reduce_are_the_parent_bit_for_bit(tmp_path, vtx_opts):
    vtx_opts('ln_rows', '3')                                  # ln_cases sets both; put back whatever happens
    vtx_opts('gemm_tn', 'auto')
    spec = {k: [list(c) for c in v] for k, v in SPEC.items()}
    want, parent = parent_build_cases(ln_cases, spec, tmp_path)
    got = ln_cases(spec)
    assert sorted(got) == sorted(want) and len(got) > 0
    ntens = nbytes = 0
    for case in got:
        assert len(got[case]) == len(want[case]) > 0
        for i, (a, b) in enumerate(zip(got[case], want[case])):
            assert a.dtype == b.dtype and a.shape == b.shape, f'{case}: output {i}'
            assert X.sentinel_touched(a) > 0, f'{case}: output {i} was never written'
            assert torch.equal(_bits(a), _bits(b)), f'{case}: output {i} differs from the parent in {int((_bits(a) != _bits(b)).sum())} elements'
            ntens, nbytes = ntens + 1, nbytes + a.numel() * a.element_size()
    line = f'ok   ln.hip bit-identical to {parent}: {len(got)} cases, {ntens} output buffers, {nbytes / 1e6:.0f} MB compared'
    print(line)
    report(line)
