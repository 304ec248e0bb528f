"""Every kernel of csrc/gemm_tn.hip against a build of the parent commit, bit for bit, on ordinary random data.

tests/test_gpu_exact_arith.py feeds integer-valued operands, for which any summation order gives the same answer.  Here
the operands are torch.randn values from a seeded generator, so the K-tile order inside a slab, the order of the
column-sum adds, the order of the row-lane fold and which workgroup takes which column-sum copy all show in the bits.
What this build computes equals what the library named by VTX_PARENT_LIB computes (the child-process mechanism of
tests/test_gpu_long_attention.py; skipped when the variable names no file).

Cases (the shapes of tests/test_gpu_exact_arith.py):
  bf16, the seven variants (auto, pp256, w4, ring, dma2, nodma, safe) over TN_SHAPES
  pp256 and w4 at tn_cus=64 on 6000 x 768 x 512: nine K tiles per slab plus the remainder
  bf16 row maps, the seven variants: M = 6 x 788 with the token map on both operands at 256 x 512, random cls rows
    (group boundaries inside a K tile: the general branch of TnFeeder::issue_piece and advance)
  fp32 over TN_SHAPES[2:]
Each case holds five buffers: C of a plain call, (C, colsum) of a want_colsum call, (C, colsum) of an accumulating call
started from random fp32 buffers.
"""
import pytest
import torch

import exact as X
from helpers import report
from test_gpu_exact_arith import TN_SHAPES, TN_VARIANTS
from test_gpu_long_attention import _bits, parent_build_cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16, F32 = torch.bfloat16, torch.float32

DEFAULTS = dict(gemm_tn='auto', gemm_nodma='0', tn_safe='0', tn_cus='256')
VARIANTS = dict(auto=dict(gemm_tn='auto'), **TN_VARIANTS)
ROWMAP = (6, 256, 512)                                      # clips, N1, N2 of test_gemm_tn_rowmaps_exact
# (case name, dtype, options, shape or None for the row-map case)
TABLE = ([(f'bf16 {v} {M}x{N1}x{N2}', 'bfloat16', o, [M, N1, N2]) for v, o in VARIANTS.items() for M, N1, N2 in TN_SHAPES] +
         [(f'bf16 {v} tn_cus=64 6000x768x512', 'bfloat16', dict(o, tn_cus='64'), [6000, 768, 512]) for v, o in VARIANTS.items() if v in ('pp256', 'w4')] +
         [(f'bf16 {v} rowmaps', 'bfloat16', o, None) for v, o in VARIANTS.items()] +
         [(f'f32 {M}x{N1}x{N2}', 'float32', {}, [M, N1, N2]) for M, N1, N2 in TN_SHAPES[2:]])


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=X.gen(seed))


def dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _three_calls(a, b, M, N1, N2, **maps):
    from vtx import ops
    plain = ops.gemm_tn(a, b, M, N1, N2, **maps)
    C, cs = ops.gemm_tn(a, b, M, N1, N2, want_colsum=True, **maps)
    Cacc, csacc = dev(rnd(N1, N2, seed=9)), dev(rnd(N1, seed=10))
    ops.gemm_tn(a, b, M, N1, N2, out=Cacc, accumulate=True, colsum_out=csacc, colsum_accumulate=True, **maps)
    return [t.cpu() for t in (plain, C, cs, Cacc, csacc)]


def tn_cases(table):
    """{case: [plain C, C, colsum, accumulated C, accumulated colsum] on the CPU} of this process's library."""
    import vtx
    from vtx import ops
    res = {}
    try:
        for name, dtype, opts, shape in table:
            for k, v in dict(DEFAULTS, **opts).items():
                vtx.set_option(k, v)
            dt = getattr(torch, dtype)
            if shape is None:
                Bn, N1, N2 = ROWMAP
                M, tm = Bn * X.TOK_N, ops.tokmap(X.TOK_N)
                a, b = dev(rnd(Bn, 1 + X.TOK_N, N1, seed=11), dt), dev(rnd(Bn, 1 + X.TOK_N, N2, seed=12), dt)
                res[name] = _three_calls(a, b, M, N1, N2, amap=tm, bmap=tm)
            else:
                M, N1, N2 = shape
                res[name] = _three_calls(dev(rnd(M, N1, seed=M + N1), dt), dev(rnd(M, N2, seed=M + N2 + 1), dt), M, N1, N2)
        torch.cuda.synchronize()
    finally:
        for k, v in DEFAULTS.items():
            vtx.set_option(k, v)
    return res


def test_gemm_tn_is_the_parent_bit_for_bit(tmp_path):
    table = [[name, dtype, dict(opts), shape] for name, dtype, opts, shape in TABLE]
    want, parent = parent_build_cases(tn_cases, table, tmp_path)
    got = tn_cases(table)
    assert sorted(got) == sorted(want) == sorted(c[0] for c in TABLE)
    ncases = ntens = nbytes = 0
    for case in got:
        assert len(got[case]) == len(want[case]) == 5
        for i, (a, b) in enumerate(zip(got[case], want[case])):
            assert a.dtype == b.dtype == F32 and a.shape == b.shape, f'{case}: output {i}'
            assert torch.isfinite(a).all() and torch.isfinite(b).all(), f'{case}: output {i} was never written'
            assert torch.equal(_bits(a), _bits(b)), f'{case}: output {i} differs from the parent in {int((_bits(a) != _bits(b)).sum())} elements'
            ntens, nbytes = ntens + 1, nbytes + a.numel() * a.element_size()
        ncases += 1
    assert ncases == len(TABLE)
    line = f'ok   gemm_tn.hip bit-identical to {parent}: {ncases} cases, {ntens} output buffers, {nbytes / 1e6:.0f} MB compared'
    print(line)
    report(line)
