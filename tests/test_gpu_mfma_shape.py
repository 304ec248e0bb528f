"""The MFMA shape of the two default bf16 GEMM kernels: what the exact-arithmetic and option-equality tests do not pin.

gemm_nt_bf16_pp_kernel issues v_mfma_f32_16x16x32_bf16 (csrc/gemm_nt.hip); gemm_tn_bf16_pp_kernel and gemm_tn_bf16_w4_kernel
issue v_mfma_f32_32x32x16_bf16 (csrc/gemm_tn.hip).  Whatever the shape, three things must hold:

  1. k-slot and lane map.  One operand is one-hot -- row m of it has a single nonzero at k = (7 m + 3) % K -- and the other holds
     small integers that differ from k to k and from column to column, so every output is a SELECTION of the other operand and
     a wrong element names the k-octet or the lane group that is wired wrong.  Everything is exact: equality.
  2. Random data against float64, with a DERIVED bound.  bf16 products are exact in fp32, so an fp32 sum of K of them, in any
     order, is within  d = K 2^-24 sum_k |a_k| |b_k|  of the exact sum (n - 1 adds, each relative 2^-24, of partial sums no
     larger than sum |a_k b_k|); a bias is a (K + 1)-th term.  Epilogues, each fp32 operation one more relative 2^-24 (u):
        plain                 e = (K + 1) u (S + |bias|)                                 S = sum_k |a_k| |b_k|
        residual + row scale  e = |s| e_plain + 2 u (|s| |pre| + |R|)                    (scale, then add)
        multiplier            e = |h| K u S + u |pre h|
        two GELU outputs      e = 1.13 e_plain + bound_gelu,  0.8 e_plain + bound_grad   (sup |gelu'| = 1.129, sup |gelu''| =
                              2 phi(0) = 0.798; bound_gelu / bound_grad: the bound tests/test_gpu_exact_gelu.py holds the
                              epilogue function to, exact_gelu.bounds at k = K_GPU, the larger of its values at pre and pre +- e)
     A bf16 output may be any value the interval [t - e, t + e] rounds to (exact_gelu.within: half a bf16 ulp at either end);
     an fp32 output (TN) is inside the interval itself.
  3. Run-to-run bit determinism: every case of 2 twice, and with pp_grid = 8 on M = 2360 -- several tiles per workgroup, so
     an accumulator that is not cleared between tiles shows.

NT shapes 600 x 320 x {192, 256, 320}: three to five K tiles (the continuous flow's minimum, and four: the rolling epilogue's), a
ragged column tile, a ragged last row tile.  TN shapes 700 x 136 x 216 (ragged everything) and 6000 x 768 x 512 at tn_cus = 64
(nine K tiles per slab plus the remainder), variants pp256 and w4, with column sums.
"""
import math

import pytest
import torch

import exact as X
import exact_gelu as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16 = torch.bfloat16
U = 2.0 ** -24
NT_M, NT_N = 600, 320
NT_KS = (192, 256, 320)
KINDS = ('plain', 'residual', 'mul', 'gelu2')
TN_SHAPES = ((700, 136, 216, '256'), (6000, 768, 512, '64'))


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(BF16)


def nt_case(M, K, kind):
    """Operands (bf16, CPU), the keyword arguments of ops.gemm_nt, and [(output name, float64 truth, bound)]."""
    N = NT_N
    A, W = rnd(M, K, seed=1), rnd(N, K, seed=2)
    Ad, Wd = A.double(), W.double()
    prod, S = Ad @ Wd.t(), Ad.abs() @ Wd.abs().t()
    bias = torch.randn(N, generator=torch.Generator().manual_seed(3))
    pre = prod + bias.double()
    e_plain = (K + 1) * U * (S + bias.double().abs())
    if kind == 'plain':
        return A, W, dict(bias=bias), [('C', pre, e_plain)]
    if kind == 'residual':
        R = rnd(M, N, seed=4)
        s = torch.rand(M, generator=torch.Generator().manual_seed(5)) + 0.5
        sd = s.double()[:, None]
        t = sd * pre + R.double()
        return A, W, dict(bias=bias, R=R, row_scale=s, rs=(1, 1, 1, 0)), [('C', t, sd * e_plain + 2 * U * (sd * pre.abs() + R.double().abs()))]
    if kind == 'mul':
        h = rnd(M, N, seed=6)
        hd = h.double()
        return A, W, dict(dgelu_in=h, dgelu_kind=1), [('C', prod * hd, hd.abs() * K * U * S + U * (prod * hd).abs())]
    assert kind == 'gelu2'
    tg, td, _, _ = G.truth(pre)
    bg = torch.stack([G.bounds(x, G.K_GPU)[0] for x in (pre, pre - e_plain, pre + e_plain)]).amax(0)
    bd = torch.stack([G.bounds(x, G.K_GPU)[1] for x in (pre, pre - e_plain, pre + e_plain)]).amax(0)
    return A, W, dict(bias=bias, act=2, C2=True), [('C', tg, 1.13 * e_plain + bg), ('C2', td, 0.8 * e_plain + bd)]


def nt_run(A, W, kw, M, K):
    from vtx import ops
    kw = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}
    C = torch.full((M, NT_N), float('nan'), dtype=BF16, device=DEV)
    out = {'C': C}
    if kw.get('C2') is True:
        kw['C2'] = out['C2'] = torch.full((M, NT_N), float('nan'), dtype=BF16, device=DEV)
    ops.gemm_nt(A.to(DEV), W.to(DEV), C, M, NT_N, K, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def hold(name, got, t, bound, dtype):
    ok = G.within(got, t, bound, dtype)
    if dtype == torch.float32:
        extra = f'largest |error| / bound {((got.double() - t).abs() / bound.clamp_min(1e-300)).max().item():.3f}'
    else:                                                   # the interval's ends round to bf16: what is left to chance is the share not pinned
        extra = f'{G.pinned_share(t, bound):.1%} pinned to one bf16 value'
    X.report(f'{"ok  " if bool(ok.all()) else "FAIL"} mfma shape {name}: {ok.numel()} elements, {extra}')
    assert bool(ok.all()), f'{name}: {int((~ok).sum())} of {ok.numel()} outside the bound, first at {(~ok).nonzero()[0].tolist()}'


# ------------------------------------------------------------------------------------------------ 1. k-slot and lane map
def test_nt_one_hot(vtx_opts):
    from vtx import ops
    vtx_opts('gemm_nt', 'pp256')
    M, N, K = NT_M, NT_N, 192
    m, n, k = torch.arange(M), torch.arange(N), torch.arange(K)
    hot = (7 * m + 3) % K
    A = torch.zeros(M, K)
    A[m, hot] = 1.0
    W = ((k[None, :] + 13 * n[:, None]) % 251 - 125).float()       # differs from k to k (K <= 251) and from column to column
    bias = (n % 7 - 3).float()
    want = W[:, hot].t() + bias                                      # |value| <= 131: exact in bf16
    C = torch.full((M, N), float('nan'), dtype=BF16, device=DEV)
    ops.gemm_nt(A.to(BF16).to(DEV), W.to(BF16).to(DEV), C, M, N, K, bias=bias.to(DEV))
    got = C.float().cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (f'{bad.shape[0]} wrong; first (m, n) = {bad[0].tolist()}: got {got[tuple(bad[0])].item():g} = W[n][k] + bias at k = '
                              f'{(got[tuple(bad[0])].item() - bias[bad[0][1]].item() + 125 - 13 * bad[0][1].item()) % 251:g}, want k = {hot[bad[0][0]].item()}')


@pytest.mark.parametrize('variant', ['pp256', 'w4'])
@pytest.mark.parametrize('M,N1,N2,cus', TN_SHAPES)
def test_tn_one_hot(M, N1, N2, cus, variant, vtx_opts):
    """Column i of A is v_i = 1 + i % 3 at token (7 i + 3) % M and zero elsewhere; B[m][j] = (m + 13 j) % 251 - 125 (the token
    index aliases every 251 rows -- prime, unrelated to the 8 / 16 / 32 / 64 structure of the K steps and tiles).  C = v_i B[m_i][j]
    and the column sums v_i are exact in fp32."""
    from vtx import ops
    vtx_opts('gemm_tn', variant)
    vtx_opts('tn_cus', cus)
    i, j, m = torch.arange(N1), torch.arange(N2), torch.arange(M)
    hot, v = (7 * i + 3) % M, (1 + i % 3).float()
    A = torch.zeros(M, N1)
    A[hot, i] = v
    B = ((m[:, None] + 13 * j[None, :]) % 251 - 125).float()
    C, cs = ops.gemm_tn(A.to(BF16).to(DEV), B.to(BF16).to(DEV), M, N1, N2, want_colsum=True)
    want = v[:, None] * B[hot]
    bad = (C.cpu() != want).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} wrong; first (i, j) = {bad[0].tolist()}: got {C.cpu()[tuple(bad[0])].item():g}, want {want[tuple(bad[0])].item():g} (token {hot[bad[0][0]].item()})'
    assert torch.equal(cs.cpu(), v), 'column sums'


# ------------------------------------------------------------------------- 2. + 3. random data: float64 bound, determinism
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('K', NT_KS)
def test_nt_random_against_float64(K, kind, vtx_opts):
    vtx_opts('gemm_nt', 'pp256')
    A, W, kw, outs = nt_case(NT_M, K, kind)
    first, second = nt_run(A, W, kw, NT_M, K), nt_run(A, W, kw, NT_M, K)
    for name, t, bound in outs:
        hold(f'nt {kind} K={K} {name}', first[name], t, bound, BF16)
        assert torch.equal(first[name].view(torch.int16), second[name].view(torch.int16)), f'{kind} K={K} {name}: two launches differ'


@pytest.mark.parametrize('kind', KINDS)
def test_nt_several_tiles_per_workgroup(kind, vtx_opts):
    """M = 2360 (ten row tiles, the last ragged) x two column tiles on eight workgroups: two or three tiles each."""
    vtx_opts('gemm_nt', 'pp256')
    vtx_opts('pp_grid', '8')
    M, K = 2360, 256
    A, W, kw, outs = nt_case(M, K, kind)
    first, second = nt_run(A, W, kw, M, K), nt_run(A, W, kw, M, K)
    for name, t, bound in outs:
        hold(f'nt {kind} M={M} grid 8 {name}', first[name], t, bound, BF16)
        assert torch.equal(first[name].view(torch.int16), second[name].view(torch.int16)), f'{kind} {name}: two launches differ'


@pytest.mark.parametrize('variant', ['pp256', 'w4'])
@pytest.mark.parametrize('M,N1,N2,cus', TN_SHAPES)
def test_tn_random_against_float64(M, N1, N2, cus, variant, vtx_opts):
    """Slab partial sums are added in fp32 as well: still one fp32 sum of M terms in some order, bound M u S; the column sum of
    column i likewise with S = sum_m |a_mi|."""
    from vtx import ops
    vtx_opts('gemm_tn', variant)
    vtx_opts('tn_cus', cus)
    A, B = rnd(M, N1, seed=1), rnd(M, N2, seed=2)
    Ad, Bd = A.double(), B.double()
    runs = []
    for _ in range(2):
        C, cs = ops.gemm_tn(A.to(DEV), B.to(DEV), M, N1, N2, want_colsum=True)
        torch.cuda.synchronize()
        runs.append((C.cpu(), cs.cpu()))
    hold(f'tn {variant} {M}x{N1}x{N2} C', runs[0][0], Ad.t() @ Bd, M * U * (Ad.abs().t() @ Bd.abs()), torch.float32)
    hold(f'tn {variant} {M}x{N1}x{N2} colsum', runs[0][1], Ad.sum(0), M * U * Ad.abs().sum(0), torch.float32)
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), 'two launches differ'
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), 'two launches differ (column sums)'


def test_bound_arithmetic():
    """The constants of the docstring: sup |gelu'| < 1.13 and sup |gelu''| < 0.8."""
    x = torch.linspace(-8, 8, 160001, dtype=torch.float64)
    _, d, _, phi = G.truth(x)
    assert d.abs().max().item() < 1.13 and ((2 - x * x) * phi).abs().max().item() < 0.8 and math.isclose(2 / math.sqrt(2 * math.pi), 0.7979, abs_tol=1e-4)
