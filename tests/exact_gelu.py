"""Pointwise GELU test helpers (imported by test modules; not a conftest).

The GELU of csrc/common.h (gelu_parts / gelu_erf / gelu_erf_grad / gelu_erf_both) forms erf by Abramowitz & Stegun 7.1.26
with v_rcp_f32 and v_exp_f32, two 1-ulp hardware approximations, so its fp32 value cannot be predicted bit for bit on the
CPU.  It is checked on two levels instead:

  accuracy  the fp32 kernels give the canonical values g32(x), d32(x); each is held to the float64 erf-GELU / its derivative
            within a per-element bound (`bounds`);
  identity  every bf16 kernel that inlines the function, fed pre-activations that are exactly x in fp32, stores exactly
            RNE_bf16(g32(x)) / RNE_bf16(d32(x)) (exact.check_exact, guards included).

A GEMM delivers a pre-activation exactly when the weight is the identity (each accumulator is x * 1 plus zeros) -- the
`all_bf16` generator, every bf16 value once -- or the identity plus 2^-8 on the next column, which gives pre-activations
with up to 16 significant bits (`fine_operands`): non-bf16 inputs of the function, and a rounding case for the bf16 store of
the pre-activation copy.

The bound.  Phi = the normal cdf, phi = its density, tail = Phi(-|x|):
  a(x)          = min(7.5e-8, 0.4 tail)      A&S 7.1.26 has |erf error| <= 1.5e-7, hence 7.5e-8 on the cdf; in the tail the
                                             kernel forms 0.5 erfc as poly * exp, whose error is RELATIVE to the tail and tends
                                             to 0.7779 / 0.5642 - 1 = 38 %, hence the cap 0.4 tail
  bound_gelu(x) = |x| (a + k 2^-24 Phi + 2^-126)
  bound_grad(x) = a + k 2^-24 max(Phi, |x| phi) + 2^-126
2^-126 allows for the flush of v_exp_f32's subnormal results (gelu_parts takes the exponential 2^64 higher below an argument
of -126 and scales it back, because the derivative multiplies a flushed Gaussian by |x| / sqrt(2 pi) = 5.3 at |x| = 13.2, five
times this allowance; the transcriptions below keep subnormals as that does).  k, the fp32 rounding allowance in units of
2^-24 of the dominant term, is the one measured number: the fp32 CPU transcription of the formula with correctly rounded 1/x
and exp2 needs k < 8 (K_REF, asserted in test_exact_gelu_premise.py), the GPU bar is twice that (K_GPU) for the two 1-ulp
instructions.  The float64 transcription needs k = 0 up to its own float64 roundings (3e-9 measured): that pins the constants and the branch structure of the formula
without a GPU.
"""
import math

import torch

import exact as X

BF16 = torch.bfloat16
K_REF = 8                  # what the fp32 CPU transcription (correctly rounded 1/x, exp2) has to stay within
K_GPU = 16                 # the bar of the GPU kernels: twice K_REF
SQRT2 = math.sqrt(2.0)
U24 = 2.0 ** -24
FLUSH = 2.0 ** -126

# Shapes of the GPU cases: K = N = 192 (3 K tiles: the minimum of the rings and of the persistent kernel's continuous flow) and
# 128 (2 K tiles: the persistent kernel's minimum, its non-continuous flow; the rings fall back to dma2); M = 2 * 256 + 88: a
# ragged row tile for 128- and 256-row tiles.
GELU_M = 600
GELU_KS = (192, 128)


# --------------------------------------------------------------------------------------------------- generators
def _bf16_patterns(lo, hi):
    """float32 values of the positive bf16 patterns lo <= pattern < hi (pattern << 16 is the fp32 pattern)."""
    return (torch.arange(lo, hi, dtype=torch.int32) << 16).view(torch.float32)


def all_bf16():
    """Every bf16 pattern that is +-0 or finite and normal, as float32, in pattern order (0, 0x0080 .. 0x7F7F, then the same
    with the sign bit): 65 026 values, neighbours in one binade."""
    pos = torch.cat([torch.zeros(1), _bf16_patterns(0x0080, 0x7F80)])
    return torch.cat([pos, -pos])


def bf16_subnormals():
    """The 254 bf16 subnormal patterns (reported through gelu_grad_mul, never asserted)."""
    pos = _bf16_patterns(0x0001, 0x0080)
    return torch.cat([pos, -pos])


def bf16_range(lo, hi):
    """The finite bf16 values with lo <= |x| <= hi, both signs, as float32."""
    v = all_bf16()
    return v[(v.abs() >= lo) & (v.abs() <= hi)]


def fill(vals, M, K):
    """vals (1-D) wrapped to fill [M, K]."""
    n = M * K
    return vals.repeat((n + vals.numel() - 1) // vals.numel())[:n].reshape(M, K).contiguous()


def identity_operands(M, K):
    """A = all_bf16() wrapped into [M, K], W = I: pre-activation = A exactly (x * 1 plus zeros, every A element finite)."""
    A = fill(all_bf16(), M, K)
    return A, torch.eye(K), A.double()


def fine_operands(M, K):
    """A [M, K] of bf16 values with 2^-20 <= |x| < 64 and W = I + 2^-8 on the next column (W[n, (n+1) % K] = 2^-8):
    pre[m][n] = A[m][n] + 2^-8 A[m][(n+1) % K], exact in fp32 (asserted) with up to 16 significant bits.
    Columns come in groups of four, (x, p, y, z): x walks up and down the bf16 values of the binades 2^-19 .. 2^5, p = the
    power of two of x's binade, y another value of that binade, z one of the binade below.  So
      x + 2^-8 p       is x plus exactly half a bf16 ulp: a tie (to even: up for an odd x, down for an even one),
      p + 2^-8 y       has 16 significant bits and lies in the upper half of a bf16 interval,
      y + 2^-8 z       lies in the lower half,
      z + 2^-8 x'      (x' the next group's x, one binade above z) anywhere in it.
    Rows alternate in sign.  Returns A, W (float32) and pre (float64)."""
    assert K % 4 == 0
    G = M * K // 4
    g = torch.arange(G, dtype=torch.int64)
    nx = 25 * 128                                         # x: binades -19 .. 5, 128 values each
    i = g % (2 * nx)
    idx = torch.where(i < nx, i, 2 * nx - 1 - i)
    e = (idx // 128 - 19).double()
    p = torch.exp2(e)
    x = p * (1.0 + (idx % 128).double() / 128.0)
    y = p * (1.0 + ((37 * g + 11) % 128).double() / 128.0)
    z = 0.5 * p * (1.0 + ((53 * g + 7) % 128).double() / 128.0)
    A = torch.stack([x, p, y, z], dim=1).reshape(M, K)
    A = A * torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0).double()[:, None]
    assert torch.equal(X.rne_bf16(A).double(), A), 'fine: A holds bf16 values'
    assert bool((A.abs() >= 2.0 ** -20).all()) and bool((A.abs() <= 64.0).all())
    W = torch.eye(K, dtype=torch.float64)
    W[torch.arange(K), (torch.arange(K) + 1) % K] = 2.0 ** -8
    X.assert_acc_bound('fine', A, W)
    pre = A + 2.0 ** -8 * A.roll(-1, dims=1)
    assert torch.equal(A @ W.t(), pre)
    X.assert_fp32_exact('fine pre-activation', pre)
    return A.float(), W.float(), pre


def operands(gen, M, K):
    """(A, W, pre) of the generator 'all' / 'fine'."""
    return identity_operands(M, K) if gen == 'all' else fine_operands(M, K)


def unit_operands(M, K, c):
    """The dgelu_kind = 0 case: A rows = e_0, W rows = c e_0: every accumulator is exactly c (1, -2, 0.5)."""
    A = torch.zeros(M, K)
    A[:, 0] = 1.0
    W = torch.zeros(K, K)
    W[:, 0] = c
    return A, W


def random_f32_normals(n, seed=5):
    """n random fp32 patterns restricted to finite normals (biased exponent 1 .. 254)."""
    g = X.gen(seed)
    bits = (torch.randint(1, 255, (n,), generator=g) << 23) | torch.randint(0, 1 << 23, (n,), generator=g)
    v = bits.to(torch.int32).view(torch.float32)
    return torch.where(torch.rand(n, generator=g) < 0.5, v, -v)


def f32_grid():
    """The inputs of the fp32 kernels: all_bf16(), the `fine` pre-activations, 2^16 random finite normal fp32 patterns, and
    dense stretches around the flush point of v_exp_f32 (x in [-14, -12.5]) and where the cdf rounds to 1 (x in [5, 6])."""
    fine = fine_operands(GELU_M, GELU_KS[0])[2].float().flatten()
    return torch.cat([all_bf16(), fine, random_f32_normals(1 << 16),
                      torch.linspace(-14.0, -12.5, 1 << 14), torch.linspace(5.0, 6.0, 1 << 14)])


# ------------------------------------------------------------------------------------------ float64 truth and bound
def truth(x):
    """(gelu, gelu', Phi, phi) in float64; Phi through erfc, so the tail keeps its relative accuracy."""
    x = x.double()
    Phi = 0.5 * torch.special.erfc(-x / SQRT2)
    phi = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return x * Phi, Phi + x * phi, Phi, phi


def _model(x):
    ax = x.double().abs()
    tail = 0.5 * torch.special.erfc(ax / SQRT2)
    return ax, torch.minimum(torch.full_like(ax, 7.5e-8), 0.4 * tail)


def bounds(x, k):
    """(bound_gelu, bound_grad) of the module docstring, float64."""
    ax, a = _model(x)
    _, _, Phi, phi = truth(x)
    return ax * (a + k * U24 * Phi + FLUSH), a + k * U24 * torch.maximum(Phi, ax * phi) + FLUSH


def k_needed(x, gelu=None, grad=None):
    """The smallest k at which the float values gelu / grad (of the inputs x) are inside the bound: (k_gelu, k_grad), None
    for an output that is not given.  Non-finite outputs are the caller's business (mask them first)."""
    ax, a = _model(x)
    tg, td, Phi, phi = truth(x)

    def need(got, t, base, unit):
        excess = ((got.double() - t).abs() - base).clamp_min(0.0)
        k = torch.where(excess > 0, excess / (unit * U24).clamp_min(1e-300), torch.zeros_like(excess))
        return k.max().item() if k.numel() else 0.0
    return (None if gelu is None else need(gelu, tg, ax * (a + FLUSH), ax * Phi),
            None if grad is None else need(grad, td, a + FLUSH, torch.maximum(Phi, ax * phi)))


def within(got, t, bound, dtype):
    """Mask of the elements of got (CPU) that a value inside [t - bound, t + bound] can be stored as: fp32 compares in
    float64; bf16 compares with RNE(t - bound) .. RNE(t + bound) (RNE is monotonic)."""
    g = got.double()
    if dtype == torch.float32:
        return (g - t).abs() <= bound
    return (g >= X.rne_bf16(t - bound).double()) & (g <= X.rne_bf16(t + bound).double())


def pinned_share(t, bound):
    """Share of the bf16 outputs the interval pins to a single value."""
    return (X.rne_bf16(t - bound) == X.rne_bf16(t + bound)).double().mean().item()


def check_bound(name, got, t, bound, dtype, extra=''):
    """Every element of got inside the bound around the float64 value t; one parity-report line with the pinned share (bf16)."""
    got = got.detach().cpu()
    ok = within(got, t, bound, dtype)
    bad = ~ok
    msg = ''
    if bad.any():
        where = bad.nonzero()[:6].tolist()
        msg = f' -- {int(bad.sum())} of {ok.numel()} elements outside the bound; first: ' + ', '.join(
            f'{tuple(i)}: got {got[tuple(i)].item():.9g} truth {t[tuple(i)].item():.9g} bound {bound[tuple(i)].item():.3g}'
            for i in where)
    pin = f', {pinned_share(t, bound):.1%} pinned to one value' if dtype == BF16 else ''
    X.report(f'{"FAIL" if msg else "ok  "} bound {name}: {ok.numel()} elements{pin}{extra}{msg}')
    assert not msg, f'{name}:{msg}'


# ------------------------------------------------------------------------------------- transcriptions of gelu_parts
_C = dict(rs2=0.70710678118654752, a0=0.3275911, a5=1.061405429, a4=-1.453152027, a3=1.421413741, a2=-0.284496736,
          a1=0.254829592, log2e=-1.4426950408889634, rs2pi=0.3989422804014327)


def gelu_f64(x):
    """gelu_parts / gelu_erf_both in float64, the same operation order (an fmaf is a multiply, then an add): (gelu, gelu')."""
    x = x.double()
    u = x.abs() * _C['rs2']
    t = 1.0 / (_C['a0'] * u + 1.0)
    p = _C['a5'] * t + _C['a4']
    p = p * t + _C['a3']
    p = p * t + _C['a2']
    p = p * t + _C['a1']
    uu = u * u
    gauss = torch.exp2(uu * _C['log2e'])
    q = (0.5 * p) * t
    half_tail = q * gauss
    cdf = torch.where(x >= 0, 1.0 - half_tail, half_tail)
    return x * cdf, (x * _C['rs2pi']) * gauss + cdf


def _c32(name):
    return torch.tensor(_C[name], dtype=torch.float32)


def _fma32(a, b, c):
    """fmaf: the product of two fp32 values is exact in float64; one rounding to float64 (53 bits) before the one to fp32."""
    return (a.double() * b.double() + c.double()).float()


def gelu_f32(x):
    """gelu_parts / gelu_erf_both in torch fp32, operation by operation, with the kernel's fp32 constants, a correctly rounded
    1/x for v_rcp_f32 and a correctly rounded exp2 for v_exp_f32 (both through float64): (gelu, gelu')."""
    x = x.float()
    u = x.abs() * _c32('rs2')
    t = (1.0 / _fma32(_c32('a0'), u, torch.tensor(1.0)).double()).float()
    p = _fma32(_c32('a5'), t, _c32('a4'))
    p = _fma32(p, t, _c32('a3'))
    p = _fma32(p, t, _c32('a2'))
    p = _fma32(p, t, _c32('a1'))
    uu = u * u
    gauss = torch.exp2((uu * _c32('log2e')).double()).float()
    q = (0.5 * p) * t
    half_tail = q * gauss
    cdf = torch.where(x >= 0, 1.0 - half_tail, half_tail)
    return x * cdf, _fma32(x * _c32('rs2pi'), gauss, cdf)
