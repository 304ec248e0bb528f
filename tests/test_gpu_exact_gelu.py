"""The GELU epilogues over every bf16 input, through every kernel that inlines the function (helpers: tests/exact_gelu.py).

Level 1, accuracy: the fp32 kernels -- vtx_gemm_nt in fp32 with act = 1 / 2 and vtx_gelu_grad_mul in fp32 -- give the canonical
fp32 values g32(x) and d32(x); they are held to the float64 erf-GELU and its derivative within the per-element bound of
exact_gelu.py at k = K_GPU = 16, and to each other bit for bit (gelu_erf, gelu_erf_grad and gelu_erf_both of csrc/common.h).
Level 2, identity: every bf16 kernel family, fed pre-activations that are exactly x in fp32 (identity weights, no bias), stores
exactly RNE_bf16(g32(x)) and RNE_bf16(d32(x)): the bit-identity promise of common.h, the rounding of the bf16 stores, the
element order of the packed pairs and every dispatch branch, guards included.  Every bf16 output is also held to float64
within the same bound, so it is tied to the truth and not only to the fp32 kernel.

The comment on a case names the branch of vtx_gemm_nt (csrc/gemm_nt.hip) it reaches; the families are those of
test_gpu_exact_arith.py.  K = N = 192 has 3 K tiles (the rings; the persistent kernel's continuous flow), K = N = 128 has 2
(the persistent kernel's per-tile flow; the rings fall back to gemm_nt_bf16_dma_kernel); M = 600 = 2 * 256 + 88.
"""
import functools
import types

import pytest
import torch

import exact as X
import exact_gelu as G
from test_gpu_exact_arith import NT_FAMILIES

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16 = torch.bfloat16
F32 = torch.float32
M0 = G.GELU_M
M_TOK = X.TOK_B * X.TOK_N                    # 2364 token rows through the token map (3 clips of 1 + 788 rows)
M_PP = 2360                                  # 10 row tiles of the persistent kernel (9 * 256 + 56): several tiles per workgroup at pp_grid = 8
KC = 192


def dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _set(vtx_opts, opts):
    for k, v in opts.items():
        vtx_opts(k, v)


# ------------------------------------------------------------------------------------------------ canonical fp32 values
def _f32_gemm_act(x2d, act):
    """vtx_gemm_nt in fp32 (gemm_nt_f32_kernel, the generic epilogue<float>) of x2d [M, K] with W = I and the activation:
    C [M, K + 8 guard columns], C2 [M + 3 guard rows, K] and the guard regions."""
    from vtx import ops
    M, K = x2d.shape
    C = X.guarded((M, K), F32, DEV)
    C2 = X.sentinel_fill(torch.empty(M + 3, K, dtype=F32, device=DEV))
    ops.gemm_nt(dev(x2d), dev(torch.eye(K)), C, M, K, K, ldc=K + 8, act=act, C2=C2)
    return C, C2, {'ldc pad': C[:, K:], 'C2 tail': C2[M:]}


def canon(pre):
    """(g32, d32) of the fp32 CPU tensor pre, from the fp32 GEMM with act = 2 (zero-padded to whole rows of 192)."""
    flat = pre.flatten()
    n = flat.numel()
    Mc = (n + KC - 1) // KC
    buf = torch.zeros(Mc * KC)
    buf[:n] = flat
    C, C2, _ = _f32_gemm_act(buf.reshape(Mc, KC), 2)
    g = C[:, :KC].cpu().flatten()[:n].reshape(pre.shape)
    d = C2[:Mc].cpu().flatten()[:n].reshape(pre.shape)
    return g, d


@functools.lru_cache(maxsize=None)
def _case(gen, M, K):
    """Operands, exact pre-activations, the canonical values of the fp32 kernel on them, the float64 truth and the bound
    at K_GPU: computed once per module."""
    A, W, pre = G.operands(gen, M, K)
    g32, d32 = canon(pre.float())
    tg, td, _, _ = G.truth(pre)
    bg, bd = G.bounds(pre, G.K_GPU)
    pre_bf16 = X.expect_bf16(f'{gen} {M}x{K} pre-activation copy', pre, 'round') if gen == 'fine' else X.rne_bf16(pre)
    return types.SimpleNamespace(A=A, W=W, pre=pre, g32=g32, d32=d32, tg=tg, td=td, bg=bg, bd=bd, pre_bf16=pre_bf16)


def _both(name, got, want32, t, b, guards=()):
    """Identity with the canonical fp32 values rounded to bf16, and the float64 bound."""
    X.check_exact(name, got, want32.to(BF16), guards)
    G.check_bound(name, got, t, b, BF16)


def test_canonical_f32_inside_bound():
    """Level 1 on f32_grid(): the fp32 GEMM with act = 1 (C = gelu, C2 = the pre-activation copy) and act = 2 (C = gelu,
    C2 = gelu') and gelu_grad_mul in fp32 with dy = 1.  C and C2 inside the bound at k = 16; act = 1 and act = 2 give the same
    C; gelu_grad_mul(1, x) equals the act = 2 C2 (gelu_erf_grad against gelu_erf_both); the pre-activation copy equals x
    (all by equality: +0 matches -0, the GEMM's x * 1 + 0 turns -0 into +0).  The report lines carry the smallest k that
    would have passed."""
    from vtx import ops
    grid = G.f32_grid()
    M = (grid.numel() + KC - 1) // KC
    x = G.fill(grid, M, KC)
    C1, P1, guards1 = _f32_gemm_act(x, 1)
    C, D, guards2 = _f32_gemm_act(x, 2)
    g, d = C[:, :KC].cpu(), D[:M].cpu()
    tg, td, _, _ = G.truth(x)
    bg, bd = G.bounds(x, G.K_GPU)
    kg, kd = G.k_needed(x, g, d)
    G.check_bound('gemm_nt f32 act=2 gelu', g, tg, bg, F32, extra=f', smallest k {kg:.2f} (bar {G.K_GPU})')
    G.check_bound("gemm_nt f32 act=2 gelu'", d, td, bd, F32, extra=f', smallest k {kd:.2f} (bar {G.K_GPU})')
    X.check_exact('gemm_nt f32 act=2 guards', C[:, :KC], g, guards2)
    X.check_exact('gemm_nt f32 act=1 gelu == act=2 gelu', C1[:, :KC], g, guards1)
    X.check_exact('gemm_nt f32 act=1 pre-activation copy == x', P1[:M], x)
    n = x.numel()
    out = X.sentinel_fill(torch.empty(n + 8, dtype=F32, device=DEV))
    ops.gelu_grad_mul(torch.ones(n, device=DEV), dev(x).flatten(), out[:n])
    X.check_exact("gelu_grad_mul f32 dy=1 == act=2 gelu' (gelu_erf_grad == gelu_erf_both)", out[:n], d.flatten(), {'tail': out[n:]})
    kd2 = G.k_needed(x.flatten(), None, out[:n].cpu())[1]
    G.check_bound("gelu_grad_mul f32 gelu'", out[:n].cpu(), td.flatten(), bd.flatten(), F32, extra=f', smallest k {kd2:.2f} (bar {G.K_GPU})')


@functools.lru_cache(maxsize=None)
def _flat_case():
    """all_bf16() wrapped to a multiple of 8 elements, its canonical gelu' and the truth."""
    v = G.all_bf16()
    h = G.fill(v, 1, (v.numel() + 7) // 8 * 8).flatten()
    _, d32 = canon(h)
    _, td, _, _ = G.truth(h)
    return h, d32, td, G.bounds(h, G.K_GPU)[1]


def test_gelu_grad_mul_f32_scalings_and_second_trip():
    """gelu_grad_mul in fp32 with dy = -2 and 0.5 (exact scalings of d32), and once with n8 = 2^22 + 1 > 16384 * 256, so the
    grid-stride loop makes a second trip: 2^25 + 8 elements, h zero except its first and last 4096 (the all_bf16() prefix),
    dy = 2^((i / 8) % 16 - 8) so that an element taken from another position shows; compared on the device (h, dy, out and the
    expected values are 128 MB each, the index and comparison temporaries about as much again: some 0.8 GB in flight)."""
    from vtx import ops
    h, d32, td, bd = _flat_case()
    assert h[0] == 0
    n = h.numel()
    for dy in (-2.0, 0.5):
        out = X.sentinel_fill(torch.empty(n + 8, dtype=F32, device=DEV))
        ops.gelu_grad_mul(torch.full((n,), dy, device=DEV), dev(h), out[:n])
        X.check_exact(f'gelu_grad_mul f32 dy={dy:g}', out[:n], dy * d32, {'tail': out[n:]})
        G.check_bound(f'gelu_grad_mul f32 dy={dy:g}', out[:n].cpu(), dy * td, abs(dy) * bd, F32)
    n = (1 << 25) + 8
    hl = torch.zeros(n, device=DEV)
    hl[:4096] = dev(h[:4096])
    hl[-4096:] = dev(h[:4096])
    dy = torch.exp2((((torch.arange(n, dtype=torch.int32, device=DEV) >> 3) & 15) - 8).float())
    want = dy * dev(d32[:1])                                         # h = 0: the canonical gelu'(0) (all_bf16() starts with +0)
    want[:4096] = dy[:4096] * dev(d32[:4096])
    want[-4096:] = dy[-4096:] * dev(d32[:4096])
    out = torch.full((n,), float('nan'), device=DEV)
    ops.gelu_grad_mul(dy, hl, out)
    nbad = int((out != want).sum().item())
    first = (out != want).nonzero()[:4].flatten().tolist()
    del hl, dy, want, out
    torch.cuda.empty_cache()
    X.report(f'{"FAIL" if nbad else "ok  "} exact gelu_grad_mul f32 n=2^25+8 (second grid-stride trip): {n} elements'
             + (f' -- {nbad} differ, first at {first}' if nbad else ''))
    assert nbad == 0, f'{nbad} elements differ, first at {first}'


def test_gelu_specials():
    """NaN in gives NaN out (asserted: the fp32 GEMM epilogue through a NaN bias, gelu_grad_mul in both types).  What the
    kernels return at +-Inf, for bf16 subnormals and for fp32 subnormals is reported only: gelu(-Inf) = -Inf * 0 is NaN in
    this formula, and whether a subnormal survives is a property of the hardware mode."""
    from vtx import ops
    sub = G.bf16_subnormals()
    spec = torch.zeros(KC)
    vals = torch.tensor([float('nan'), float('inf'), float('-inf'), 2.0 ** -127, -2.0 ** -127, 2.0 ** -133, 2.0 ** -140, 2.0 ** -149])
    spec[:vals.numel()] = vals
    M = 8
    C = X.guarded((M, KC), F32, DEV)
    C2 = X.sentinel_fill(torch.empty(M + 3, KC, dtype=F32, device=DEV))
    ops.gemm_nt(torch.zeros(M, KC, device=DEV), dev(torch.eye(KC)), C, M, KC, KC, ldc=KC + 8, act=2, C2=C2, bias=dev(spec))
    g, d = C[0, :KC].cpu(), C2[0].cpu()
    for i, v in enumerate(vals.tolist()):
        X.report(f'info gelu specials (fp32 epilogue, pre-activation = bias): x={v:g} gelu={g[i].item():g} gelu\'={d[i].item():g}')
    assert bool(torch.isnan(g[0])) and bool(torch.isnan(d[0])), 'NaN in, NaN out'
    n = 256
    for dtype in (F32, BF16):
        h = torch.zeros(n)
        h[:254] = sub
        h[254] = float('nan')
        h[255] = float('inf')
        out = torch.empty(n, dtype=dtype, device=DEV)
        ops.gelu_grad_mul(torch.ones(n, dtype=dtype, device=DEV), dev(h, dtype), out)
        o = out.float().cpu()
        assert bool(torch.isnan(o[254])), f'gelu_grad_mul {dtype}: NaN in, NaN out'
        X.report(f'info gelu specials gelu_grad_mul {dtype}: gelu\'(+Inf)={o[255].item():g}; bf16 subnormal inputs: '
                 f'{int((o[:254] == 0.5).sum())} of 254 give 0.5 (min {o[:254].min().item():g}, max {o[:254].max().item():g})')


# ------------------------------------------------------------------------------------------------ bf16, every family
def run_act(tag, gen, K, act, scale=False, M=M0, keep=None):
    """act = 1: C == RNE(g32(pre)), C2 == RNE(pre); act = 2: C == RNE(g32(pre)), C2 == RNE(d32(pre)).  With scale: a row
    scale s[m / 4] from {0, 0.5, 1, 2} on C (an exact scaling in fp32; C2, the derivative, is stored unscaled)."""
    from vtx import ops
    N = K
    c = _case(gen, M, K)
    C = X.guarded((M, N), BF16, DEV)
    C2 = X.sentinel_fill(torch.empty(M + 3, N, dtype=BF16, device=DEV))
    kw, srow = {}, None
    if scale:
        s = X.dyadic_scales(M // 4, seed=K)
        kw = dict(row_scale=dev(s), rs=(4, 1, 1, 0))
        srow = s.repeat_interleave(4)[:, None]
    ops.gemm_nt(dev(c.A, BF16), dev(c.W, BF16), C, M, N, K, ldc=N + 8, act=act, C2=C2, **kw)
    name = f'{tag} {gen} {M}x{N}x{K} act={act}' + (' row_scale' if scale else '')
    guards = {'ldc pad': C[:, N:], 'C2 tail': C2[M:]}
    if srow is None:
        _both(f'{name} gelu', C[:, :N], c.g32, c.tg, c.bg, guards)
    else:
        _both(f'{name} gelu', C[:, :N], c.g32 * srow, c.tg * srow.double(), c.bg * srow.double(), guards)
    if act == 1:
        X.check_exact(f'{name} pre-activation copy', C2[:M], c.pre_bf16)
    else:
        _both(f"{name} gelu'", C2[:M], c.d32, c.td, c.bd)
    if keep is not None:
        keep['gelu_prime'] = C2[:M].clone()


def run_act_residual(tag, gen, K):
    """act = 1 with a residual, A / C / R rows through the token map: C == RNE(g32(pre) +_fp32 R), R integers in [-32, 32]
    (the fp32 add done on the CPU from the canonical values); C2 == RNE(pre).  The bound grows by the add's rounding,
    2^-24 |gelu + R|."""
    from vtx import ops
    M, N = M_TOK, K
    B = X.TOK_B
    c = _case(gen, M, K)
    tm = ops.tokmap(X.TOK_N)
    Xp = torch.full((B, 1 + X.TOK_N, K), 3.0)                        # cls rows the map must skip: non-zero
    Xp[:, 1:] = c.A.reshape(B, X.TOK_N, K)
    R = X.ints((B, 1 + X.TOK_N, N), -32, 32, 1.0, seed=K)
    out = X.guarded((B, 1 + X.TOK_N, N), BF16, DEV)
    C2 = X.sentinel_fill(torch.empty(M + 3, N, dtype=BF16, device=DEV))
    ops.gemm_nt(dev(Xp, BF16), dev(c.W, BF16), out, M, N, K, ldc=N + 8, amap=tm, cmap=tm, rmap=tm, act=1, C2=C2, R=dev(R, BF16))
    Rt = R[:, 1:].reshape(M, N)
    name = f'{tag} {gen} {M}x{N}x{K} act=1 residual (token map)'
    guards = {'cls rows': out[:, 0, :N], 'ldc pad': out[..., N:], 'C2 tail': C2[M:]}
    t = c.tg + Rt.double()
    _both(f'{name} gelu + R', out[:, 1:, :N].reshape(M, N), c.g32 + Rt, t, c.bg + G.U24 * (t.abs() + c.bg), guards)
    X.check_exact(f'{name} pre-activation copy', C2[:M], c.pre_bf16)


def run_dgelu(tag, K, acc, M=M0):
    """dgelu_kind = 0 (v *= gelu'(h)) with every accumulator exactly acc and h = all_bf16(): C == RNE(acc * d32(h)).  Adjacent
    columns of h hold different values, so a swapped even / odd element of a packed pair fails."""
    from vtx import ops
    N = K
    c = _case('all', M, K)
    A, W = G.unit_operands(M, K, acc)
    C = X.guarded((M, N), BF16, DEV)
    ops.gemm_nt(dev(A, BF16), dev(W, BF16), C, M, N, K, ldc=N + 8, dgelu_in=dev(c.A, BF16), dgelu_kind=0)
    _both(f"{tag} {M}x{N}x{K} dgelu_kind=0 acc={acc:g}", C[:, :N], acc * c.d32, acc * c.td, abs(acc) * c.bd, {'ldc pad': C[:, N:]})


def run_mul_stored(tag, K, acc, stored, M=M0):
    """dgelu_kind = 1 fed the bf16 gelu' an act = 2 run stored: exact, C == RNE(acc * stored)."""
    from vtx import ops
    N = K
    A, W = G.unit_operands(M, K, acc)
    C = X.guarded((M, N), BF16, DEV)
    ops.gemm_nt(dev(A, BF16), dev(W, BF16), C, M, N, K, ldc=N + 8, dgelu_in=stored, dgelu_kind=1)
    X.check_exact(f"{tag} {M}x{N}x{K} dgelu_kind=1 acc={acc:g} (stored gelu')", C[:, :N], (acc * stored.float().cpu()).to(BF16),
                  {'ldc pad': C[:, N:]})


# Branches reached (nt_family / launch_pp of csrc/gemm_nt.hip), beyond the family table of test_gpu_exact_arith.py:
#   pp256, act alone              gemm_nt_bf16_pp_kernel<EPI2, PRE_NONE, no scale, HAS_ACT, CONT = (K = 192)>: act = 2 takes the lean
#                                 passes (PP_LF) on whole 128 x 64 blocks and the general ones (PP_EPI2) on the ragged row tile, act = 1
#                                 the general ones everywhere
#   pp256, dgelu_kind = 0         gemm_nt_bf16_pp_kernel<EPI2, PRE_DGELU, ...>: the packed-pair read of PP_EPI2, never continuous
#   pp256, act with a residual or a row scale: combo_ok is false, nt_family falls back to launch_ring<4,3,32> at K = 192 and to
#                                 gemm_nt_bf16_dma_kernel at K = 128 (two K tiles); every other family runs its own kernel with the
#                                 generic epilogue<bf16raw>, which takes any combination
#   auto                          M = 600: dma2; M = 2364 (the residual case): pp256 and its fall-back
@pytest.mark.parametrize('K', G.GELU_KS)
@pytest.mark.parametrize('family', list(NT_FAMILIES))
def test_gemm_nt_gelu_family(family, K, vtx_opts):
    """Level 2 for every family, K = 192 and 128, both generators: act = 1 with C2, act = 2, act = 2 with a row scale, act = 1
    with a residual through the token map, and dgelu_kind = 0 with accumulators 1, -2 and 0.5."""
    _set(vtx_opts, NT_FAMILIES[family])
    tag = f'gemm_nt {family}'
    for gen in ('all', 'fine'):
        run_act(tag, gen, K, 1)
        run_act(tag, gen, K, 2)
        run_act(tag, gen, K, 2, scale=True)
        run_act_residual(tag, gen, K)
    for acc in (1.0, -2.0, 0.5):
        run_dgelu(tag, K, acc)


PP_OPTIONS = [dict(pp_cont=c, pp_epi=e, pp_grid=g) for c in ('0', '1') for e in ('0', '1', '4') for g in ('256', '8')]


@pytest.mark.parametrize('opts', PP_OPTIONS, ids=lambda o: '-'.join(f'{k}{v}' for k, v in o.items()))
def test_gemm_nt_pp256_gelu_structures(opts, vtx_opts):
    """The persistent kernel under both flows (pp_cont), its epilogue structures (pp_epi 0 / 4: the macro epilogues, 1: the
    generic epilogue) and grids (256: at most one tile per workgroup; 8: with M = 2360, ten tiles, several each), K = 192:
    act = 2, dgelu_kind = 0, and dgelu_kind = 1 fed the bf16 gelu' that the act = 2 run stored (exact: RNE(acc * stored))."""
    _set(vtx_opts, dict(gemm_nt='pp256', **opts))
    tag = 'gemm_nt pp256 ' + ' '.join(f'{k}={v}' for k, v in opts.items())
    for M in (M0, M_PP):
        keep = {}
        run_act(tag, 'all', KC, 2, M=M, keep=keep)
        run_dgelu(tag, KC, 1.0, M=M)
        run_dgelu(tag, KC, -2.0, M=M)
        for acc in (1.0, -2.0):
            run_mul_stored(tag, KC, acc, keep['gelu_prime'], M=M)


# ------------------------------------------------------------------------------------------------ gelu_grad_mul, bf16
def test_gelu_grad_mul_bf16():
    """out == RNE(dy * d32(h)) over all_bf16() with dy = 1, -2 and 0.5 (exact scalings)."""
    from vtx import ops
    h, d32, td, bd = _flat_case()
    n = h.numel()
    for dy in (1.0, -2.0, 0.5):
        out = X.sentinel_fill(torch.empty(n + 8, dtype=BF16, device=DEV))
        ops.gelu_grad_mul(torch.full((n,), dy, dtype=BF16, device=DEV), dev(h, BF16), out[:n])
        _both(f'gelu_grad_mul bf16 dy={dy:g}', out[:n], dy * d32, dy * td, abs(dy) * bd, {'tail': out[n:]})


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_gelu_grad_mul_rejects_bad_arguments(dtype):
    """n % 8 != 0 and a pointer that is not 16-byte aligned (a view offset by one element) raise, and nothing is launched: the
    sentinel-filled output is unchanged."""
    from vtx import ops
    from vtx._lib import VtxError
    n = 4096
    buf = torch.ones(n + 8, dtype=dtype, device=DEV)
    out = X.sentinel_fill(torch.empty(n + 8, dtype=dtype, device=DEV))
    with pytest.raises(VtxError):
        ops.gelu_grad_mul(buf[:n - 2], buf[:n - 2], out[:n - 2])
    for off in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        with pytest.raises(VtxError):
            ops.gelu_grad_mul(buf[off[0]:off[0] + n], buf[off[1]:off[1] + n], out[off[2]:off[2] + n])
    torch.cuda.synchronize()
    touched = X.sentinel_touched(out)
    X.report(f'{"FAIL" if touched else "ok  "} exact gelu_grad_mul {dtype} rejected calls launch nothing: {touched} of {out.numel()} '
             f'sentinel elements overwritten')
    assert touched == 0
