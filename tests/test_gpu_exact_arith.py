"""Exact-arithmetic parity of the GEMM, wprod, reduction, copy and cast kernels (helpers: tests/exact.py).

The inputs are small integers and dyadic scales, so every fp32 operation inside a kernel is exact and the correct output is
unique whatever the summation order: the exact value for fp32 outputs, RNE(exact value) for bf16 outputs.  Every case is
compared with equality, and the guard regions around the output (ldc padding columns, the cls rows a row map skips, the
tail of Csplit / C2) must be bit-unchanged.  Each dispatch branch is forced with the vtx_opts fixture; the comment on a
case names the branch of vtx_gemm_nt (csrc/gemm_nt.hip) / vtx_gemm_tn (csrc/gemm_tn.hip) it reaches.  The 'act_residual' case
checks its pre-activation copy exactly and the GELU output against float64 with a tolerance; the GELU value itself is pinned,
element by element, in test_gpu_exact_gelu.py.
"""
import functools

import pytest
import torch

import exact as X
from helpers import check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16 = torch.bfloat16


def dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


# ---------------------------------------------------------------------------------------------------- vtx_gemm_nt
# family -> options.  Branches (vtx_gemm_nt, bf16, K % 64 == 0 unless noted):
#   pp256         launch_pp: gemm_nt_bf16_pp_kernel<...> (>= 2 K tiles; act with residual / scale / multiplier -> ring<4,3,32>)
#   ring256x3     launch_ring<4,3,64>   (>= 3 K tiles; else gemm_nt_bf16_dma_kernel)
#   ring256x3k32  launch_ring<4,3,32>
#   ring256x4k32  launch_ring<4,4,32>
#   ring128x3     launch_ring<2,3,64>
#   ring128x4k32  launch_ring<2,4,32>
#   dma2          gemm_nt_bf16_dma_kernel
#   nodma         gemm_nodma=1: gemm_nt_bf16_kernel (register-staged; also every K % 64 != 0)
#   auto          M >= 2048 pp256, 1024 <= M < 2048 ring256x3k32, below dma2
NT_FAMILIES = {
    'pp256': dict(gemm_nt='pp256'),
    'ring256x3': dict(gemm_nt='ring256x3'),
    'ring256x3k32': dict(gemm_nt='ring256x3k32'),
    'ring256x4k32': dict(gemm_nt='ring256x4k32'),
    'ring128x3': dict(gemm_nt='ring128x3'),
    'ring128x4k32': dict(gemm_nt='ring128x4k32'),
    'dma2': dict(gemm_nt='dma2'),
    'nodma': dict(gemm_nodma='1'),
    'auto': dict(gemm_nt='auto'),
}


def _set(vtx_opts, opts):
    for k, v in opts.items():
        vtx_opts(k, v)


@functools.lru_cache(maxsize=None)
def _epi_case(epi, kind, seed):
    return X.nt_epilogue_case(epi, kind, seed=seed)


@functools.lru_cache(maxsize=None)
def _shape_case(M, N, K, kind):
    A, W, b = X.nt_operands(M, N, K, kind, seed=M)
    return A, W, b, X.nt_reference(f'{M}x{N}x{K}', A, W, bias=b)


def _expect(name, v, kind, dtype):
    if dtype == BF16:
        return X.expect_bf16(name, v, kind)
    X.assert_fp32_exact(name, v)
    return v.float()


def run_nt_shape(tag, M, N, K, kind, dtype=BF16):
    """bias epilogue, output with 8 guard columns (ldc = N + 8)."""
    from vtx import ops
    A, W, b, ref = _shape_case(M, N, K, kind)
    C = X.guarded((M, N), dtype, DEV)
    ops.gemm_nt(dev(A, dtype), dev(W, dtype), C, M, N, K, ldc=N + 8, bias=dev(b))
    X.check_exact(f'{tag} {M}x{N}x{K} {kind}', C[:, :N], _expect(tag, ref, kind, dtype), {'ldc pad': C[:, N:]})


def run_nt_epilogue(tag, epi, kind, dtype=BF16, seed=0):
    """One case of exact.nt_epilogue_case through vtx_gemm_nt, every output guarded."""
    from vtx import ops
    c = _epi_case(epi, kind, seed)
    M, N, K = c['M'], c['N'], c['K']
    tm = ops.tokmap(X.TOK_N)
    B, T = X.TOK_B, X.TOK_T
    kw = dict(bias=None if c['bias'] is None else dev(c['bias']), rs=c['rs'], r_period=c['r_period'], act=c['act'])
    if c['amap_tok']:
        kw['amap'] = tm
    if c['cmap_tok']:
        kw['cmap'] = tm
    if c['rmap_tok']:
        kw['rmap'] = tm
    if c['h'] is not None:
        kw.update(dgelu_in=dev(c['h'], dtype), dgelu_kind=1)
    if c['scale'] is not None:
        kw['row_scale'] = dev(c['scale'])
    if c['R'] is not None:
        kw['R'] = dev(c['R'], dtype)
    guards = {}
    if c['split_row']:
        Cs = X.sentinel_fill(torch.empty(B * T + 3, N, dtype=dtype, device=DEV))       # ldsplit = N: guard rows behind
        kw.update(split_row=c['split_row'], Csplit=Cs)
        guards['Csplit tail'] = Cs[B * T:]
    if c['act']:
        C2 = X.sentinel_fill(torch.empty(M + 3, N, dtype=dtype, device=DEV))
        kw['C2'] = C2
        guards['C2 tail'] = C2[M:]
    if c['out'] == 'tok':
        out = X.guarded((B, 1 + X.TOK_N, N), dtype, DEV)
        guards['cls rows'] = out[:, 0, :N]
        got = out[:, 1:, :N]
    else:
        out = X.guarded((M, N), dtype, DEV)
        got = out[:, :N]
    guards['ldc pad'] = out[..., N:]
    ops.gemm_nt(dev(c['A'], dtype), dev(c['W'], dtype), out, M, N, K, ldc=N + 8, **kw)
    name = f'{tag} {epi} {kind} {M}x{N}x{K}'
    if c['act']:
        # the GELU output is not exact: float64 tolerance on it (its guards still exact); the pre-activation copy exact
        pre = c['expected_pre']
        gelu = torch.nn.functional.gelu(pre).reshape(B, X.TOK_N, N) + c['R'][:, 1:].double()
        check(f'{name} gelu+residual', got.float(), gelu, 1e-2 if dtype == BF16 else 1e-5)
        X.check_exact(f'{name} pre-activation copy', C2[:M], _expect(name, pre, kind, dtype), guards)
        return
    X.check_exact(name, got, _expect(name, c['expected'], kind, dtype), guards)
    if c['split_row']:
        X.check_exact(f'{name} Csplit', Cs[:B * T], _expect(name, c['expected_split'], kind, dtype))


@pytest.mark.parametrize('family', list(NT_FAMILIES))
def test_gemm_nt_bf16_family_exact(family, vtx_opts):
    """Every bf16 family on the base shapes (ragged row / column tiles; 3, 4 and 2 K tiles) and every exact epilogue, as
    exact-range and as rounding cases (plain has no bias offset to round with: exact-range only).  nodma and auto also
    take K = 96 and K = 8 (K % 64 != 0: the register-staged kernel)."""
    _set(vtx_opts, NT_FAMILIES[family])
    shapes = X.NT_SHAPES + (X.NT_NODMA_SHAPES if family in ('nodma', 'auto') else ())
    for M, N, K, kind in shapes:
        run_nt_shape(f'gemm_nt {family}', M, N, K, kind)
    for epi in X.NT_EPILOGUES:
        for kind in (('exact',) if epi == 'plain' else ('exact', 'round')):
            run_nt_epilogue(f'gemm_nt {family}', epi, kind)


PP_OPTIONS = [dict(pp_grid=g, pp_cont=c, pp_epi=e, pp_cg=cg)
              for g in ('256', '8') for c in ('0', '1') for e in ('0', '1', '4') for cg in ('0', '1')]


@pytest.mark.parametrize('opts', PP_OPTIONS, ids=lambda o: '-'.join(f'{k}{v}' for k, v in o.items()))
def test_gemm_nt_pp256_options_exact(opts, vtx_opts):
    """The persistent kernel under every grid (256: one tile per workgroup and more; 8: many tiles each), flow (pp_cont 0:
    per-tile prologue, 1: continuous), epilogue structure (pp_epi 0 / 1 / 4) and column-group size (pp_cg 0: from K,
    1: forced): the same exact results -- a tile drawn twice or skipped, or a wrong slot in the continuous flow, fails."""
    _set(vtx_opts, dict(gemm_nt='pp256', **opts))
    tag = 'gemm_nt pp256 ' + ' '.join(f'{k}={v}' for k, v in opts.items())
    run_nt_shape(tag, *X.NT_SHAPES[0])
    run_nt_shape(tag, *X.NT_SHAPES[1])
    for i, epi in enumerate(('bias', 'scale', 'residual', 'mul', 'scale_split')):
        run_nt_epilogue(tag, epi, 'round' if i % 2 == 0 else 'exact')


def test_gemm_nt_f32_exact():
    """The fp32 kernel (gemm_nt_f32_kernel, mfma_f32_32x32x2f32): exact fp32 equality on the base shapes and every exact
    epilogue, both generators."""
    for M, N, K, kind in X.NT_SHAPES + X.NT_NODMA_SHAPES:
        run_nt_shape('gemm_nt f32', M, N, K, kind, dtype=torch.float32)
    for epi in X.NT_EPILOGUES:
        for kind in (('exact',) if epi == 'plain' else ('exact', 'round')):
            run_nt_epilogue('gemm_nt f32', epi, kind, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------- vtx_gemm_tn
# variant -> options.  Branches (vtx_gemm_tn, bf16):
#   pp256  gemm_tn_bf16_pp_kernel  when tp_eligible (M >= 4096, N1 and N2 multiples of 256) and the row-map groups are > 64
#          rows; otherwise the ring (M >= 1024) or gemm_tn_bf16_dma_kernel
#   w4     gemm_tn_bf16_w4_kernel  under the same conditions, the same fall-backs
#   ring   gemm_tn_bf16_ring_kernel (M >= 1024; below: dma2)
#   dma2   gemm_tn_bf16_dma_kernel
#   nodma  gemm_nodma=1: gemm_tn_bf16_kernel<false> (register-staged)
#   safe   tn_safe=1: gemm_tn_bf16_kernel<true> (bounds-checked loader)
TN_VARIANTS = {
    'pp256': dict(gemm_tn='pp256'),
    'w4': dict(gemm_tn='w4'),
    'ring': dict(gemm_tn='ring'),
    'dma2': dict(gemm_tn='dma2'),
    'nodma': dict(gemm_nodma='1'),
    'safe': dict(tn_safe='1'),
}
# (M, N1, N2): pp / w4 eligible; N1 / N2 tails of 216, 8 and 136 (ring / dma2 whatever the variant asks for)
TN_SHAPES = ((6000, 768, 512), (8192, 256, 256), (5000, 216, 768), (1500, 8, 136), (700, 136, 216))


@functools.lru_cache(maxsize=None)
def _tn_case(M, N1, N2, seed=0):
    A, B = X.tn_operands(M, N1, N2, seed)
    return A, B, X.tn_reference(f'tn {M}x{N1}x{N2}', A, B).float(), A.double().sum(0).float()


def run_tn(tag, M, N1, N2, dtype=BF16):
    from vtx import ops
    A, B, ref, cs = _tn_case(M, N1, N2)
    Ad, Bd = dev(A, dtype), dev(B, dtype)
    C, s = ops.gemm_tn(Ad, Bd, M, N1, N2, want_colsum=True)
    X.check_exact(f'{tag} {M}x{N1}x{N2}', C, ref)
    X.check_exact(f'{tag} {M}x{N1}x{N2} fused colsum', s, cs)
    # accumulate into an integer-valued C, colsum accumulated into its own buffer
    C0, s0 = X.ints((N1, N2), -50, 50, 1.0, 7), X.ints((N1,), -50, 50, 1.0, 8)
    Cacc, sacc = dev(C0), dev(s0)
    ops.gemm_tn(Ad, Bd, M, N1, N2, out=Cacc, accumulate=True, colsum_out=sacc, colsum_accumulate=True)
    X.check_exact(f'{tag} {M}x{N1}x{N2} accumulate', Cacc, ref + C0)
    X.check_exact(f'{tag} {M}x{N1}x{N2} colsum_accumulate', sacc, cs + s0)
    C2 = ops.gemm_tn(Ad, Bd, M, N1, N2)
    X.check_exact(f'{tag} {M}x{N1}x{N2} no colsum', C2, ref)


@pytest.mark.parametrize('variant', list(TN_VARIANTS))
def test_gemm_tn_exact(variant, vtx_opts):
    """Every TN variant on every shape: plain, fused colsum, accumulate, colsum_accumulate -- exact fp32 equality."""
    _set(vtx_opts, TN_VARIANTS[variant])
    for M, N1, N2 in TN_SHAPES:
        run_tn(f'gemm_tn {variant}', M, N1, N2)


@pytest.mark.parametrize('variant', ['pp256', 'w4'])
def test_gemm_tn_slab_partitions_exact(variant, vtx_opts):
    """tn_cus changes the slab partition of the pp256 / w4 kernels (slabs = tn_cus / column tiles, at most M / 128; 32 is
    the smallest value vtx_set_option accepts): at 6000 x 768 x 512 the slabs hold 2 K tiles (256, 240, 192), 9 (64) and
    18 (32), the last slab also the remainder; at 8192 x 256 x 256 2 (256 .. 64) and 4 (32).  Every partition gives the
    identical exact result."""
    _set(vtx_opts, TN_VARIANTS[variant])
    for cus in ('256', '240', '192', '64', '32'):
        vtx_opts('tn_cus', cus)
        for M, N1, N2 in TN_SHAPES[:2]:
            run_tn(f'gemm_tn {variant} tn_cus={cus}', M, N1, N2)


@pytest.mark.parametrize('variant', list(TN_VARIANTS))
def test_gemm_tn_rowmaps_exact(variant, vtx_opts):
    """Token maps on both operands (groups of 788 rows: boundaries inside a 64-row K tile), M = 6 x 788 = 4728 (pp / w4
    eligible), with the fused colsum."""
    from vtx import ops
    _set(vtx_opts, TN_VARIANTS[variant])
    Bn, N1, N2 = 6, 256, 512
    M = Bn * X.TOK_N
    Xp = X.ints((Bn, 1 + X.TOK_N, N1), -3, 3, 1.0, 11)
    Yp = X.ints((Bn, 1 + X.TOK_N, N2), -3, 3, 1.0, 12)              # cls rows non-zero: a map that reads them fails
    tm = ops.tokmap(X.TOK_N)
    C, s = ops.gemm_tn(dev(Xp, BF16), dev(Yp, BF16), M, N1, N2, amap=tm, bmap=tm, want_colsum=True)
    A, B = Xp[:, 1:].reshape(M, N1), Yp[:, 1:].reshape(M, N2)
    X.check_exact(f'gemm_tn {variant} rowmaps {M}x{N1}x{N2}', C, X.tn_reference('tn rowmaps', A, B).float())
    X.check_exact(f'gemm_tn {variant} rowmaps colsum', s, A.double().sum(0).float())


def test_gemm_tn_f32_exact():
    """The fp32 TN kernel (gemm_tn_f32_kernel)."""
    for M, N1, N2 in TN_SHAPES[2:]:
        run_tn('gemm_tn f32', M, N1, N2, dtype=torch.float32)


# -------------------------------------------------------------------------------------------------------- vtx_wprod
@pytest.mark.parametrize('ta', [False, True])
@pytest.mark.parametrize('tb', [False, True])
def test_wprod_exact(ta, tb):
    """out (+)= alpha op(A) op(B) + u v^T, y (+)= alpha_y op(A) x + beta_z z (include/vtx.h), ragged 68 x 132 x 36,
    dyadic alpha in {1, -2, 0.5}: exact fp32 equality."""
    from vtx import ops
    N1, N2, K = 68, 132, 36
    A = X.ints((K, N1) if ta else (N1, K), -4, 4, 1.0, 1)
    Bm = X.ints((N2, K) if tb else (K, N2), -4, 4, 1.0, 2)
    Ad = A.t().double() if ta else A.double()
    Bd = Bm.t().double() if tb else Bm.double()
    P = Ad @ Bd
    u, v = X.ints((N1,), -8, 8, 1.0, 3), X.ints((N2,), -8, 8, 1.0, 4)
    x, z = X.ints((K,), -8, 8, 1.0, 5), X.ints((N1,), -8, 8, 1.0, 6)
    C0, y0 = X.ints((N1, N2), -64, 64, 1.0, 7), X.ints((N1,), -64, 64, 1.0, 8)
    tag = f'wprod[{int(ta)},{int(tb)}] {N1}x{N2}x{K}'
    for alpha in (1.0, -2.0, 0.5):
        got = ops.wprod(dev(A), dev(Bm), ta=ta, tb=tb, alpha=alpha)
        X.check_exact(f'{tag} alpha={alpha:g}', got, (alpha * P).float())
    C = dev(C0)
    _, y = ops.wprod(dev(A), dev(Bm), ta=ta, tb=tb, alpha=-2.0, out=C, accumulate=True, u=dev(u), v=dev(v), x=dev(x),
                     y=dev(y0), alpha_y=0.5, z=dev(z), beta_z=-2.0, y_accumulate=True)
    X.check_exact(f'{tag} accumulate + u v^T', C, (C0.double() - 2 * P + torch.outer(u, v).double()).float())
    X.check_exact(f'{tag} y accumulate', y, (y0.double() + 0.5 * Ad @ x.double() - 2 * z.double()).float())
    _, y2 = ops.wprod(dev(A), dev(Bm), ta=ta, tb=tb, x=dev(x), alpha_y=2.0, z=dev(z), beta_z=0.5)
    X.check_exact(f'{tag} y', y2, (2 * Ad @ x.double() + 0.5 * z.double()).float())


# --------------------------------------------------------------------------------------------- reductions and copies
def _out(t, dtype):
    """Expected output of a float64 value that is exact in fp32: RNE to bf16, or the fp32 value itself."""
    X.assert_fp32_exact('expected', t)
    return X.rne_bf16(t) if dtype == BF16 else t.float()


@pytest.mark.parametrize('dtype', [torch.float32, BF16])
def test_reductions_exact(dtype):
    """One exact case per reduction (formulas from include/vtx.h):
    colsum           out[n] (+)= sum_m A[amap(m)][n]
    reduce_rows      out[j,:] (+)= scale * sum_{i<ni} in[base + i*si + j*sj, :]        (scale 1 and 0.5)
    dropped_rows_fix out[omap(m)] = x[xmap(m)] + bias, zero[m] = 0 on the rows of groups with s == 0
    dropped_rows_colsum  sum of the [nparts, D] partials = column sums of src[smap(m)] over the dropped groups' rows
    cls_qkv_reduce   dqkv[b,0,:] = sum_t dqkv_cls[b*T+t,:]
    cls_mean_fwd     out[b,0,:] = x[b,0,:] + mean_t a_cls[b*T+t,:]                      (T = 4: 1/T exact)
    space_grad_prep  da[b*N+n] = dout[b,1+n] s[b*T + n%T],  da[B*N + b*T+t] = dout[b,0] s[b*T+t] / T"""
    from vtx import ops
    B, P, T, D = 3, 7, 4, 200
    N = P * T
    M = B * N
    tm = ops.tokmap(N)
    x = X.ints((B, 1 + N, D), -8, 8, 1.0, 1)
    xq = x.double()
    tok = xq[:, 1:].reshape(M, D)
    # colsum, plain and accumulated, through the token map
    c = ops.colsum(dev(x, dtype), M, D, amap=tm)
    X.check_exact(f'colsum {dtype}', c, tok.sum(0).float())
    c0 = X.ints((D,), -20, 20, 1.0, 2)
    cacc = dev(c0)
    ops.colsum(dev(x, dtype), M, D, amap=tm, out=cacc, accumulate=True)
    X.check_exact(f'colsum accumulate {dtype}', cacc, (tok.sum(0) + c0.double()).float())
    # reduce_rows: the sum over clips, then by position / frame; scale 0.5 with accumulate
    r = ops.reduce_rows(dev(x, dtype), N, B, D, D, 1, 1 + N, 1)
    X.check_exact(f'reduce_rows batch {dtype}', r, xq[:, 1:].sum(0).float())
    r2 = ops.reduce_rows(r, P, T, D, D, 0, 1, T)
    X.check_exact(f'reduce_rows pos {dtype}', r2, xq[:, 1:].sum(0).reshape(P, T, D).sum(1).float())
    o0 = X.ints((T, D), -20, 20, 1.0, 3)
    r3 = dev(o0)
    ops.reduce_rows(r, T, P, D, D, 0, T, 1, out=r3, scale=0.5, accumulate=True)
    X.check_exact(f'reduce_rows time scale 0.5 accumulate {dtype}', r3,
                  (o0.double() + 0.5 * xq[:, 1:].sum(0).reshape(P, T, D).sum(0)).float())
    # dropped-row fix-ups
    s = X.dyadic_scales(M // T, 4)
    assert 0 < int((s == 0).sum()) < s.numel()
    bias = X.ints((D,), -8, 8, 1.0, 5)
    out0, z0 = X.ints((B, 1 + N, D), -8, 8, 1.0, 6), X.ints((M, D), -8, 8, 1.0, 7)
    out, zo = dev(out0, dtype), dev(z0, dtype)
    ops.dropped_rows_fix(dev(s), M, D, T, x=dev(x, dtype), xmap=tm, bias=dev(bias), out=out, omap=tm, zero=zo)
    drop = (s == 0).repeat_interleave(T).reshape(B, N)
    ref = out0.double().clone()
    ref[:, 1:][drop] = (xq[:, 1:] + bias.double())[drop]
    refz = z0.double().clone()
    refz[drop.reshape(M)] = 0
    X.check_exact(f'dropped_rows_fix out {dtype}', out, _out(ref, dtype))
    X.check_exact(f'dropped_rows_fix zero {dtype}', zo, _out(refz, dtype))
    for nparts in (1, 5, 32):
        part = ops.dropped_rows_colsum(dev(x, dtype), dev(s), M, D, T, smap=tm, nparts=nparts)
        fold = ops.reduce_rows(part, 1, nparts, D, D, 0, 1, 0)
        X.check_exact(f'dropped_rows_colsum nparts={nparts} {dtype}', fold[0], xq[:, 1:][drop].sum(0).float())
    # cls rows: per-frame sums, means
    W3 = 96
    dcls = X.ints((B * T, W3), -16, 16, 1.0, 8)
    dqkv = X.guarded((B, 1 + N, W3), dtype, DEV, pad_cols=0)
    ops.cls_qkv_reduce(dev(dcls, dtype), dqkv, B, T, W3, 1 + N)
    X.check_exact(f'cls_qkv_reduce {dtype}', dqkv[:, 0], _out(dcls.double().reshape(B, T, W3).sum(1), dtype),
                  {'token rows': dqkv[:, 1:]})
    a_cls = X.ints((B * T, D), -16, 16, 1.0, 9)
    o = X.guarded((B, 1 + N, D), dtype, DEV, pad_cols=0)
    ops.cls_mean_fwd(dev(a_cls, dtype), dev(x, dtype), o, B, T, D, 1 + N)
    X.check_exact(f'cls_mean_fwd {dtype}', o[:, 0], _out(xq[:, 0] + a_cls.double().reshape(B, T, D).mean(1), dtype),
                  {'token rows': o[:, 1:]})
    sg = X.dyadic_scales(B * T, 10)
    da = torch.empty(M + B * T, D, dtype=dtype, device=DEV)
    ops.space_grad_prep(dev(x, dtype), dev(sg), da, B, T, P, D)
    n = torch.arange(N)
    ref_tok = xq[:, 1:] * sg.double().reshape(B, T)[:, n % T][:, :, None]
    ref_cls = (xq[:, :1] * sg.double().reshape(B, T, 1) / T).reshape(B * T, D)
    X.check_exact(f'space_grad_prep tokens {dtype}', da[:M], _out(ref_tok.reshape(M, D), dtype))
    X.check_exact(f'space_grad_prep cls {dtype}', da[M:], _out(ref_cls, dtype))


@pytest.mark.parametrize('dtype', [torch.float32, BF16])
def test_copies_exact(dtype):
    """row_scale_copy  dst[dmap(m)] = src[smap(m)] * s[(m/rs_d1)*rs_m1 + (m%rs_d2)*rs_m2]
    fact_glue_fwd    h[i,0] = x[i,0] + e[0],  h[i,1+t] = mean_p x[i*T+t, 1+p] + e[1+t]    (P = 16: 1/P exact)
    fact_glue_bwd    its adjoint: dx, d_time_embed (+)= sum_i dh[i]
    embed_table      E[p*T+t] = bias + pos[1+p] + time[t] (frame_major: row t*P+p),  cls_row = cls + pos[0]
    MaxPoolSkipFn backward: scatter-add of dy into the argmax positions (integer sums)"""
    from vtx import ops
    from vtx import functions as F_
    B, P, T, D = 3, 16, 4, 128
    N = P * T
    M = B * N
    tm = ops.tokmap(N)
    src = X.ints((M, D), -16, 16, 1.0, 1)
    s = X.dyadic_scales(B * T, 2)
    dst = X.guarded((B, 1 + N, D), dtype, DEV, pad_cols=8)
    ops.row_scale_copy(dev(src, dtype), dst, M, D, ldd=D + 8, dmap=tm, s=dev(s), rs=(N, T, T, 1))
    m = torch.arange(M)
    ref = src.double() * s.double()[(m // N) * T + m % T][:, None]
    X.check_exact(f'row_scale_copy spatial index {dtype}', dst[:, 1:, :D], _out(ref.reshape(B, N, D), dtype),
                  {'cls rows': dst[:, 0, :D], 'ld pad': dst[..., D:]})
    # fact_glue forward / backward against the float64 autograd of the reference expression
    xg = X.ints((B * T, 1 + P, D), -16, 16, 1.0, 3)
    e = X.ints((1, 1 + T, D), -16, 16, 1.0, 4)
    dh = X.ints((B, 1 + T, D), -16, 16, 1.0, 5)
    xr = xg.double().requires_grad_(True)
    er = e.double().requires_grad_(True)
    ref = torch.cat((xr[:B, 0, :].unsqueeze(1), xr[:, 1:, :].reshape(B, T, P, D).mean(2)), dim=1) + er
    ref.backward(dh.double())
    h = ops.fact_glue_fwd(dev(xg, dtype), dev(e.reshape(1 + T, D)), B, T, P, D)
    X.check_exact(f'fact_glue_fwd {dtype}', h, _out(ref.detach(), dtype))
    de = torch.full((1 + T, D), float('nan'), device=DEV)
    dx = ops.fact_glue_bwd(dev(dh, dtype), B, T, P, D, d_time_embed=de)
    X.check_exact(f'fact_glue_bwd dx {dtype}', dx, _out(xr.grad, dtype))
    X.check_exact(f'fact_glue_bwd d_time_embed {dtype}', de, er.grad.reshape(1 + T, D).float())
    de2 = dev(X.ints((1 + T, D), -16, 16, 1.0, 6))
    de2_0 = de2.cpu().double()
    ops.fact_glue_bwd(dev(dh, dtype), B, T, P, D, d_time_embed=de2, accumulate=True)
    X.check_exact(f'fact_glue_bwd d_time_embed accumulate {dtype}', de2, (de2_0 + er.grad.reshape(1 + T, D)).float())
    # embedding table, token-major and frame-major, with and without the time embedding
    Pe, Te, De = 14, 3, 96
    bias, pos = X.ints((De,), -32, 32, 1.0, 7), X.ints((1 + Pe, De), -32, 32, 1.0, 8)
    te, cls = X.ints((Te, De), -32, 32, 1.0, 9), X.ints((De,), -32, 32, 1.0, 10)
    for fm in (False, True):
        for with_time in (True, False):
            E, cr = ops.embed_table(dtype, Pe, Te, De, dev(bias), dev(pos), dev(te) if with_time else None, dev(cls), frame_major=fm)
            ref = bias.double() + pos.double()[1:, None, :] + (te.double()[None] if with_time else 0.0)      # [P, T, D]
            ref = ref.expand(Pe, Te, De)
            ref = (ref.transpose(0, 1) if fm else ref).reshape(Pe * Te, De)
            X.check_exact(f'embed_table frame_major={fm} time={with_time} {dtype}', E, _out(ref, dtype))
            X.check_exact(f'embed_table cls row {dtype}', cr, _out(cls.double() + pos.double()[0], dtype))
    # MaxPoolSkipFn backward: distinct values per window (a permutation per (b, t, c) frame) so the argmax is unique
    Bm, Tm, Hm, Wm, Cm = 2, 3, 7, 9, 40
    g = X.gen(11)
    perm = torch.stack([torch.randperm(Hm * Wm, generator=g) for _ in range(Bm * Tm * Cm)]).float() - 32
    xm = torch.zeros(Bm, 1 + Tm * Hm * Wm, Cm)
    xm[:, 1:] = perm.reshape(Bm, Tm, Cm, Hm * Wm).permute(0, 1, 3, 2).reshape(Bm, Tm * Hm * Wm, Cm)
    xm[:, 0] = X.ints((Bm, Cm), -8, 8, 1.0, 12)
    from oracle import mvit_oracle as MO
    xr = xm.double().requires_grad_(True)
    pool = torch.nn.MaxPool3d([1, 3, 3], [1, 2, 2], [0, 1, 1])
    yr, _ = MO.attention_pool(xr, pool, [Tm, Hm, Wm])
    dy = X.ints(tuple(yr.shape), -16, 16, 1.0, 13)
    yr.backward(dy.double())
    xd = dev(xm, dtype).requires_grad_(True)
    y = F_.MaxPoolSkipFn.apply(xd, [Tm, Hm, Wm])
    y.backward(dev(dy, dtype))
    X.check_exact(f'maxpool_skip fwd {dtype}', y, _out(yr.detach(), dtype))
    X.check_exact(f'maxpool_skip bwd (scatter-add) {dtype}', xd.grad, _out(xr.grad, dtype))


# ------------------------------------------------------------------------------------------------------------ casts
def _f32_specials():
    """fp32 bit patterns: RNE ties (low half 0x8000) below / above even and odd upper halves around several exponents,
    the neighbours of ties, +-0, +-Inf, quiet and signalling NaNs of both signs, the largest finite values (those with an
    upper half of 0x7F7F round to Inf when the low half is >= 0x8000), and fp32 subnormals."""
    his = []
    for e in (1, 2, 0x3F, 0x40, 0x7E, 0x7F, 0x80, 0x8F, 0xFE):           # biased exponents 2, 4, ..., 126, 254, ...
        for mant in (0x00, 0x01, 0x7E, 0x7F):
            his.append((e << 7) | mant)
    his += [0x0000, 0x0001, 0x0040, 0x007F, 0x7F7F, 0x7F7E]                # subnormal upper halves, largest finite
    lows = [0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF]
    bits = [(s << 31) | (h << 16) | lo for s in (0, 1) for h in his for lo in lows]
    bits += [0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FBFFFFF, 0x7FFFFFFF,
             0x00000001, 0x80000001, 0x00000002, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000]
    rnd = torch.randint(-2 ** 31, 2 ** 31 - 1, (1 << 16,), generator=X.gen(3), dtype=torch.int64)
    t = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int64)
    return torch.cat([t, rnd]).to(torch.int32).view(torch.float32)


def _check_cast(name, got, want):
    """Bit equality with torch's conversion, except that a NaN only has to stay a NaN (torch's own float -> bf16 drops the
    sign and payload of a NaN, so neither is asserted)."""
    got = got.detach().cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f'{name}: NaN positions differ'
    ib = X._INT[got.dtype]
    X.check_exact(f'{name} (bit patterns)', got.view(ib)[~nan], want.view(ib)[~nan])


def test_casts_bitexact():
    """cast_from_f32 / cast_to_f32 / cast_transpose / mt_cast_transpose against torch's conversions, bit for bit: RNE ties,
    +-0 (the sign of zero is compared through the bits), +-Inf, NaNs, the overflow to Inf, subnormals; cast_to_f32 on
    all 65536 bf16 patterns.  gfx950 converts with v_cvt_pk_bf16_f32, which keeps fp32 subnormals (as torch does)."""
    from vtx import ops
    f = _f32_specials()
    want = f.to(BF16)
    got = ops.cast_from_f32(dev(f), BF16)
    _check_cast('cast_from_f32 specials', got, want)
    allb = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int64).to(torch.int16).view(BF16)
    _check_cast('cast_to_f32 all bf16 patterns', ops.cast_to_f32(dev(allb)), allb.float())
    # weight staging of the same patterns: [R, C] and its transpose, ragged 64 x 64 tiles
    Rr = 97
    Cc = f.numel() // Rr
    W = f[:Rr * Cc].reshape(Rr, Cc)
    wc, wt = ops.cast_transpose(dev(W), BF16)
    _check_cast('cast_transpose Wc', wc, W.to(BF16))
    _check_cast('cast_transpose WcT', wt, W.t().contiguous().to(BF16))
    # multi-tensor staging: a table of three ragged matrices, some targets absent
    mats = [f[:130 * 72].reshape(130, 72), f[1000:1000 + 8 * 200].reshape(8, 200), f[5000:5000 + 64 * 64].reshape(64, 64)]
    Ws = [dev(m_) for m_ in mats]
    outs = [(torch.empty(m_.shape, dtype=BF16, device=DEV), torch.empty(m_.shape[::-1], dtype=BF16, device=DEV))
            for m_ in mats]
    entries = [(Ws[0], outs[0][0], outs[0][1]), (Ws[1], None, outs[1][1]), (Ws[2], outs[2][0], None)]
    tab, starts, ntiles = ops.ct_table(entries, DEV)
    ops.mt_cast_transpose(BF16, tab, starts, len(entries), ntiles)
    _check_cast('mt_cast_transpose 0 c', outs[0][0], mats[0].to(BF16))
    _check_cast('mt_cast_transpose 0 t', outs[0][1], mats[0].t().contiguous().to(BF16))
    _check_cast('mt_cast_transpose 1 t', outs[1][1], mats[1].t().contiguous().to(BF16))
    _check_cast('mt_cast_transpose 2 c', outs[2][0], mats[2].to(BF16))


# --------------------------------------------------------------------------------------------------- large operands
GB2 = 1 << 31


def _row_blocks(M, row_bytes, tile=256):
    """Row ranges that get non-zero values: the first tile, the tiles around the row holding byte 2^31, the last
    (ragged) tile."""
    r = GB2 // row_bytes
    t0 = r // tile * tile
    return [(0, tile), (t0 - tile, t0 + 2 * tile), (M // tile * tile, M)]


@pytest.mark.parametrize('family', ['pp256', 'ring256x3k32', 'dma2'])
def test_gemm_nt_operand_beyond_2gb_exact(family, vtx_opts):
    """A [1 500 037, 768] bf16 (2.3 GB) and C [1 500 037, 768] (2.3 GB): zeros except the first, the 2^31-byte-straddling and
    the last tiles of A.  Those output rows are exact; every other output element is exactly 0 (one count_nonzero on the
    device).  Catches 32-bit overflow of a tile's base or of a lane offset in the loads and the stores."""
    from vtx import ops
    vtx_opts('gemm_nt', family)
    M, N, K = 1500037, 768, 768
    A = torch.zeros(M, K, dtype=BF16, device=DEV)
    blocks = _row_blocks(M, K * 2)
    W = X.ints((N, K), -2, 2, X.density_for(K), 2)
    parts = []
    for i, (r0, r1) in enumerate(blocks):
        Ab = X.ints((r1 - r0, K), -1, 1, X.density_for(K), 10 + i)
        A[r0:r1] = dev(Ab, BF16)
        parts.append(X.expect_bf16(f'large {family} block {i}', X.nt_reference('large', Ab, W), 'exact'))
    C = torch.empty(M, N, dtype=BF16, device=DEV)
    ops.gemm_nt(A, dev(W, BF16), C, M, N, K)
    del A
    nz = int(torch.count_nonzero(C).item())
    for i, (r0, r1) in enumerate(blocks):
        X.check_exact(f'gemm_nt {family} > 2 GB operand, rows {r0}..{r1}', C[r0:r1], parts[i])
    want_nz = sum(int(torch.count_nonzero(p_).item()) for p_ in parts)
    del C
    torch.cuda.empty_cache()
    assert nz == want_nz, f'{family}: {nz - want_nz} non-zero outputs outside the written row blocks'


@pytest.mark.parametrize('variant', ['pp256', 'w4'])
def test_gemm_tn_operand_beyond_2gb_exact(variant, vtx_opts):
    """A [1 500 037, 768] bf16 (2.3 GB), B [1 500 037, 256]: zeros except the first, the 2^31-byte-straddling and the last
    row blocks; C = the sum over those rows alone, exact (with the fused colsum)."""
    from vtx import ops
    vtx_opts('gemm_tn', variant)
    M, N1, N2 = 1500037, 768, 256
    A = torch.zeros(M, N1, dtype=BF16, device=DEV)
    B = torch.zeros(M, N2, dtype=BF16, device=DEV)
    As, Bs = [], []
    for i, (r0, r1) in enumerate(_row_blocks(M, N1 * 2, tile=64)):
        Ab, Bb = X.tn_operands(r1 - r0, N1, N2, seed=20 + 2 * i)
        A[r0:r1] = dev(Ab, BF16)
        B[r0:r1] = dev(Bb, BF16)
        As.append(Ab)
        Bs.append(Bb)
    Acat, Bcat = torch.cat(As), torch.cat(Bs)
    C, cs = ops.gemm_tn(A, B, M, N1, N2, want_colsum=True)
    del A, B
    torch.cuda.empty_cache()
    X.check_exact(f'gemm_tn {variant} > 2 GB operand', C, X.tn_reference('tn large', Acat, Bcat).float())
    X.check_exact(f'gemm_tn {variant} > 2 GB operand colsum', cs, Acat.double().sum(0).float())
