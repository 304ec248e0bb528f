"""Exact-arithmetic test helpers (imported by test modules; not a conftest).

Inputs are small integers and dyadic scales chosen so that every fp32 operation a kernel performs is exact: every partial
sum of an accumulator is an integer (or a dyadic value) below 2^24 in magnitude, whatever the summation order.  The
correct output is then unique -- the exact value for fp32 outputs, RNE(exact value) for bf16 outputs -- and the kernel is
held to it with equality, on every dispatch path and independently of any tolerance policy.

Two kinds of bf16 case:
  'exact'  every expected output is representable in bf16 (|x| <= 256 integers, dyadic values with <= 8 significant
           bits), so the store leaves it unchanged: an error of one unit of the output shows;
  'round'  a bias offset of ~512 puts the outputs where the bf16 spacing is 2..8, so a good share of them are exact ties
           and most are inexact: round-to-nearest-even and ties-to-even are exercised on every store.
"""
import torch

from helpers import report

EXACT_LIMIT = 2 ** 24                        # every fp32 intermediate stays strictly below this in magnitude
SENT_BF16 = 0x7FA5                           # NaN bit patterns the guard regions are filled with
SENT_F32 = 0x7FC0A5A5
_INT = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, lo, hi, density=1.0, seed=0):
    """float32 CPU tensor of integers uniform in [lo, hi], each element zero with probability 1 - density."""
    g = gen(seed)
    v = torch.randint(lo, hi + 1, shape, generator=g).float()
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density).float()
    return v


def density_for(K, target=12.0):
    """Operand density such that a K-term dot product has ~target non-zero terms on average (small sums, any K)."""
    return min(1.0, (target / K) ** 0.5)


def dyadic_scales(n, seed=0, choices=(0.0, 0.5, 1.0, 2.0), weights=None):
    """Row scales drawn from `choices` (DropPath keep-scales with exact products; 0 = a dropped group)."""
    c = torch.tensor(choices, dtype=torch.float32)
    w = torch.ones(len(choices)) if weights is None else torch.tensor(weights, dtype=torch.float32)
    return c[torch.multinomial(w, n, replacement=True, generator=gen(seed))]


def rne_bf16(x):
    """float64 -> float32 -> bfloat16 (both steps round to nearest even; the first is exact under the premise)."""
    return x.to(torch.float32).to(torch.bfloat16)


def assert_fp32_exact(name, x):
    """x (float64) is exactly representable in fp32 and below 2^24 in magnitude."""
    x = x.double()
    assert bool((x.abs() < EXACT_LIMIT).all()), f'{name}: |x| reaches 2^24 (max {x.abs().max().item():g})'
    assert torch.equal(x.float().double(), x), f'{name}: not representable in fp32'


def assert_acc_bound(name, A, B):
    """Every partial sum of A @ B^T (float64 operands [M,K], [N,K]) is below 2^24: (|A| @ |B|^T).max() < 2^24."""
    b = (A.double().abs() @ B.double().abs().t()).max().item() if A.numel() and B.numel() else 0.0
    assert b < EXACT_LIMIT, f'{name}: accumulator bound {b:g} >= 2^24'
    return b


def bf16_stats(x):
    """(ties, inexact) fractions of the float64 values x (fp32-exact) under bf16 rounding: bf16 keeps the upper 16 bits
    of the fp32 pattern, so the lower 16 bits are 0 (exact), 0x8000 (a tie) or anything else (inexact, no tie)."""
    low = x.double().float().view(torch.int32) & 0xFFFF
    n = max(x.numel(), 1)
    return (low == 0x8000).sum().item() / n, (low != 0).sum().item() / n


def expect_bf16(name, v, kind):
    """float64 expected values -> bf16 expected output, asserting the premise of the case kind."""
    assert_fp32_exact(name, v)
    e = rne_bf16(v)
    if kind == 'exact':
        assert torch.equal(e.double(), v.double()), f'{name}: exact-range case has non-representable outputs'
    elif kind == 'round':
        ties, inexact = bf16_stats(v)
        assert ties >= 0.20, f'{name}: only {ties:.1%} of the outputs are ties'
        assert inexact >= 0.40, f'{name}: only {inexact:.1%} of the outputs are inexact'
    else:
        raise ValueError(kind)
    return e


# ------------------------------------------------------------------------------------------- NT GEMM cases
def nt_operands(M, N, K, kind, seed=0, amp=2):
    """A [M,K], W [N,K] integer operands with ~12 non-zero terms per dot product, and a bias: small integers for
    'exact', 512 + small integers for 'round'."""
    p = density_for(K)
    A = ints((M, K), -1, 1, p, seed)
    W = ints((N, K), -amp, amp, p, seed + 1)
    bias = ints((N,), -16, 16, 1.0, seed + 2) + (512.0 if kind == 'round' else 0.0)
    return A, W, bias


def nt_reference(name, A, W, bias=None, h=None, scale=None, R=None):
    """Epilogue of vtx_gemm_nt in float64 with every fp32 intermediate checked exact:
    ((A W^T + bias) * h) * scale[:, None] + R  (each factor optional; h / R per element, scale per row)."""
    assert_acc_bound(name, A, W)
    v = A.double() @ W.double().t()
    assert_fp32_exact(f'{name} acc', v)
    if bias is not None:
        v = v + bias.double()
        assert_fp32_exact(f'{name} +bias', v)
    if h is not None:
        v = v * h.double()
        assert_fp32_exact(f'{name} *h', v)
    if scale is not None:
        v = v * scale.double()[:, None]
        assert_fp32_exact(f'{name} *scale', v)
    if R is not None:
        v = v + R.double()
        assert_fp32_exact(f'{name} +R', v)
    return v


# The token layout of the epilogue cases: B clips of 1 + P*T rows (a cls row, then the tokens).  Ntok = 788: the row-map
# group boundaries (788, 1576, ...) fall inside a 16-row epilogue pass (788 % 16 = 4) and inside a 64-row K tile of the
# TN GEMM (788 % 64 = 20).
TOK_B, TOK_P, TOK_T = 3, 197, 4
TOK_N = TOK_P * TOK_T

# vtx_gemm_nt epilogues with exact arithmetic (the GELU epilogues, act 1 / 2 and dgelu_kind 0, are not: exact_gelu.py and
# test_gpu_exact_gelu.py hold them to the fp32 kernel's values by equality and to float64 by a per-element bound;
# 'act_residual' is checked exactly on its pre-activation copy only)
NT_EPILOGUES = ('plain', 'bias', 'mul', 'scale', 'scale_split', 'residual', 'periodic', 'act_residual')


def nt_epilogue_case(epi, kind, N=320, K=192, seed=0):
    """One epilogue case of vtx_gemm_nt on the token layout, as CPU tensors and the float64 expected result.
    Returns a dict: M, N, K, A (physical rows), W, and for the call bias / h / scale / rs / R / r_period / split_row and the
    row maps as flags (amap_tok / cmap_tok / rmap_tok: ops.tokmap(TOK_N)); 'out' = 'tok' ([B, 1 + Ntok, N] output through
    the token map, cls rows untouched) or 'flat' ([M, N]); 'expected' (float64, the shape of the compared view) and, for
    split cases, 'expected_split' ([B*T, N])."""
    B, T = TOK_B, TOK_T
    M = B * TOK_N
    round_ = kind == 'round'
    c = dict(M=M, N=N, K=K, kind=kind, amap_tok=False, cmap_tok=False, rmap_tok=False, bias=None, h=None, scale=None,
             rs=(1, 0, 1, 0), R=None, r_period=0, split_row=0, out='flat', act=0)
    A, W, bias = nt_operands(M, N, K, kind, seed)
    c['W'] = W
    scales = dict(choices=(0.5, 1.0, 2.0)) if round_ else dict(choices=(0.0, 0.5, 1.0, 2.0))
    if epi == 'plain':
        assert not round_, 'plain has no offset to round with'
        c['A'] = A
        c['expected'] = nt_reference(epi, A, W)
    elif epi == 'bias':
        c['A'], c['bias'] = A, bias
        c['expected'] = nt_reference(epi, A, W, bias=bias)
    elif epi == 'mul':                                            # dgelu_kind 1: v *= dgelu_in[m][n]
        h = ints((M, N), -2, 2, 1.0, seed + 3)
        if round_:
            h = torch.where(h == 0, torch.ones_like(h), h)
        c['A'], c['bias'], c['h'] = A, bias, h
        c['expected'] = nt_reference(epi, A, W, bias=bias, h=h)
    elif epi == 'scale':                                          # row_scale, rs = (T, 1, 1, 0): s[m // T]
        s = dyadic_scales(M // T, seed + 4, **scales)
        c['A'], c['bias'], c['scale'], c['rs'] = A, bias, s, (T, 1, 1, 0)
        c['expected'] = nt_reference(epi, A, W, bias=bias, scale=s.repeat_interleave(T))
    elif epi in ('residual', 'act_residual'):                     # A and C and R rows through the token map
        X = torch.zeros(B, 1 + TOK_N, K)
        X[:, 1:] = A.reshape(B, TOK_N, K)
        X[:, 0] = ints((B, K), -1, 1, 1.0, seed + 5)             # cls rows the map must skip: non-zero
        R = ints((B, 1 + TOK_N, N), -32, 32, 1.0, seed + 6)
        c.update(A=X, bias=bias, R=R, amap_tok=True, cmap_tok=True, rmap_tok=True, out='tok')
        if epi == 'act_residual':                                # GELU output is checked against float64 with a tolerance
            c['act'] = 1
            c['expected_pre'] = nt_reference(epi, A, W, bias=bias)
        else:
            c['expected'] = nt_reference(epi, A, W, bias=bias, R=R[:, 1:].reshape(M, N)).reshape(B, TOK_N, N)
    elif epi == 'periodic':                                       # C rows through the token map, R row m % Ntok
        E = ints((TOK_N, N), -32, 32, 1.0, seed + 7)
        if round_:
            E = 512.0 + 4.0 * ints((TOK_N, N), -8, 8, 1.0, seed + 7)
        c.update(A=A, R=E, r_period=TOK_N, cmap_tok=True, out='tok')
        c['expected'] = nt_reference(epi, A, W, R=E.repeat(B, 1)).reshape(B, TOK_N, N)
    elif epi == 'scale_split':
        # M token rows then B*T cls rows (split_row = M) to Csplit; spatial scale index rs = (Ntok, T, T, 1):
        # token m -> s[(m // Ntok) * T + m % T], split row m -> s[m - M]; residual on token rows only
        Mo = M + B * T
        A2, _, _ = nt_operands(Mo, N, K, kind, seed + 8)
        s = dyadic_scales(B * T, seed + 9, **scales)
        R = ints((B, 1 + TOK_N, N), -32, 32, 1.0, seed + 6)
        m = torch.arange(M)
        tok_s = s[(m // TOK_N) * T + m % T]
        c.update(A=A2, M=Mo, bias=bias, scale=s, rs=(TOK_N, T, T, 1), R=R, rmap_tok=True, cmap_tok=True, out='tok',
                 split_row=M)
        c['expected'] = nt_reference(epi, A2[:M], W, bias=bias, scale=tok_s, R=R[:, 1:].reshape(M, N)).reshape(B, TOK_N, N)
        c['expected_split'] = nt_reference(epi + ' split', A2[M:], W, bias=bias, scale=s)
    else:
        raise ValueError(epi)
    return c


# Base shapes of the NT family cases, (M, N, K, kind); the branch each reaches is named in test_gpu_exact_arith.py.
NT_SHAPES = ((2352, 320, 192, 'exact'),      # 3 K tiles (odd; the ring minimum), ragged row tile (2352 = 9 * 256 + 48), ragged column tile
             (1100, 264, 256, 'round'),      # 4 K tiles (even), a column tile 8 wide
             (600, 136, 128, 'round'))       # 2 K tiles: the persistent kernel's minimum; below the rings' (they fall back to dma2)
NT_NODMA_SHAPES = ((300, 256, 96, 'exact'),  # K % 64 != 0: the register-staged kernel whatever the family
                   (130, 216, 8, 'round'))


def tn_operands(M, N1, N2, seed=0, lo=-3, hi=3):
    """Dense integer operands of the weight-gradient GEMM: |sum| <= M * 9, exact in fp32 for M < 1.8M."""
    return ints((M, N1), lo, hi, 1.0, seed), ints((M, N2), lo, hi, 1.0, seed + 1)


def tn_reference(name, A, B):
    """sum_m A[m]^T B[m] in float64 (A [M, N1], B [M, N2] as the kernel sees the mapped rows), checked fp32-exact."""
    assert_acc_bound(name, A.t(), B.t())
    v = A.double().t() @ B.double()
    assert_fp32_exact(name, v)
    return v


# ----------------------------------------------------------------------------------------------- checking
def sentinel_fill(t):
    """Fill t (bf16 or fp32) with the NaN sentinel bit pattern; returns t."""
    t.view(_INT[t.dtype]).fill_(SENT_BF16 if t.element_size() == 2 else SENT_F32)
    return t


def guarded(shape, dtype, device, pad_cols=8):
    """Output buffer [*shape[:-1], shape[-1] + pad_cols] filled with the sentinel: pass ld = shape[-1] + pad_cols to the
    kernel, compare buf[..., :shape[-1]], and hand buf[..., shape[-1]:] to check_exact as a sentinel region."""
    full = torch.empty(*shape[:-1], shape[-1] + pad_cols, dtype=dtype, device=device)
    return sentinel_fill(full)


def sentinel_touched(t):
    """Number of elements of the sentinel-filled tensor t that no longer hold the sentinel."""
    want = SENT_BF16 if t.element_size() == 2 else SENT_F32
    return int((t.contiguous().view(_INT[t.dtype]) != want).sum().item())


_sentinel_touched = sentinel_touched


def _tile_of(idx, shape):
    if len(shape) != 2:
        return ''
    r, c = idx
    return f' tile(128x128)=({r // 128},{c // 128}) tile(256x256)=({r // 256},{c // 256})'


def mismatch(got, expected):
    """Boolean mask of the elements where got (CPU) differs from expected (NaN matches NaN; +0 matches -0)."""
    assert got.shape == expected.shape, f'shape {tuple(got.shape)} != {tuple(expected.shape)}'
    assert got.dtype == expected.dtype, f'dtype {got.dtype} != {expected.dtype}'
    return ~((got == expected) | (torch.isnan(got) & torch.isnan(expected)))


def check_exact(name, got, expected, sentinel_regions=()):
    """got (device or CPU) equals expected (CPU, same dtype) element for element, and every sentinel region (a view of a
    sentinel-filled buffer the kernel must not touch; a list or a {label: view} dict) is bit-unchanged.  On failure the
    message names the count of wrong elements, the first few with their tiles, and the touched regions.  Writes one
    parity-report line."""
    got = got.detach().cpu()
    bad = mismatch(got, expected)
    nbad = int(bad.sum().item())
    msgs = []
    if nbad:
        where = bad.nonzero()[:6].tolist()
        shown = ', '.join(f'{tuple(i)}: got {got[tuple(i)].item():g} want {expected[tuple(i)].item():g}'
                          f'{_tile_of(i, got.shape)}' for i in where)
        msgs.append(f'{nbad} of {got.numel()} elements differ; first: {shown}')
    for label, region in (sentinel_regions.items() if isinstance(sentinel_regions, dict) else enumerate(sentinel_regions)):
        touched = sentinel_touched(region.detach())
        if touched:
            msgs.append(f'{touched} guard elements of region {label} overwritten')
    report(f'{"FAIL" if msgs else "ok  "} exact {name}: {got.numel()} elements'
           + (f' -- {"; ".join(msgs)}' if msgs else ''))
    assert not msgs, f'{name}: ' + '; '.join(msgs)
