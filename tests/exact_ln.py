"""Exact-arithmetic cases of the LayerNorm kernels (csrc/ln.hip) and their float64 references; importable without a GPU.

Built on tests/exact.py: small integers and dyadic scales, every fp32 intermediate asserted representable, so the correct
output is unique whatever the summation order or FMA contraction and is compared with equality.

Backward (vtx_layernorm_bwd F32 / BF16 / BF16_X32, vtx_layernorm_bwd_g32).  The kernel takes mean and rstd as inputs and is
algebraic in them:
    xh = (x - mu) rs,  g = dy gamma,  dgamma += sum_rows dy xh,  dbeta += sum_rows dy,
    c1 = sum g / D,  c2 = sum g xh / D,  dx = rs (g - c1 - xh c2) (+ dres)
so the builder supplies dyadic statistics (mu an integer, rs in {1/4, 1/2, 1} per row) that need not be the statistics of x.
  * dgamma / dbeta hold no 1/D: exact for every D and every row count.
  * Every row is of one of two kinds (drawn per row, about half each):
      mirrored    columns j and j + D/2 carry equal x and gamma and opposite dy (dense): both row sums are exactly zero and
                  dx = rs g + dres is exact whatever 1/D rounds to;
      unmirrored  sparse dy (density_for), non-zero row sums.  For D a power of two 1/D and both products with it are exact, and
                  so is dx.  For other D, dx is held to a per-element bound against float64, derived from the operation count:
                  c1 and c2 carry at most two roundings each (1/D and the product), xh c2 one more, the two subtractions one
                  each, rs is a power of two, the residual add one -- at most 5 u rs (|g| + |c1| + |xh c2|) + u |dres| with
                  u = 2^-24, rounded up to
                      8 * 2^-24 * (rs (|g| + |c1| + |xh c2|) + |dres|)
                  plus half a bf16 ulp of the reference where the store is bf16 (contracted FMAs only remove roundings).
  * bf16 stores with a residual are rounding cases (exact.expect_bf16 'round'): in the mirrored rows the residual of an element
    is placed in the binade whose bf16 spacing is twice the lowest set bit of rs g, so rs g + dres is an exact tie; the
    unmirrored rows are inexact through c1 / c2.

Forward (vtx_layernorm_fwd fp32 / bf16, vtx_layernorm_acc_fwd).  x = m + d with d sparse integers, d[j + D/2] = -d[j]: the row
sum is exactly D m.  For D a power of two m is a small integer per row and mean and variance are exact; for other D m = 0, so
mu = 0 whatever 1/D rounds to (so the 3- and 6-chunk instantiations, whose D is never a power of two, subtract a zero mean: a
fault in their `x - mu` alone is not seen here; NCH 1, 2, 4 and 8 run it with m != 0).  mean_out is checked with equality;
rstd_out against float64 (var + eps)^-1/2 within 4 ulp (relative 2^-21: 1/D, one product and the eps add move the argument by at most 1.5 ulp, halved by the square root; the rest is
margin for rsqrtf, whose largest observed distance goes into the report); y is then exact GIVEN the kernel's own rstd_out:
t = fl32(d rstd), y = fl32(t gamma + beta), t gamma exact (gamma a power of two), so FMA and multiply-add round alike.
"""
import torch

import exact as X
from helpers import report

TOK_N = 37                    # tokens per clip of the [B, 1 + N, ld] operand buffers (a cls row every 38 physical rows)
PAD = 8                       # ld = D + PAD
U = 2.0 ** -24
EPS = 1e-5
RSTD_ULPS = 4.0


def is_pow2(n):
    return n & (n - 1) == 0


# ------------------------------------------------------------------------------------------------ layout
class Layout:
    """Logical row m -> physical row base + m + (m // n) * skip of a flat [phys, ld] buffer (ops.rowmap(n, skip, base); the
    default is ops.tokmap(TOK_N) on a [B, 1 + N, ld] tensor whose last clip may be partly filled) plus two trailing rows.
    With `table` (an exact_tab.TabLayout of `rows` logical rows) the rows are placed and gathered through the table's index
    vector base + m + tab[m // grp] instead, the buffer has the table layout's row count, and rowmap() is ops.tabmap(...)."""

    def __init__(self, rows, n=TOK_N, skip=1, base=1, table=None):
        self.table = table
        if table is not None:
            assert rows == table.M
            n, skip, base = table.grp, table.max_step, table.base
        self.rows, self.n, self.skip, self.base = rows, n, skip, base
        m = torch.arange(rows)
        self.idx = base + m + (m // n) * skip if table is None else table.rows
        self.phys = int(self.idx[-1]) + 3 if table is None else table.phys
        self.clips = (rows + n - 1) // n
        self.unmapped = torch.ones(self.phys, dtype=torch.bool)
        self.unmapped[self.idx] = False

    def rowmap(self, ops):
        if self.table is not None:
            return self.table.rowmap(ops)
        return ops.rowmap(self.n, self.skip, self.base)

    def place(self, vals, dtype=torch.float32, seed=0, pad=PAD):
        """Input buffer [phys, D + pad]: vals on the mapped rows, non-zero junk integers everywhere else."""
        D = vals.shape[1]
        buf = X.ints((self.phys, D + pad), 1, 5, 1.0, seed + 977) * 7.0
        buf[self.idx, :D] = vals.float()
        return buf.to(dtype)

    def out(self, D, dtype, device, pad=PAD):
        return X.guarded((self.phys, D), dtype, device, pad)

    def got(self, buf, D):
        return buf[self.idx.to(buf.device), :D]

    def guards(self, buf, D, unmapped=None):
        um = (self.unmapped if unmapped is None else unmapped).to(buf.device)
        return {'ld padding': buf[:, D:], 'unmapped rows': buf[um, :D]}


def assert_sums_exact(name, terms, dim, q, extra=0.0):
    """Every partial sum of `terms` along dim, in any order, is fp32-exact: the terms are multiples of the power of two q and
    (sum |terms| + extra) / q < 2^24."""
    t = terms.double()
    assert torch.equal((t / q).round(), t / q), f'{name}: a term is no multiple of {q:g}'
    b = (t.abs().sum(dim).max().item() + extra) / q
    assert b < X.EXACT_LIMIT, f'{name}: partial sums reach {b:g} units of {q:g} (>= 2^24)'


def tie_offsets(u, seed):
    """Per element of u (multiples of 1/8, |u| <= 6): a bf16-representable offset r with u + r an exact bf16 tie -- r lies in
    the binade [256 s, 512 s) with s the lowest set bit of u, whose bf16 spacing is 2 s; where u == 0, a small integer."""
    g = X.gen(seed)
    k = (u.double() * 8).round().long().abs()
    s = (k & -k).double() / 8
    mag = s * 256 + 2 * s * torch.randint(8, 101, u.shape, generator=g).double()
    sign = torch.randint(0, 2, u.shape, generator=g).double() * 2 - 1
    small = torch.randint(-32, 33, u.shape, generator=g).double()
    return torch.where(k == 0, small, sign * mag)


def half_bf16_ulp(v):
    """Half the bf16 spacing at |v| (float64; 0 at 0)."""
    _, e = torch.frexp(v.double().abs())
    return torch.where(v == 0, torch.zeros_like(v, dtype=torch.float64), torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 9))


# ------------------------------------------------------------------------------------------------ backward
BWD_KINDS = ('f32', 'bf16', 'x32', 'g32')      # VTX_F32, VTX_BF16, VTX_BF16_X32, vtx_layernorm_bwd_g32


def bwd_case(rows, D, kind, res=True, seed=0):
    """One backward case as CPU float32 tensors in logical row order and the float64 expected results.
    Keys: x, dy, mu, rs, gamma, dres (None without residual; the float32 dres32 for 'g32'), dg0 / db0 (entry values),
    dgamma / dbeta (float64, entry included), dx (float64), exact_rows (bool per row: dx is checked with equality),
    bound (float64 [rows, D], meaningful on the other rows, without the bf16 half ulp), round (bf16 outputs are a
    rounding case)."""
    assert kind in BWD_KINDS and D % 4 == 0 and (res or kind != 'g32')
    g = X.gen(seed)
    pow2, h = is_pow2(D), D // 2
    mir = torch.rand(rows, generator=g) < 0.5
    mir[:2] = torch.tensor([True, False])[:rows]          # both kinds wherever there are two rows
    rs = X.dyadic_scales(rows, seed + 1, choices=(0.25, 0.5, 1.0))
    # a float32 x (x32 / g32) sits where bf16 could not hold it: integers near 300
    mu = X.ints((rows,), -2, 2, 1.0, seed + 2) + (300.0 if kind in ('x32', 'g32') else 0.0)
    x = mu[:, None] + X.ints((rows, D), -6, 6, 1.0, seed + 3)
    gamma = X.dyadic_scales(D, seed + 4, choices=(0.5, 1.0, 2.0)) * (X.ints((D,), 0, 1, 1.0, seed + 5) * 2 - 1)
    gamma[h:2 * h] = gamma[:h]
    dense = X.ints((rows, D), 1, 3, 1.0, seed + 6) * (X.ints((rows, D), 0, 1, 1.0, seed + 7) * 2 - 1)
    dy = torch.where(mir[:, None], dense, X.ints((rows, D), -3, 3, X.density_for(D), seed + 8))
    x[:, h:2 * h] = torch.where(mir[:, None], x[:, :h], x[:, h:2 * h])
    dy[:, h:2 * h] = torch.where(mir[:, None], -dy[:, :h], dy[:, h:2 * h])
    dg0 = X.ints((D,), 1, 50, 1.0, seed + 9) * (X.ints((D,), 0, 1, 1.0, seed + 10) * 2 - 1)
    db0 = X.ints((D,), 1, 50, 1.0, seed + 11) * (X.ints((D,), 0, 1, 1.0, seed + 12) * 2 - 1)

    name = f'ln_bwd {kind} {rows}x{D}'
    xh = (x.double() - mu.double()[:, None]) * rs.double()[:, None]
    gg = dy.double() * gamma.double()
    X.assert_fp32_exact(f'{name} xh', xh)
    X.assert_fp32_exact(f'{name} g', gg)
    assert_sums_exact(f'{name} dgamma', dy.double() * xh, 0, 0.25, extra=50.0)
    assert_sums_exact(f'{name} dbeta', dy, 0, 1.0, extra=50.0)
    dgamma = dg0.double() + (dy.double() * xh).sum(0)
    dbeta = db0.double() + dy.double().sum(0)
    gx = gg * xh
    assert_sums_exact(f'{name} sum g', gg, 1, 0.5)
    assert_sums_exact(f'{name} sum g xh', gx, 1, 0.125)
    s1, s2 = gg.sum(1), gx.sum(1)
    del gx
    assert bool((s1[mir] == 0).all()) and bool((s2[mir] == 0).all()), f'{name}: a mirrored row has a non-zero sum'
    c1, c2 = (s1 / D)[:, None], (s2 / D)[:, None]
    exact_rows = torch.ones(rows, dtype=torch.bool) if pow2 else mir.clone()
    t = xh * c2
    a = gg - c1
    b = a - t
    o = rs.double()[:, None] * b
    for nm, v in (('c1', c1), ('c2', c2), ('xh c2', t), ('g - c1', a), ('g - c1 - xh c2', b), ('rs (...)', o)):
        X.assert_fp32_exact(f'{name} {nm}', v[exact_rows])
    bound = 8 * U * rs.double()[:, None] * (gg.abs() + c1.abs() + t.abs())
    del t, a, b
    dres = None
    if res:
        if kind == 'f32':
            dres = X.ints((rows, D), -32, 32, 1.0, seed + 13)
        else:
            plain = X.ints((rows, D), -32, 32, 1.0, seed + 13)
            if kind == 'g32':                      # float32 residual gradient: values bf16 could not hold
                plain = plain + X.ints((rows, D), -3, 3, 1.0, seed + 14) * 2.0 ** -9
            dres = torch.where(mir[:, None], tie_offsets(o, seed + 15).float(), plain)
        o = o + dres.double()
        X.assert_fp32_exact(f'{name} + dres', o[exact_rows])
        bound = bound + 8 * U * dres.double().abs()
    return dict(name=name, rows=rows, D=D, kind=kind, x=x, dy=dy, mu=mu, rs=rs, gamma=gamma, dres=dres, dg0=dg0, db0=db0,
                dgamma=dgamma, dbeta=dbeta, dx=o, exact_rows=exact_rows, mirrored=mir, bound=bound,
                round=res and kind != 'f32', xh=xh, g=gg, c1=c1, c2=c2)


def bwd_expected_dx(c):
    """(fp32 expected, bf16 expected or None) of the exactly checked rows; asserts the rounding premise on bf16 cases."""
    v = c['dx'][c['exact_rows']]
    X.assert_fp32_exact(f"{c['name']} dx", v)
    if c['kind'] == 'f32':
        return v.float(), None
    return v.float(), (X.expect_bf16(f"{c['name']} dx", v, 'round') if c['round'] else X.rne_bf16(v))


def check_bounded(name, got, ref, bound, store_half_ulp=None):
    """|got - ref| <= bound (+ store_half_ulp, for a bf16 store) element for element (float64).  Reports the largest used
    fraction of the bound for float32 stores; a bf16 store hides the float32 error behind its own rounding (an element next
    to a rounding boundary uses the whole half ulp), so no fraction is reported for it."""
    got = got.detach().double().cpu()
    if store_half_ulp is not None:
        bound = bound + store_half_ulp
    if got.numel() == 0:
        report(f'ok   bound {name}: 0 elements')
        return 0.0
    err = (got - ref).abs()
    bad = ~(err <= bound)                      # a NaN fails
    inf = torch.full_like(err, float('inf'))
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
    worst = float(frac.nan_to_num(nan=float('inf')).max())
    nbad = int(bad.sum())
    msg = ''
    if nbad:
        i = tuple(bad.nonzero()[0].tolist())
        msg = f' -- {nbad} elements beyond their bound; first {i}: got {got[i].item():.9g} want {ref[i].item():.9g} bound {bound[i].item():.3g}'
    used = 'bf16 store, no fraction' if store_half_ulp is not None else f'largest used fraction of the bound {worst:.3f}'
    report(f'{"FAIL" if nbad else "ok  "} bound {name}: {got.numel()} elements, {used}{msg}')
    assert not nbad, f'{name}:{msg}'
    return worst


# ------------------------------------------------------------------------------------------------- forward
def eps32():
    return float(torch.tensor(EPS, dtype=torch.float32))       # the float the ABI receives


def fwd_case(rows, D, kind, seed=0):
    """One forward case ('f32' / 'bf16' for vtx_layernorm_fwd; 'acc' / 'acc0' for vtx_layernorm_acc_fwd with / without xs:
    the row is xs + d resp. d) as CPU float32 tensors and the float64 statistics.  Keys: x (the float32 row the statistics
    are of), xs / d (acc forms), gamma, beta, dev (x - mean), mean, rstd (float64)."""
    assert kind in ('f32', 'bf16', 'acc', 'acc0') and D % 4 == 0
    pow2, h = is_pow2(D), D // 2
    name = f'ln_fwd {kind} {rows}x{D}'
    m = X.ints((rows,), -3, 3, 1.0, seed) if pow2 else torch.zeros(rows)
    dev = X.ints((rows, D), -4, 4, 0.6, seed + 1)
    dev[:, h:2 * h] = -dev[:, :h]
    x = m[:, None] + dev
    gamma = X.dyadic_scales(D, seed + 2, choices=(0.5, 1.0, 2.0)) * (X.ints((D,), 0, 1, 1.0, seed + 3) * 2 - 1)
    if kind == 'f32':
        beta = X.ints((D,), -16, 16, 1.0, seed + 4)
    else:       # bf16 y: where dev == 0, y = beta is an exact tie of the spacing-4 binade
        beta = (514.0 + 4.0 * X.ints((D,), 0, 120, 1.0, seed + 4)) * (X.ints((D,), 0, 1, 1.0, seed + 5) * 2 - 1)
    assert_sums_exact(f'{name} sum x', x, 1, 1.0)
    assert torch.equal(x.double().sum(1), D * m.double())
    if pow2:
        X.assert_fp32_exact(f'{name} mean', x.double().sum(1) / D)
    assert_sums_exact(f'{name} sum d^2', dev * dev, 1, 1.0)
    var = (dev.double() ** 2).sum(1) / D
    if pow2:
        X.assert_fp32_exact(f'{name} var', var)
    c = dict(name=name, rows=rows, D=D, kind=kind, x=x, gamma=gamma, beta=beta, dev=dev, mean=m.double(),
             rstd=(var + eps32()) ** -0.5)
    if kind == 'acc':       # d bf16 integers, xs float32: xs + d = x exactly
        d = X.ints((rows, D), -100, 100, 1.0, seed + 6)
        c['d'], c['xs'] = d, x - d
    elif kind == 'acc0':
        c['d'], c['xs'] = x, None
    return c


def ulp_distance(got, ref):
    """|got - ref| in units of the fp32 spacing at ref (float64 ref)."""
    _, e = torch.frexp(ref.double().abs())
    return (got.double() - ref.double()).abs() / torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - 24)


def check_rstd(name, got, ref):
    """rstd_out within RSTD_ULPS of the float64 value; the largest distance goes into the report.  Returns it."""
    d = ulp_distance(got.detach().cpu(), ref)
    worst = float(d.nan_to_num(nan=float('inf')).max())
    ok = worst <= RSTD_ULPS
    report(f'{"ok  " if ok else "FAIL"} rstd {name}: {ref.numel()} rows, largest distance {worst:.3f} ulp (bar {RSTD_ULPS:g})')
    assert ok, f'{name}: rstd_out {worst:.3f} ulp from float64 (row {int(d.argmax())})'
    return worst


def fwd_expected_y(c, rstd32):
    """y given the kernel's own (already checked) rstd_out, float32 CPU [rows]: fl32(fl32(d rstd) gamma + beta) as float32,
    and its RNE for bf16 outputs (asserting the rounding premise)."""
    t = (c['dev'].double() * rstd32.double()[:, None]).float()
    y = (t.double() * c['gamma'].double() + c['beta'].double()).float()
    if c['kind'] == 'f32':
        return y
    return X.expect_bf16(f"{c['name']} y", y.double(), 'round')


# --------------------------------------------------------------------------------------- the GPU file's tables
EDGE_D = (256, 128)                                            # FULL and ragged single-chunk rows
BWD_EDGE_ROWS = (1, 3, 5, 2032, 2033, 20487, 24581)            # also vtx_layernorm_acc_fwd
FWD_EDGE_ROWS = (1, 7, 8193, 32773)
INST_ROWS = 2100                                               # 132 partial slabs: the wide partial reduce
INST_D = (64, 200, 256, 384, 512, 600, 768, 960, 1024)
INST_D_WIDE = (1280, 1536, 1800, 2048)                         # NCH 6 and 8; vtx_layernorm_fwd / vtx_layernorm_bwd only
BENCH_ROWS, BENCH_D = 24581, 768


def bwd_table():
    """(rows, D, kind, res) of every backward case the GPU file runs."""
    out = [(r, D, k, True) for D in EDGE_D for k in ('f32', 'bf16') for r in BWD_EDGE_ROWS]
    out += [(BENCH_ROWS, BENCH_D, 'bf16', True), (BENCH_ROWS, BENCH_D, 'g32', True)]
    for D in INST_D + INST_D_WIDE:
        out += [(INST_ROWS, D, k, res) for k in ('f32', 'bf16') for res in (True, False)]
    out += [(INST_ROWS, D, 'x32', res) for D in INST_D for res in (True, False)]
    out += [(INST_ROWS, D, 'g32', True) for D in INST_D]
    return out


def fwd_table():
    """(rows, D, kind) of every forward case the GPU file runs."""
    out = [(r, D, k) for D in EDGE_D for k in ('f32', 'bf16') for r in FWD_EDGE_ROWS]
    out += [(r, D, 'acc') for D in EDGE_D for r in BWD_EDGE_ROWS]
    out += [(BENCH_ROWS, BENCH_D, 'acc')]
    out += [(INST_ROWS, D, k) for D in INST_D + INST_D_WIDE for k in ('f32', 'bf16')]
    out += [(INST_ROWS, D, k) for D in INST_D for k in ('acc', 'acc0')]
    return out


def case_seed(rows, D):
    return 13 * rows + D
