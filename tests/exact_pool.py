"""Exact-arithmetic cases of the MViT pooling, position and stem kernels (csrc/mvit.hip) and their float64 references;
importable without a GPU.  Built on tests/exact.py and tests/exact_ln.py.

Forward (vtx_pool_conv_ln_fwd: pre, y, mean, rstd).  x holds sparse small integers, the conv weights integers in [-2, 2] drawn
per (channel, tap), so `pre` is an integer tensor (|pre| <= 256: a bf16 store keeps it) compared with equality against
torch.nn.functional.conv3d in float64; the cls row is copied through.  The LayerNorm half, per (token, head) row of width hd:
  hd 64   mu = S / 64 and q = sum (v - mu)^2 are exact dyadic values (asserted): mean is compared with equality, rstd within
          exact_ln.RSTD_ULPS of float64 (q / 64 + eps)^-1/2 (the division q / HD is one rounding, as the product with 1/D is
          there), and y with equality GIVEN the kernel's own rstd: t = fl32((v - mu) rstd), y = fl32(t gamma + beta); gamma is
          a power of two, so t gamma is exact and the contracted and the uncontracted form round alike.
  hd 96   an input (token, head) is mirrored -- channel j + 48 carries -x of channel j, with equal conv weights -- or, at a rate
          that leaves about one output row in four unmirrored, not.  An output row whose window holds only mirrored inputs
          has pre[j + 48] = -pre[j]: its sum is exactly 0, mu = 0 whatever 1/96 rounds to, and the hd-64 checks apply.
          On the other rows mean must equal fl32(S / 96), one IEEE division of an exact integer; y is held to a per-element
          bound against the float64 value y* = (v - S/96) rstd gamma + beta, rstd being the kernel's own: the rounding of mu
          moves v - mu by u |mu| (u = 2^-24), the subtraction and the product with rstd by u |v - mu| each, the product with
          gamma is exact, the add of beta rounds the result once -- u (rstd |gamma| (|mu| + 2 |v - mu|) + |y*|) to first
          order, rounded up to
              4 * 2^-24 * (rstd |gamma| (|mu| + |v - mu|) + |y*|)
          plus half a bf16 ulp where the store is bf16.  rstd of these rows: the error of mu enters q only in second order
          (sum (v - mu) = 0), each v - mu, each square, the seven adds per lane, the four shuffle adds, the division and the
          eps add round once: at most 16 u relative on the argument, halved by the square root -- 8 ulp on top of the 4 of
          the exact rows (RSTD_ULPS_UNMIRRORED).
  'round' one bf16 case, every row mirrored and x sparser: about half of pre is 0, where y = beta, an exact tie of the
          spacing-4 binade (beta = +-(514 + 4 k)); the other outputs are inexact through rstd.

Backward (vtx_pool_conv_ln_bwd: dpre, dx, dw, dgamma, dbeta).  The entry point is algebraic in pre, mean and rstd and x feeds only
dw, so each is supplied independently, as exact_ln.bwd_case does: mean integers, rstd in {1/4, 1/2, 1} per row, rows mirrored
(equal pre and gamma, opposite dense dy: both row sums zero, dpre = rs g exact) or unmirrored (sparse dy).  At hd 64 every
intermediate of an unmirrored row is dyadic (asserted) and a bf16 dpre is RNE of the exact value; at hd 96 dpre of those rows is
held to exact_ln's derived bound without the residual, 8 * 2^-24 * rs (|g| + |c1| + |xh c2|) (+ half a bf16 ulp).  dgamma /
dbeta hold no 1/hd: exact at every hd.  The expected dx and dw are computed from the expected STORED dpre (rounded to bf16
where it is bf16), which is what the conv kernels read back:
  * every row exact and sum |dpre| |w| resp. sum |dpre| |x| below 2^24 units of dpre's common power-of-two unit: dx, dw are
    exact sums, compared with equality (mode 'mirrored' -- every row mirrored, dpre multiples of 1/8 -- at every shape);
  * otherwise (mode 'mixed' with unmirrored hd-96 rows, or sums too fine for fp32) against float64 within the bound carried
    through the linear maps, |w| delta resp. |x| delta summed over the taps / pairs, delta = dpre's bound (+ a bf16 ulp), plus
    the summation's own rounding, (depth of the sum) u sum |terms| -- 27 for dx; for dw a block's chain over its pairs and
    heads and then at most one add per block's partial -- plus half a bf16 ulp on a bf16 dx.
"""
import functools
import itertools

import torch
import torch.nn.functional as TF

import exact as X
import exact_ln as L

U = L.U
RSTD_ULPS_UNMIRRORED = L.RSTD_ULPS + 8.0
F32, BF16 = torch.float32, torch.bfloat16

# (B, heads, hd, (T, H, W), (sh, sw), dtypes, backward modes); test_gpu_exact_pool.py names the branch each reaches
BOTH = ('f32', 'bf16')
TABLE = (
    (2, 2, 96, (2, 7, 12), (2, 4), BOTH, ('mixed', 'mirrored')),
    (2, 3, 64, (3, 8, 5), (4, 2), BOTH, ('mixed', 'mirrored')),
    (2, 1, 96, (1, 5, 6), (8, 8), BOTH, ('mixed', 'mirrored')),
    (1, 2, 64, (2, 1, 9), (1, 2), BOTH, ('mixed', 'mirrored')),
    (2, 4, 96, (2, 5, 7), (1, 1), BOTH, ('mixed', 'mirrored')),
    (2, 2, 64, (2, 8, 8), (2, 2), BOTH, ('mixed', 'mirrored')),
    (2, 2, 64, (2, 32, 32), (1, 1), BOTH, ('mixed', 'mirrored')),
    (2, 1, 64, (4, 130, 130), (1, 1), ('bf16',), ('mirrored',)),
    (2, 1, 96, (4, 130, 130), (1, 1), ('f32',), ('mirrored',)),
)
ROUND_SHAPE = TABLE[0][:5]                   # the one bf16 'round' forward case
OLD_SHAPES = ((2, 2, 96, (2, 8, 8), (2, 2)), (2, 1, 96, (2, 16, 16), (8, 8)), (2, 3, 64, (3, 8, 12), (4, 4)),
              (2, 4, 96, (2, 5, 7), (1, 1)))          # test_gpu_mvit.test_pool_conv_ln: sh == sw throughout
LN_GRID, W_BLOCKS, PB = 1024, 2048, 64       # launch constants of vtx_pool_conv_ln_bwd


def shapes():
    return [t[:5] for t in TABLE]


def fwd_table():
    out = [(t[:5], dt, 'plain') for t in TABLE for dt in t[5]]
    return out + [(ROUND_SHAPE, 'bf16', 'round')]


def bwd_table():
    return [(t[:5], dt, mode) for t in TABLE for dt in t[5] for mode in t[6]]


def case_seed(shape):
    B, heads, hd, (T, H, W), (sh, sw) = shape
    return 7 * hd + 131 * heads + 17 * T + 1009 * H + 53 * W + 3 * sh + sw


def pooled(n, s):
    return (n - 1) // s + 1


def dims(shape):
    B, heads, hd, (T, H, W), (sh, sw) = shape
    Ho, Wo = pooled(H, sh), pooled(W, sw)
    return dict(B=B, heads=heads, hd=hd, T=T, H=H, W=W, sh=sh, sw=sw, Ho=Ho, Wo=Wo, C=heads * hd, n_in=1 + T * H * W,
                n_out=1 + T * Ho * Wo, units=B * (1 + T * Ho * Wo) * heads, pairs=B * T * Ho * Wo)


def signs(shape, seed):
    return X.ints(shape, 0, 1, 1.0, seed) * 2 - 1


# ------------------------------------------------------------------------------------- float64 references
def _wt(w, heads):
    """[hd, 27] -> depthwise Conv3d weight [heads * hd, 1, 3, 3, 3] (column c uses w[c % hd])."""
    return w.double().reshape(-1, 1, 3, 3, 3).repeat(heads, 1, 1, 1, 1)


def conv_ref(x, w, shape):
    """pre [B, n_out, C] in float64: conv3d (groups = C) on the [B, C, T, H, W] view of the grid tokens, cls row copied."""
    d = dims(shape)
    g = x[:, 1:].double().reshape(d['B'], d['T'], d['H'], d['W'], d['C']).permute(0, 4, 1, 2, 3)
    o = TF.conv3d(g, _wt(w, d['heads']), stride=(1, d['sh'], d['sw']), padding=1, groups=d['C'])
    assert tuple(o.shape[2:]) == (d['T'], d['Ho'], d['Wo'])
    return torch.cat([x[:, :1].double(), o.flatten(2).transpose(1, 2)], 1)


def conv_T_ref(dpre, w, shape):
    """dx [B, n_in, C] in float64: the transposed depthwise conv of dpre's grid rows; the cls row passes through."""
    d = dims(shape)
    g = dpre[:, 1:].double().reshape(d['B'], d['T'], d['Ho'], d['Wo'], d['C']).permute(0, 4, 1, 2, 3)
    op = (0, d['H'] - 1 - (d['Ho'] - 1) * d['sh'], d['W'] - 1 - (d['Wo'] - 1) * d['sw'])
    o = TF.conv_transpose3d(g, _wt(w, d['heads']), stride=(1, d['sh'], d['sw']), padding=1, output_padding=op, groups=d['C'])
    assert tuple(o.shape[2:]) == (d['T'], d['H'], d['W'])
    return torch.cat([dpre[:, :1].double(), o.flatten(2).transpose(1, 2)], 1)


def dw_ref(dpre, x, shape, pair_weight=None):
    """dw [hd, 27] in float64: dw[c][tap] = sum over (b, output token) pairs and heads of dpre * x at the tap's position
    (pair_weight [pairs]: each pair counted that many times)."""
    d = dims(shape)
    B, T, H, W, Ho, Wo, sh, sw, C = (d[k] for k in ('B', 'T', 'H', 'W', 'Ho', 'Wo', 'sh', 'sw', 'C'))
    xp = TF.pad(x[:, 1:].double().reshape(B, T, H, W, C), (0, 0, 1, 1, 1, 1, 1, 1))
    g = dpre[:, 1:].double().reshape(B, T, Ho, Wo, C)
    if pair_weight is not None:
        g = g * pair_weight.double().reshape(B, T, Ho, Wo, 1)
    out = torch.zeros(C, 27, dtype=torch.float64)
    for kt, kh, kw in itertools.product(range(3), repeat=3):
        xs = xp[:, kt:kt + T, kh:kh + (Ho - 1) * sh + 1:sh, kw:kw + (Wo - 1) * sw + 1:sw]
        out[:, (kt * 3 + kh) * 3 + kw] = (g * xs).sum((0, 1, 2, 3))
    return out.reshape(d['heads'], d['hd'], 27).sum(0)


def dyadic_unit(v):
    """The largest power of two (<= 1) that divides every element of v (float64, fp32-exact values)."""
    q = 1.0
    for _ in range(60):
        t = v / q
        if torch.equal(t.round(), t):
            return q
        q /= 2
    raise AssertionError('not dyadic')


# ------------------------------------------------------------------------------------------------ forward
X_DENSITY, ROUND_DENSITY = 0.15, 0.06


@functools.lru_cache(maxsize=4)
def fwd_case(shape, dt, kind='plain'):
    """One forward case as CPU float32 tensors and the float64 expected values.  Keys: x [B, n_in, C], w [hd, 27], gamma, beta,
    pre (float64 [B, n_out, C]), exact (bool per unit: mirrored or hd 64), S, mean (float64 S / hd), mean32 (the float32 the
    kernel must store), dev (pre - mean per unit [units, hd]), rstd (float64)."""
    d = dims(shape)
    B, heads, hd, n_in, C = d['B'], d['heads'], d['hd'], d['n_in'], d['C']
    seed = case_seed(shape) + (500 if kind == 'round' else 0)
    name = f'pool_fwd {dt} {kind} {shape}'
    assert kind == 'plain' or (dt == 'bf16' and hd == 96)
    g = X.gen(seed)
    x = X.ints((B, n_in, heads, hd), -2, 2, ROUND_DENSITY if kind == 'round' else X_DENSITY, seed + 1)
    x[:, 0] = X.ints((B, heads, hd), 1, 3, 1.0, seed + 2) * signs((B, heads, hd), seed + 3)      # cls: non-zero, per clip
    w = X.ints((hd, 27), -2, 2, 1.0, seed + 4)
    if hd == 96:
        w[48:] = w[:48]
        unm = torch.zeros(B, n_in, heads, dtype=torch.bool)
        if kind == 'plain':
            # inputs per window on average -> the input rate that leaves about one output row in four unmirrored
            ones = torch.ones(1, 1, d['T'], d['H'], d['W'], dtype=torch.float64)
            n_eff = float(TF.conv3d(ones, torch.ones(1, 1, 3, 3, 3, dtype=torch.float64), stride=(1, d['sh'], d['sw']), padding=1).mean())
            unm = torch.rand(B, n_in, heads, generator=g) < 1 - 0.75 ** (1 / n_eff)
            unm[:, 0] = torch.rand(B, heads, generator=g) < 0.25
            unm[0, 1, 0] = True
            unm[0, 0, 0] = False
            unm[B - 1, 0, heads - 1] = True
        x[..., 48:] = torch.where(unm[..., None], x[..., 48:], -x[..., :48])
    x = x.reshape(B, n_in, C)
    gamma = X.dyadic_scales(hd, seed + 5, choices=(0.5, 1.0, 2.0)) * signs((hd,), seed + 6)
    if kind == 'round':
        beta = (514.0 + 4.0 * X.ints((hd,), 0, 120, 1.0, seed + 7)) * signs((hd,), seed + 8)
    else:
        beta = X.ints((hd,), -64, 64, 1.0, seed + 7) / 4
    pre = conv_ref(x, w, shape)
    assert torch.equal(pre.round(), pre) and float(pre.abs().max()) <= 256, f'{name}: pre is no integer tensor within +-256'
    assert torch.equal(x.to(BF16).float(), x)
    v = pre.reshape(d['units'], hd)
    S = v.sum(1)
    exact = torch.ones(d['units'], dtype=torch.bool) if hd == 64 else (v[:, 48:] == -v[:, :48]).all(1)
    mean = S / hd
    X.assert_fp32_exact(f'{name} mean', mean[exact])
    if hd == 96:
        assert bool((S[exact] == 0).all())
    dev = v - mean[:, None]
    X.assert_fp32_exact(f'{name} v - mu', dev[exact])
    L.assert_sums_exact(f'{name} sum (v - mu)^2', (dev * dev)[exact], 1, 2.0 ** -12)
    q = (dev * dev).sum(1)
    rstd = (q / hd + L.eps32()) ** -0.5
    return dict(name=name, shape=shape, dt=dt, kind=kind, d=d, x=x, w=w, gamma=gamma, beta=beta, pre=pre, exact=exact, S=S,
                mean=mean, mean32=(S.float() / hd), dev=dev, rstd=rstd)


def fwd_expected_y(c, rstd32):
    """Given the kernel's own rstd (float32 CPU [units]): (y of the exact rows as the stored dtype, float64 y* of the other
    rows, their bound without the bf16 half ulp)."""
    ex, g, b = c['exact'], c['gamma'].double(), c['beta'].double()
    rs = rstd32.double()[:, None]
    t = (c['dev'][ex] * rs[ex]).float()
    y = (t.double() * g + b).float()
    if c['dt'] == 'bf16':
        y = X.expect_bf16(f"{c['name']} y", y.double(), 'round') if c['kind'] == 'round' else y.to(BF16)
    dv, mu = c['dev'][~ex], c['mean'][~ex][:, None]
    ystar = dv * rs[~ex] * g + b
    bound = 4 * U * (rs[~ex] * g.abs() * (mu.abs() + dv.abs()) + ystar.abs())
    return y, ystar, bound


# ----------------------------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=2)
def bwd_case(shape, dt, mode):
    """One backward case ('mixed': about half the rows mirrored; 'mirrored': all) as CPU float32 tensors and the float64
    expected results.  Keys: pre, dy [B, n_out, C], x [B, n_in, C], mu, rs [units], w, gamma, dgamma, dbeta, dpre (float64
    [units, hd]), exact_rows, bound, stored (float64 of the expected stored dpre, [B, n_out, C]), dx, dw (float64, from
    `stored`), sums_exact (dx / dw are compared with equality) and, where not, dx_bound / dw_bound."""
    d = dims(shape)
    B, heads, D, C, rows = d['B'], d['heads'], d['hd'], d['C'], d['units']
    seed = case_seed(shape) + (900 if mode == 'mirrored' else 700)
    name = f'pool_bwd {dt} {mode} {shape}'
    g = X.gen(seed)
    pow2, h = L.is_pow2(D), D // 2
    if mode == 'mirrored':
        mir = torch.ones(rows, dtype=torch.bool)
    else:
        mir = torch.rand(rows, generator=g) < 0.5
        mir[:2] = torch.tensor([True, False])
    rs = X.dyadic_scales(rows, seed + 1, choices=(0.25, 0.5, 1.0))
    mu = X.ints((rows,), -2, 2, 1.0, seed + 2)
    pre = mu[:, None] + X.ints((rows, D), -6, 6, 1.0, seed + 3)
    gamma = X.dyadic_scales(D, seed + 4, choices=(0.5, 1.0, 2.0)) * signs((D,), seed + 5)
    gamma[h:] = gamma[:h]
    dense = X.ints((rows, D), 1, 3, 1.0, seed + 6) * signs((rows, D), seed + 7)
    dy = torch.where(mir[:, None], dense, X.ints((rows, D), -3, 3, X.density_for(D), seed + 8))
    pre[:, h:] = torch.where(mir[:, None], pre[:, :h], pre[:, h:])
    dy[:, h:] = torch.where(mir[:, None], -dy[:, :h], dy[:, h:])
    x = X.ints((B, d['n_in'], C), -2, 2, X_DENSITY, seed + 9)
    x[:, 0] = X.ints((B, C), 1, 3, 1.0, seed + 10)
    w = X.ints((D, 27), -2, 2, 1.0, seed + 11)

    xh = (pre.double() - mu.double()[:, None]) * rs.double()[:, None]
    gg = dy.double() * gamma.double()
    X.assert_fp32_exact(f'{name} xh', xh)
    L.assert_sums_exact(f'{name} dgamma', dy.double() * xh, 0, 0.25)
    L.assert_sums_exact(f'{name} dbeta', dy, 0, 1.0)
    dgamma, dbeta = (dy.double() * xh).sum(0), dy.double().sum(0)
    gx = gg * xh
    L.assert_sums_exact(f'{name} sum g', gg, 1, 0.5)
    L.assert_sums_exact(f'{name} sum g xh', gx, 1, 0.125)
    s1, s2 = gg.sum(1), gx.sum(1)
    del gx
    assert bool((s1[mir] == 0).all()) and bool((s2[mir] == 0).all()), f'{name}: a mirrored row has a non-zero sum'
    c1, c2 = (s1 / D)[:, None], (s2 / D)[:, None]
    exact_rows = torch.ones(rows, dtype=torch.bool) if pow2 else mir.clone()
    t = xh * c2
    o = rs.double()[:, None] * (gg - c1 - t)
    for nm, v in (('c1', c1), ('c2', c2), ('xh c2', t), ('g - c1', gg - c1), ('rs (...)', o)):
        X.assert_fp32_exact(f'{name} {nm}', v[exact_rows])
    bound = 8 * U * rs.double()[:, None] * (gg.abs() + c1.abs() + t.abs())
    del t
    stored = X.rne_bf16(o).double() if dt == 'bf16' else o.float().double()
    delta = torch.where(exact_rows[:, None], torch.zeros_like(bound), bound + (2 * L.half_bf16_ulp(o) if dt == 'bf16' else 0.0))
    sh3 = (B, d['n_out'], C)
    c = dict(name=name, shape=shape, dt=dt, mode=mode, d=d, pre=pre.reshape(sh3), dy=dy.reshape(sh3), x=x, mu=mu, rs=rs, w=w,
             gamma=gamma, dgamma=dgamma, dbeta=dbeta, dpre=o, exact_rows=exact_rows, mirrored=mir, bound=bound,
             stored=stored.reshape(sh3))
    c['dx'] = conv_T_ref(c['stored'], w, shape)
    c['dw'] = dw_ref(c['stored'], x, shape)
    # exact sums: every term a multiple of dpre's unit, and the sums of magnitudes below 2^24 units
    c['sums_exact'] = False
    if bool(exact_rows.all()):
        q = dyadic_unit(stored)
        dx_mag = 27 * 2 * float(stored.abs().max()) / q
        dw_mag = 2 * float(stored.abs().sum(0).max()) / q
        c['sums_exact'] = dx_mag < X.EXACT_LIMIT and dw_mag < X.EXACT_LIMIT
        c['sum_units'] = (q, dx_mag, dw_mag)
    if c['sums_exact']:
        X.assert_fp32_exact(f'{name} dx', c['dx'])
        X.assert_fp32_exact(f'{name} dw', c['dw'])
    else:
        aw, ax, ast = w.abs(), x.abs(), c['stored'].abs()
        dl = delta.reshape(sh3)
        c['dx_bound'] = conv_T_ref(dl, aw, shape) + 27 * U * conv_T_ref(ast, aw, shape)
        c['dx_bound'][:, 0] = delta.reshape(sh3)[:, 0]              # the cls row is a copy of the stored dpre
        nb, per = w_block_slices(shape)          # a block's chain of per * heads fmas, then at most nb - 1 adds of the partials
        terms = per * heads + nb
        c['dw_bound'] = dw_ref(dl, ax, shape) + terms * U * dw_ref(ast, ax, shape)
    return c


def bwd_expected_dpre(c):
    """The expected stored dpre of the exactly checked rows, in the stored dtype."""
    v = c['dpre'][c['exact_rows']]
    X.assert_fp32_exact(f"{c['name']} dpre", v)
    return X.rne_bf16(v) if c['dt'] == 'bf16' else v.float()


# ------------------------------------------------------------------ literal restatements, with faults
def emu_pre(x, w, shape, fault=None):
    """The forward gather as the header of pool_conv_ln states it: output token (to, ho, wo) sums w[c % hd][(kt*3+kh)*3+kw] *
    x[t, h, w'] over t = to + kt - 1, h = ho sh + kh - 1, w' = wo sw + kw - 1 inside the grid; row 0 of a clip is the cls
    token and is copied.  Faults: 'swap' (sh and sw exchanged in the window origin), 'flip' (tap order reversed), 'far_edge'
    (the window row at h = H - 1 dropped), 'cls_conv' (the cls row also picks up its right-hand neighbour through tap kw = 2)."""
    d = dims(shape)
    B, T, H, W, Ho, Wo, sh, sw, C = (d[k] for k in ('B', 'T', 'H', 'W', 'Ho', 'Wo', 'sh', 'sw', 'C'))
    if fault == 'swap':
        sh, sw = sw, sh
    xd, wc = x.double(), w.double().repeat(d['heads'], 1)                   # wc [C, 27]
    r = torch.arange(T * Ho * Wo)
    to, ho, wo = r // (Ho * Wo), r // Wo % Ho, r % Wo
    out = torch.zeros(B, d['n_out'], C, dtype=torch.float64)
    out[:, 0] = xd[:, 0]
    for kt, kh, kw in itertools.product(range(3), repeat=3):
        t, hh, ww = to + kt - 1, ho * sh + kh - 1, wo * sw + kw - 1
        ok = (t >= 0) & (t < T) & (hh >= 0) & (hh < (H - 1 if fault == 'far_edge' else H)) & (ww >= 0) & (ww < W)
        tap = (kt * 3 + kh) * 3 + kw
        idx = (1 + (t * H + hh) * W + ww).clamp(0, d['n_in'] - 1)
        out[:, 1:] += ok.double()[None, :, None] * xd[:, idx] * wc[:, 26 - tap if fault == 'flip' else tap]
    if fault == 'cls_conv':
        out[:, 0] += xd[:, 1] * wc[:, 14]
    return out


def emu_dx(dpre, w, shape, fault=None):
    """The backward-data gather: input token (t, h, w') collects w[c % hd][tap] * dpre[to, hq, wq] over the taps with
    to = t - kt + 1 in range, h - kh + 1 = hq sh, hq < Ho and w' - kw + 1 = wq sw, wq < Wo.  Fault 'head_offset': the
    [tap][channel] weight table read at tap * hd + c instead of tap * hd + c % hd (head k reads tap + k; past the table: 0)."""
    d = dims(shape)
    B, T, H, W, Ho, Wo, sh, sw, C, hd = (d[k] for k in ('B', 'T', 'H', 'W', 'Ho', 'Wo', 'sh', 'sw', 'C', 'hd'))
    if fault == 'swap':
        sh, sw = sw, sh
    dd = dpre.double()
    flat = torch.cat([w.double().t().reshape(-1), torch.zeros(C)])          # [tap][channel], zeros behind
    ch = torch.arange(C)
    r = torch.arange(T * H * W)
    t, hh, ww = r // (H * W), r // W % H, r % W
    out = torch.zeros(B, d['n_in'], C, dtype=torch.float64)
    out[:, 0] = dd[:, 0]
    for kt, kh, kw in itertools.product(range(3), repeat=3):
        to, hn, wn = t - kt + 1, hh - kh + 1, ww - kw + 1
        hq, wq = hn // sh, wn // sw
        ok = (to >= 0) & (to < T) & (hn >= 0) & (hq * sh == hn) & (hq < Ho) & (wn >= 0) & (wq * sw == wn) & (wq < Wo)
        tap = (kt * 3 + kh) * 3 + kw
        idx = (1 + (to * Ho + hq) * Wo + wq).clamp(0, d['n_out'] - 1)
        wt = flat[tap * hd + (ch if fault == 'head_offset' else ch % hd)]
        out[:, 1:] += ok.double()[None, :, None] * dd[:, idx] * wt
    return out


def w_block_slices(shape):
    """(blocks, pairs per block) of the weight-gradient launch: cdiv(pairs, 32) blocks capped at W_BLOCKS."""
    pairs = dims(shape)['pairs']
    nb = min(max((pairs + 31) // 32, 1), W_BLOCKS)
    return nb, (pairs + nb - 1) // nb


def pair_weight_without_second_batch(shape):
    """1 for the pairs of the first PB of their block's slice, 0 for the later batches."""
    pairs = dims(shape)['pairs']
    _, per = w_block_slices(shape)
    return ((torch.arange(pairs) % per) < PB).double()


def empty_w_blocks(shape):
    nb, per = w_block_slices(shape)
    return sum(1 for b in range(nb) if b * per >= dims(shape)['pairs'])


# ------------------------------------------------------------------------------------- position encoding
POS_B, POS_T, POS_HW = 2, 3, 35


def pos_case(C, kind):
    """Integer operands of PosEncodingFn: x [B, T*HW, C], cls / pos_class [1, 1, C], spatial [1, HW, C], temporal [1, T, C], dy
    [B, 1 + T*HW, C].  'round': the spatial table and pos_class sit near 512 (bf16 spacing 4).  The kernel adds spatial +
    temporal first and x last; with integers below 2^24 every grouping is exact, so the order is not observable here."""
    off = 512.0 if kind == 'round' else 0.0
    s = 1000 + C
    return dict(x=X.ints((POS_B, POS_T * POS_HW, C), -16, 16, 1.0, s), cls=X.ints((1, 1, C), -32, 32, 1.0, s + 1),
                pos_class=X.ints((1, 1, C), -32, 32, 1.0, s + 2) + off, spatial=X.ints((1, POS_HW, C), -32, 32, 1.0, s + 3) + off,
                temporal=X.ints((1, POS_T, C), -32, 32, 1.0, s + 4), dy=X.ints((POS_B, 1 + POS_T * POS_HW, C), -16, 16, 1.0, s + 5))


def pos_reference(c):
    """(out, dx, d_cls, d_pos_class, d_spatial, d_temporal) in float64 by autograd of the oracle module."""
    from oracle import mvit_oracle as MO
    C = c['x'].shape[-1]
    enc = MO.SpatioTemporalClsPositionalEncoding(C, [POS_T, 5, 7]).double()
    with torch.no_grad():
        enc.cls_token.copy_(c['cls']); enc.pos_embed_class.copy_(c['pos_class'])
        enc.pos_embed_spatial.copy_(c['spatial']); enc.pos_embed_temporal.copy_(c['temporal'])
    xr = c['x'].double().requires_grad_(True)
    out = enc(xr)
    out.backward(c['dy'].double())
    res = (out.detach(), xr.grad, enc.cls_token.grad, enc.pos_embed_class.grad, enc.pos_embed_spatial.grad, enc.pos_embed_temporal.grad)
    for v in res:
        X.assert_fp32_exact('pos_encoding', v)
    return res


# ------------------------------------------------------------------------------------------- stem gather
# (kernel, stride, padding, Cc, clip [B, T, Cc, H, W], Kp)
IM2COL_GEOMS = (((3, 7, 7), (2, 4, 4), (1, 3, 3), 3, (2, 5, 3, 18, 25), 448),      # the stem's own: K = 441 ends inside the last 8-column group
                ((2, 3, 5), (1, 2, 3), (0, 1, 2), 2, (2, 4, 2, 9, 11), 64),        # every axis different; K = 60 -> 64
                ((2, 3, 5), (1, 2, 3), (0, 1, 2), 2, (2, 4, 2, 9, 11), 128))       # and a row of 8 whole zero groups


def im2col_ref(clip, geom):
    """rows [M, Kp] float32: pad + unfold, columns ordered (c, kt, kh, kw), zero columns K .. Kp - 1.  Pure copies: bit patterns kept."""
    k3, s3, p3, Cc, _, Kp = geom
    v = TF.pad(clip.permute(0, 2, 1, 3, 4), (p3[2], p3[2], p3[1], p3[1], p3[0], p3[0]))
    v = v.unfold(2, k3[0], s3[0]).unfold(3, k3[1], s3[1]).unfold(4, k3[2], s3[2])           # [B, Cc, To, Ho, Wo, KT, KH, KW]
    B, _, To, Ho, Wo = v.shape[:5]
    rows = v.permute(0, 2, 3, 4, 1, 5, 6, 7).reshape(B * To * Ho * Wo, Cc * k3[0] * k3[1] * k3[2])
    return TF.pad(rows, (0, Kp - rows.shape[1]))


def emu_im2col(clip, geom, fault=None):
    """The gather as im2col3d's header states it: row (b, to, ho, wo), column k -> (c, kt, kh, kw) by carrying kw -> kh -> kt
    -> c from the first column of each group of 8.  Fault 'kh_carry': the carry out of kh is skipped (kt, c never advance
    within a group)."""
    k3, s3, p3, Cc, _, Kp = geom
    B, Tc, _, H, W = clip.shape
    To, Ho, Wo = ((n + 2 * p - k) // s + 1 for n, p, k, s in zip((Tc, H, W), p3, k3, s3))
    K = Cc * k3[0] * k3[1] * k3[2]
    cols = []
    for k0 in range(0, Kp, 8):
        kw, kh, kt, c = k0 % k3[2], k0 // k3[2] % k3[1], k0 // (k3[2] * k3[1]) % k3[0], k0 // (k3[2] * k3[1] * k3[0])
        for j in range(8):
            cols.append((c, kt, kh, kw, k0 + j < K))
            kw += 1
            if kw == k3[2]:
                kw, kh = 0, kh + 1
                if kh == k3[1]:
                    kh = 0
                    if fault != 'kh_carry':
                        kt += 1
                        if kt == k3[0]:
                            kt, c = 0, c + 1
    m = torch.arange(B * To * Ho * Wo)
    b, to, ho, wo = m // (To * Ho * Wo), m // (Ho * Wo) % To, m // Wo % Ho, m % Wo
    out = torch.zeros(len(m), Kp)
    for k, (c, kt, kh, kw, live) in enumerate(cols):
        t, h, w = to * s3[0] - p3[0] + kt, ho * s3[1] - p3[1] + kh, wo * s3[2] - p3[2] + kw
        ok = (t >= 0) & (t < Tc) & (h >= 0) & (h < H) & (w >= 0) & (w < W) & live & (c < Cc)
        val = clip[b, t.clamp(0, Tc - 1), min(c, Cc - 1), h.clamp(0, H - 1), w.clamp(0, W - 1)]
        out[:, k] = torch.where(ok, val, torch.zeros(()))
    return out


def stem_case():
    """ConvStemFn end to end with integers: clip [2, 5, 3, 18, 25] in [-1, 1] and weights [96, 3, 3, 7, 7] in [-2, 2], both
    sparse (density_for(441)), integer bias and dy; out, d_w and d_b are exact integer sums."""
    p = X.density_for(441)
    clip = X.ints((2, 5, 3, 18, 25), -1, 1, p, 31)
    w = X.ints((96, 3, 3, 7, 7), -2, 2, p, 32)
    b = X.ints((96,), -16, 16, 1.0, 33)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    out = TF.conv3d(clip.double().transpose(1, 2), wr, br, stride=(2, 4, 4), padding=(1, 3, 3)).flatten(2).transpose(1, 2)
    dy = X.ints(tuple(out.shape), -2, 2, 0.5, 34)
    out.backward(dy.double())
    for v in (out.detach(), wr.grad, br.grad):
        X.assert_fp32_exact('conv stem', v)
    assert float(out.detach().abs().max()) <= 256
    return dict(clip=clip, w=w, b=b, dy=dy, out=out.detach(), d_w=wr.grad, d_b=br.grad)


# ---------------------------------------------------------------------------------------------- max pool
MAXPOOL_GRIDS = ((3, 7, 9), (2, 1, 9), (1, 6, 1))
MAXPOOL_C = 40


def maxpool_case(thw, seed=0):
    """x [2, 1 + T*H*W, 40] of few distinct integers (so most windows repeat their maximum), with whole -inf patches (border
    windows whose in-range taps are all -inf) and scattered NaNs; dy integers."""
    T, H, W = thw
    g = X.gen(seed + 13 * H + W)
    B, C = 2, MAXPOOL_C
    v = torch.randint(-2, 3, (B, T, H, W, C), generator=g).float()
    ninf = torch.rand(B, T, 1, 1, C, generator=g) < 0.15                 # a whole frame of a channel
    v = torch.where(ninf.expand_as(v), torch.full_like(v, float('-inf')), v)
    patch = torch.rand(B, T, (H + 2) // 3, (W + 2) // 3, C, generator=g) < 0.2
    patch = patch.repeat_interleave(3, 2).repeat_interleave(3, 3)[:, :, :H, :W]
    v = torch.where(patch, torch.full_like(v, float('-inf')), v)
    v = torch.where(torch.rand(v.shape, generator=g) < 0.03, torch.full_like(v, float('nan')), v)
    x = torch.cat([X.ints((B, 1, C), -8, 8, 1.0, seed + 1), v.reshape(B, T * H * W, C)], 1)
    Ho, Wo = pooled(H, 2), pooled(W, 2)
    dy = X.ints((B, 1 + T * Ho * Wo, C), 1, 16, 1.0, seed + 2)
    return x, dy


def maxpool_ref(x, dy, thw, last=False):
    """(y, dx) float64.  last=False: torch.nn.MaxPool3d on the CPU (through the oracle's attention_pool) and its autograd.
    last=True: a literal (kh, kw) scan in which a later equal value replaces the maximum (the fault)."""
    if not last:
        from oracle import mvit_oracle as MO
        xr = x.double().requires_grad_(True)
        y, _ = MO.attention_pool(xr, torch.nn.MaxPool3d([1, 3, 3], [1, 2, 2], [0, 1, 1]), list(thw))
        y.backward(dy.double())
        return y.detach(), xr.grad
    T, H, W = thw
    B, _, C = x.shape
    Ho, Wo = pooled(H, 2), pooled(W, 2)
    g = x[:, 1:].double().reshape(B, T, H, W, C)
    best = torch.full((B, T, Ho, Wo, C), float('-inf'), dtype=torch.float64)
    arg = torch.full((B, T, Ho, Wo, C), -1, dtype=torch.long)
    ho, wo = torch.arange(Ho), torch.arange(Wo)
    for kh, kw in itertools.product(range(3), repeat=2):
        hh, ww = ho * 2 + kh - 1, wo * 2 + kw - 1
        ok = ((hh >= 0) & (hh < H))[:, None] & ((ww >= 0) & (ww < W))[None, :]
        val = g[:, :, hh.clamp(0, H - 1)][:, :, :, ww.clamp(0, W - 1)]
        take = ok[None, None, :, :, None] & ((val >= best) | torch.isnan(val) | (arg < 0))
        best, arg = torch.where(take, val, best), torch.where(take, torch.full_like(arg, kh * 3 + kw), arg)
    dx = torch.zeros(B, T, H, W, C, dtype=torch.float64)
    dyg = dy[:, 1:].double().reshape(B, T, Ho, Wo, C)
    for kh, kw in itertools.product(range(3), repeat=2):
        for i, j in itertools.product(range(Ho), range(Wo)):
            hh, ww = 2 * i + kh - 1, 2 * j + kw - 1
            if 0 <= hh < H and 0 <= ww < W:
                dx[:, :, hh, ww] += dyg[:, :, i, j] * (arg[:, :, i, j] == kh * 3 + kw)
    y = torch.cat([x[:, :1].double(), best.reshape(B, T * Ho * Wo, C)], 1)
    return y, torch.cat([dy[:, :1].double(), dx.reshape(B, T * H * W, C)], 1)
