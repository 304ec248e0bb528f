"""Exact tests of what runs either side of the backbone in a training step (imported by test modules; not a conftest):
csrc/head.hip (Mixup, CutMix, soft targets, softmax cross-entropy, top-k), the MaskFeat half of csrc/hog.hip (mask-token
blend, masked MSE) and csrc/optim.hip (chunk norms, norm of norms, clipped SGD / AdamW).

Three kinds of expected value, in the order of preference:
  equality   inputs chosen so that every fp32 operation of the kernel is exact (integers, dyadic values, powers of two), or so
             that the one inexact operation is a single correctly rounded IEEE division / sqrt / subtraction whose float32
             replay on the CPU is THE answer.  The builders assert the premise (exact.assert_fp32_exact on every intermediate).
  bound      a per-element bound against float64 in units of 2^-24 of the quantity's own scale; the number of roundings is
             derived in the docstring of the bound and k, the allowance for the transcendental functions, is the one measured
             number: K_* is what the fp32 CPU transcription needs, asserted in test_exact_step_premise.py, the GPU bar is twice
             that for the device's 1-ulp expf / logf (or its fma contraction, for the optimizer).
  select     kernels that only move values (CutMix, the blend) are bit-exact for any input.

Softmax cross-entropy bound (xent_bounds).  u = 2^-24, d = lse - x >= 0 (minus the log-probability), p = exp(-d),
ts = sum_c t, n = ceil(C / 64) + 6 the additions of a lane loop and the wave butterfly:
  d      |d32 - d| <= k u (1 + d): the max-first form (mx - x) + log(se) rounds the difference at the scale of the SPREAD of the
         row (<= u d each for the subtraction and the sum), and log(se) in [0, log C] carries its own ulp and that of se;
  row    labels: the same, the row loss IS d[label].  Soft targets: sum_c t d with one rounding per product and n roundings of
         the running sum, all terms >= 0:  u (k (ts + row) + (1 + n) row);
  mean   the sum of the row bounds, ceil(B / 256) + 8 additions of the block reduction and one division, over the count;
  p      |p32 - p| <= k u (1 + d) p: the argument of exp carries an absolute error of the size of d's, exp turns it into a
         relative one and adds its own ulp;
  dx     g (p ts - t): g is one division, p ts one product of an n-addition sum, then one subtraction and one product:
         |g| u (p ts (k (1 + d) + n + 1) + 3 |p ts - t|) + |g| ts 2^-126 (a flushed or subnormal exponential).
A common offset of the row moves none of these: that is the property the offset cases hold (the form lse = mx + log(se),
lse - x rounds at the magnitude of the logits instead and misses the bound by orders of magnitude at offset 4096).
Measured over XENT_ACCURACY (test_exact_step_premise.py writes the figures to the parity report): the max-first float32
transcription needs k = 4.42 on d and k = 4.53 on p, hence K_REF = 8.

Optimizer bound (opt_bounds), one step from given state, u = 2^-24:
  |p - p64| <= u (|p64| + K dP),   |m - m64| <= u K dM,   |v - v64| <= u K v64
with the scales taken gross of cancellation: SGD dM = |c g| + |wd p| + mom |m0|, dP = lr dM (1 + mom with nesterov);
AdamW dM = b1 |m0| + (1 - b1) |c g|, dP = lr wd |p| + (lr / bc1) dM / denom.  The reference of a step is float64 arithmetic on
the float32 hyper-parameters and the float32 state the step started from.  K is measured per parameter group (K_OPT, asserted
in test_exact_step_premise.py over four general steps of the float32 CPU transcription): SGD needs 2.44 without and 3.21 with
weight decay (K = 4, 4); AdamW needs 5.22 without decay (K = 8).  With decay AdamW rounds p four times at the scale of p itself
(lr wd, 1 - lr wd, the multiply, the final subtraction) where the form above allows one: the others are charged to K dP with
dP >= lr wd |p| = 5e-4 |p|, and the transcription needs 1849 (K = 2048).  That bound still holds every element to a few ulp of
its own magnitude, which max|a - b| / max|b| does not.
"""
import math

import numpy as np
import torch

import exact as X
from helpers import report

U24 = 2.0 ** -24
FLUSH = 2.0 ** -126
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
GUARD = 64                                   # elements of sentinel either side of a flat buffer (keeps 16-byte alignment)

K_REF = 8                                    # cross-entropy: what the max-first fp32 transcription stays within (4.42 / 4.53)
K_GPU = 2 * K_REF
K_OPT = {'sgd': (4, 4), 'adamw': (8, 2048)}  # optimizer, (no-decay group, decayed group): the fp32 transcription of a step


def flat_guarded(n, device, dtype=F32, guard=GUARD):
    """Sentinel-filled flat buffer of guard + n + guard elements -> (buffer, the n-element body, {label: guard view})."""
    buf = X.sentinel_fill(torch.empty(n + 2 * guard, dtype=dtype, device=device))
    return buf, buf[guard:guard + n], {'before': buf[:guard], 'after': buf[guard + n:]}


def k_needed(err, fixed, per_k):
    """Smallest k with err <= fixed + k * per_k everywhere (0 where per_k is 0 and err within fixed; inf where it is not)."""
    over = (err - fixed).clamp_min(0.0)
    k = torch.where(per_k > 0, over / per_k.clamp_min(1e-300), torch.where(over > 0, torch.full_like(over, math.inf), over))
    return float(k.max()) if k.numel() else 0.0


# ===================================================================================== softmax cross-entropy
XENT_SHAPES = ((1, 1), (3, 2), (4, 63), (5, 64), (5, 65), (7, 174), (257, 400), (1030, 1000), (13, 7))
XENT_IGNORED = (-100, None, -1)              # None stands for C
GLOSS = 0.5                                  # upstream gradient of the loss: a power of two
XENT_STRUCTURE_MODES = ('labels', 'all_ignored', 'soft')
XENT_ACCURACY = tuple((s, off, tgt) for s in (3, 30) for off in (0, -64, 64, 4096) for tgt in ('labels', 'soft', 'smoothed'))


def argmax_columns(B, C, seed):
    """Arg-max column of every row, cycling through the last column, lane 63's tail element (the last column that lane 63
    reads), column 64, column 0 and a random one."""
    special = [C - 1]
    if C >= 64:
        special.append(63 + 64 * ((C - 64) // 64))
    if C > 64:
        special.append(64)
    special.append(0)
    rnd = torch.randint(0, C, (B,), generator=X.gen(seed))
    n = len(special) + 1
    return torch.tensor([special[b % n] if b % n < len(special) else int(rnd[b]) for b in range(B)])


def xent_structure_case(B, C, mode, seed=0):
    """Integer logits with one entry m_b per row and every other at least 200 below: expf of the difference is exactly 0, se
    = 1, log(se) = 0, lse = m_b, every row loss an integer (labels) or a multiple of 1/8 (soft targets k/8, rows that sum to 1
    and rows that do not), the mean ONE rounded division, dx = g (onehot(argmax) ts - t) with g = 0.5 / count ONE rounded
    division and one rounded product (exact when the count is a power of two)."""
    g = X.gen(seed)
    m = torch.randint(-50, 51, (B,), generator=g).double()
    am = argmax_columns(B, C, seed + 1)
    x = m[:, None] - 200.0 - torch.randint(0, 101, (B, C), generator=g).double()
    x[torch.arange(B), am] = m
    X.assert_fp32_exact('xent structure logits', x)
    d = m[:, None] - x
    hot = torch.zeros(B, C, dtype=F64)
    hot[torch.arange(B), am] = 1.0
    c = dict(B=B, C=C, mode=mode, x=x.float(), lse=m.float(), argmax=am, name=f'xent structure {mode} {B}x{C}')
    if mode == 'soft':
        t = X.ints((B, C), 0, 8, min(0.3, 6000.0 / (B * C)), seed + 2).double() / 8.0     # sparse: the sum over the batch stays exact
        for b in range(0, B, 3):                                  # rows that sum to exactly 1
            t[b] = 0.0
            cols = torch.randperm(C, generator=g)[:3]
            t[b, cols] = torch.tensor([0.5, 0.25, 0.25], dtype=F64)[:len(cols)] if C >= 3 else 1.0 / len(cols)
        if B > 1:
            assert bool((t.sum(1) != 1.0).any()), 'some soft rows must not sum to 1'
        rows = (t * d).sum(1)
        ts = t.sum(1, keepdim=True)
        count = B
        valid = torch.ones(B, dtype=torch.bool)
        c['target'] = t.float()
    else:
        lab = torch.randint(0, C, (B,), generator=g)
        lab[1::4] = am[1::4]                                      # the label is the arg-max: loss 0
        ign = torch.tensor([C if v is None else v for v in XENT_IGNORED])
        if mode == 'all_ignored':
            lab = ign[torch.arange(B) % 3]
        elif B >= 3:
            lab[2::5] = ign[(torch.arange(B)[2::5] // 5) % 3]
        valid = (lab >= 0) & (lab < C)
        t = torch.zeros(B, C, dtype=F64)
        t[valid, lab[valid]] = 1.0
        rows = (t * d).sum(1)
        ts = torch.ones(B, 1, dtype=F64)
        count = int(valid.sum())
        c['target'] = lab
    assert float(rows.sum()) * 8 < X.EXACT_LIMIT, 'every partial sum of the rows and of their sum is fp32-exact'
    X.assert_fp32_exact('xent structure rows', rows * 8)
    v = hot * ts - t
    X.assert_fp32_exact('xent structure onehot ts - t', v * 8)
    g32 = torch.tensor(GLOSS, dtype=F32) / torch.tensor(float(count), dtype=F32)     # the kernel's g /= count
    dx = g32 * v.float()
    dx[~valid] = 0.0
    c.update(rows=rows.float(), count=count, valid=valid, dx=dx, pow2_count=count > 0 and count & (count - 1) == 0,
             mean=rows.sum().float() / torch.tensor(float(count), dtype=F32))
    return c


def xent_accuracy_case(B, C, s, offset, target, seed=0):
    """Dyadic random logits round(s N(0,1) 64) / 64 plus a common offset (fp32-exact, asserted); targets: labels, normalised
    random soft targets, or label-smoothed one-hot rows mixed with the flipped batch's (smoothing 0.1, lam 0.37)."""
    g = X.gen(seed)
    x = torch.round(s * torch.randn(B, C, generator=g, dtype=F64) * 64.0) / 64.0 + offset
    X.assert_fp32_exact('xent accuracy logits', x)
    lab = torch.randint(0, C, (B,), generator=g)
    if target == 'labels':
        t = lab
    elif target == 'soft':
        t = torch.rand(B, C, generator=g)
        t = t / t.sum(-1, keepdim=True)
    else:
        off = 0.1 / C
        oh = lambda l: torch.full((B, C), off).scatter_(1, l.view(-1, 1), 1. - 0.1 + off)   # noqa: E731
        t = oh(lab) * 0.37 + oh(lab.flip(0)) * (1. - 0.37)
    return dict(B=B, C=C, x=x.float(), target=t, name=f'xent accuracy {target} {B}x{C} s={s} offset={offset}')


def xent_f64(x, target, gloss=GLOSS):
    """float64 reference: d = lse - x, p = softmax, row losses, their mean over the counted rows, dx (and t, ts, g)."""
    B, C = x.shape
    x64 = x.double()
    mx = x64.max(1, keepdim=True).values
    lse = mx + torch.log(torch.exp(x64 - mx).sum(1, keepdim=True))
    d = lse - x64
    p = torch.exp(-d)
    if target.is_floating_point():
        t = target.double()
        valid = torch.ones(B, dtype=torch.bool)
        ts = t.sum(1, keepdim=True)
    else:
        valid = (target >= 0) & (target < C)
        t = torch.zeros(B, C, dtype=F64)
        t[valid, target[valid]] = 1.0
        ts = torch.ones(B, 1, dtype=F64)
    rows = (t * d).sum(1)
    count = int(valid.sum())
    g = gloss / count if count else math.inf
    dx = g * (p * ts - t) if count else torch.zeros(B, C, dtype=F64)
    dx[~valid] = 0.0
    return dict(B=B, C=C, d=d, p=p, t=t, ts=ts, rows=rows, count=count, valid=valid, g=g, dx=dx, lse=lse[:, 0],
                mean=rows.sum() / count if count else torch.tensor(math.nan, dtype=F64), soft=target.is_floating_point())


def xent_bounds(r, k):
    """Per-element bounds of the row losses, their mean and dx for the reference r (xent_f64); derivation: module docstring."""
    B, C = r['B'], r['C']
    n = (-(-C // 64) + 6) if r['soft'] else 0
    ts1 = r['ts'][:, 0]
    rows_fixed = U24 * (1 + n) * r['rows'] if r['soft'] else torch.zeros(B, dtype=F64)
    rows_k = U24 * (ts1 + r['rows']) * r['valid']
    rows_b = rows_fixed + k * rows_k
    cnt = max(r['count'], 1)
    mean_fixed = (rows_fixed.sum() + U24 * (-(-B // 256) + 9) * r['rows'].abs().sum()) / cnt
    mean_k = rows_k.sum() / cnt
    g = abs(r['g']) if r['count'] else 0.0
    pts = r['p'] * r['ts']
    dx_fixed = g * (U24 * (pts * (n + 1) + 3 * (pts - r['t']).abs()) + r['ts'] * FLUSH) * r['valid'][:, None]
    dx_k = g * U24 * pts * (1 + r['d']) * r['valid'][:, None]
    return dict(rows=(rows_fixed, rows_k), mean=(mean_fixed.reshape(1), mean_k.reshape(1)), dx=(dx_fixed, dx_k))


def xent_check(name, got, r, k, quiet=False):
    """got: dict(rows [B], mean scalar, dx [B,C]) as CPU float32.  Every element within xent_bounds(r, k); returns the k each
    output needs and writes one parity-report line."""
    b = xent_bounds(r, k)
    need, bad = {}, []
    for key in ('rows', 'mean', 'dx'):
        ref = r[key].reshape(-1) if key == 'mean' else r[key]
        err = (got[key].double().reshape(ref.shape) - ref).abs()
        fixed, per_k = b[key]
        if key == 'mean' and not r['count']:
            ok = bool(torch.isnan(got[key]).all())                # 0 / 0
            need[key] = 0.0
        else:
            err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
            need[key] = k_needed(err, fixed, per_k)
            ok = bool((err <= fixed + k * per_k).all())
        if not ok:
            bad.append(f'{key} needs k = {need[key]:.3g}')
    line = ', '.join(f'{key} k={v:.2f}' for key, v in need.items())
    if not quiet:
        report(f'{"FAIL" if bad else "ok  "} bound {name}: {line} (bar k = {k})')
    assert not bad or quiet, f'{name}: beyond the bound at k = {k}: ' + '; '.join(bad)
    return need, not bad


def lane_sum32(v):
    """[B, C] float32 -> [B]: lane c % 64 adds its columns in order, then the xor butterfly of wave_sum."""
    B, C = v.shape
    n = -(-C // 64)
    pad = torch.zeros(B, n * 64)
    pad[:, :C] = v
    acc = torch.zeros(B, 64)
    for i in range(n):
        acc = acc + pad[:, i * 64:(i + 1) * 64]
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def block_sum32(v, valid=None):
    """mean_rows_kernel's sum of v [B]: thread i % 256 adds its rows in order, then the halving tree over 256 threads."""
    B = v.numel()
    n = -(-B // 256)
    pad = torch.zeros(n * 256)
    pad[:B] = v
    acc = torch.zeros(256)
    for i in range(n):
        acc = acc + pad[i * 256:(i + 1) * 256]
    s = 128
    while s:
        acc = acc[:s] + acc[s:2 * s]
        s >>= 1
    return acc[0]


def xent_terms32(x, form):
    """d = lse - x and p = softmax in float32, as 'max_first' ((mx - x) + log se, exp((x - mx) - log se)) or as the 'kernel'
    form before the fix (lse = mx + log se; lse - x; exp(x - lse))."""
    mx = x.max(1, keepdim=True).values
    lg = torch.log(lane_sum32(torch.exp(x - mx)))[:, None]
    if form == 'max_first':
        return (mx - x) + lg, torch.exp((x - mx) - lg), (mx + lg)[:, 0]
    lse = mx + lg
    return lse - x, torch.exp(x - lse), lse[:, 0]


def xent_replay32(x, target, form='max_first', gloss=GLOSS, rows_limit=None, skip_tail=False):
    """The kernels' arithmetic in float32 on the CPU -> dict(rows, lse, mean, dx).  Faults for the premise tests:
    rows_limit = R leaves rows >= R out of the mean; skip_tail drops the last column a lane reads beyond its first."""
    B, C = x.shape
    d, p, lse = xent_terms32(x, form)
    keep = torch.ones(C)
    if skip_tail and C > 64:
        keep[64 * ((C - 1) // 64):] = 0.0
    if target.is_floating_point():
        t = target.float()
        rows = lane_sum32(t * d * keep)
        ts = lane_sum32(t * keep)[:, None]
        valid = torch.ones(B, dtype=torch.bool)
    else:
        valid = (target >= 0) & (target < C)
        t = torch.zeros(B, C)
        t[valid, target[valid]] = 1.0
        rows = (t * d).sum(1)                                     # one non-zero term
        ts = torch.ones(B, 1)
    counted = valid if rows_limit is None else valid & (torch.arange(B) < rows_limit)
    count = torch.tensor(float(counted.sum()))
    mean = block_sum32(rows * counted) / count
    g = torch.tensor(gloss) / torch.tensor(float(valid.sum()))
    dx = g * (p * ts - t)
    dx[~valid] = 0.0
    return dict(rows=rows, lse=lse, mean=mean, dx=dx)


# ======================================================================================================= top-k
def topk_ref(scores, labels, k, smaller_index_first=True):
    """Rows whose label is among the k largest: entries strictly greater count first, then equal entries at a smaller index
    (smaller_index_first=False: the opposite tie rule, a fault for the premise test).  Labels outside [0, C): never."""
    B, C = scores.shape
    valid = (labels >= 0) & (labels < C)
    lab = labels.clamp(0, C - 1)
    v = scores[torch.arange(B), lab][:, None]
    idx = torch.arange(C)[None, :]
    side = idx < lab[:, None] if smaller_index_first else idx > lab[:, None]
    ahead = (scores > v).sum(1) + ((scores == v) & side).sum(1)
    return int((valid & (ahead < k)).sum())


def topk_ks(C):
    return sorted({1, 5, C, C + 3})


def topk_tie_case(B, C, k, seed=0):
    """Scores from max(2, C // 2) integer levels (ties everywhere), one +inf and one -inf entry in every third row; half of the
    labels sit among the first k + 2 places of the row in the stated order, where a tie decides; the first rows are all-equal
    with the label at index k - 1 (the k-th place: correct) and k (one beyond: not), so the label is tied on both sides; some
    labels are ignored."""
    g = X.gen(seed)
    s = torch.randint(0, max(2, C // 2), (B, C), generator=g).float()
    for r in range(0, B, 3):
        s[r, torch.randint(0, C, (1,), generator=g)] = math.inf
        s[r, torch.randint(0, C, (1,), generator=g)] = -math.inf
    lab = torch.randint(0, C, (B,), generator=g)
    order = torch.sort(s, dim=1, descending=True, stable=True).indices
    place = torch.randint(0, min(C, k + 2), (B,), generator=g)
    near = torch.arange(B) % 2 == 0
    lab[near] = order[torch.arange(B), place][near]
    for r, at in ((0, k - 1), (1, k), (2, 0)):
        if r < B:
            s[r] = 1.0
            lab[r] = min(at, C - 1)
    if B > 4:
        lab[4::7] = torch.tensor([-100, C, -1])[(torch.arange(B)[4::7] // 7) % 3]
    return s, lab


def topk_free_case(B, C, seed=0):
    """Tie-free scores (a random permutation of 0 .. C-1 per row, scaled) and labels: torch.topk is then a reference."""
    g = X.gen(seed)
    s = torch.stack([torch.randperm(C, generator=g) for _ in range(B)]).float() * 0.25 - 3.0
    return s, torch.randint(0, C, (B,), generator=g)


# =================================================================================================== optimizer
MT_SIZES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 4095, 4096, 4097, 8192, 12292, 3 * 4096 + 1)
MT_CHUNK = 4096
MT_GROUPS = ((2.0 ** -4, 0.0), (2.0 ** -3, 0.5))          # (lr, wd) of the exact cases: no-decay and decayed group
MT_GROUPS_ADAMW = ((2.0 ** -4, 0.0), (2.0 ** -4, 0.25))
MT_GROUPS_GENERAL = {'sgd': ((0.05, 0.0), (0.05, 0.05)), 'adamw': ((0.01, 0.0), (0.01, 0.05))}


class MtLayout:
    """About 300 tensors in four flat buffers (p, g, s1, s2): sizes MT_SIZES twenty times over with one zero-length tensor in
    the middle; a third of the tensors have ONE of their four pointers 1, 2 or 3 floats off 16-byte alignment; at least 8
    sentinel floats between neighbours and GUARD at the ends.  pos[t][j]: offset of tensor t in buffer j."""

    def __init__(self, cycles=20, seed=7):
        sizes = list(MT_SIZES) * cycles
        sizes.insert(len(sizes) // 2, 0)
        self.sizes = sizes
        self.n = n = len(sizes)
        rng = np.random.RandomState(seed)
        mis, which, by = rng.rand(n) < 1 / 3, rng.randint(0, 4, n), rng.randint(1, 4, n)
        self.off = np.zeros((n, 4), dtype=np.int64)
        self.off[mis, which[mis]] = by[mis]
        self.group = [t % 2 for t in range(n)]
        self.pos = np.zeros((n, 4), dtype=np.int64)
        self.total = []
        for j in range(4):
            cur = GUARD
            for t in range(n):
                self.pos[t, j] = (cur + 3) // 4 * 4 + self.off[t, j]
                cur = self.pos[t, j] + sizes[t] + 8
            self.total.append(int((cur + 3) // 4 * 4 + GUARD))
        self.numel = sum(sizes)
        self.tid = torch.repeat_interleave(torch.arange(n), torch.tensor(sizes))            # tensor of every packed element
        self.index = [torch.cat([torch.arange(self.pos[t, j], self.pos[t, j] + sizes[t]) for t in range(n)]) for j in range(4)]
        self.chunks = [-(-s // MT_CHUNK) for s in sizes]

    def flat(self, j, packed):
        """Sentinel-filled flat CPU buffer j with the packed values in place."""
        buf = X.sentinel_fill(torch.empty(self.total[j], dtype=F32))
        buf[self.index[j]] = packed.float()
        return buf

    def packed(self, j, flat):
        return flat.cpu()[self.index[j]]

    def per_element(self, per_tensor):
        return torch.as_tensor(per_tensor, dtype=F64)[self.tid]

    def hyper(self, groups):
        """(lr, wd) per packed element, as the float32 values the table holds."""
        lr = torch.tensor([groups[g][0] for g in self.group], dtype=F32).double()
        wd = torch.tensor([groups[g][1] for g in self.group], dtype=F32).double()
        return lr[self.tid], wd[self.tid]

    def scalar_forced_by(self):
        """For each of the four pointers: the tensors with a full chunk whose scalar path is forced by that pointer alone."""
        return [[t for t in range(self.n) if self.sizes[t] >= MT_CHUNK and self.off[t, j] and not np.delete(self.off[t], j).any()]
                for j in range(4)]


def mt_params(lay, seed=1):
    return X.ints((lay.numel,), -8, 8, 1.0, seed).double()


def mt_grads(lay, kind, seed=2):
    """Packed gradients.  'ints': integers in [-8, 8], dense in the small tensors and 1 in 4 non-zero in the large ones (the
    total sum of squares stays below 2^24).  'clip': designed norms for clip = 1: 64 (coef = 2^-6: 64 + 1e-6f == 64), 32
    (coef = 2^-5), 0.25 or 0.5 (coef >= 1: untouched) and 0, cycling over the tensors."""
    g = X.gen(seed)
    out = []
    for t, n in enumerate(lay.sizes):
        if kind == 'ints':
            out.append(X.ints((n,), -8, 8, 1.0 if n <= 9 else 0.25, seed + 3 * t + 1).double())
            continue
        v = torch.zeros(n, dtype=F64)
        sign = lambda k: (torch.randint(0, 2, (k,), generator=g) * 2 - 1).double()    # noqa: E731
        what = t % 4
        if n and what in (0, 1):
            norm, cnt = (64.0, 64) if what == 0 else (32.0, 16)
            if n >= cnt:
                at = torch.linspace(0, n - 1, cnt).round().long()
                assert at.unique().numel() == cnt
                v[at] = 8.0 * sign(cnt)
            else:
                v[n - 1] = norm * sign(1)
        elif n and what == 2:
            v[(t // 4) % n] = (0.25 if t % 8 == 2 else 0.5) * sign(1)
        out.append(v)
    return torch.cat(out)


def mt_norms_expected(lay, g):
    """float32(sqrt(sum of squares)) per tensor and over the total, with the premise that every partial sum is exact."""
    sq = torch.zeros(lay.n, dtype=F64).index_add_(0, lay.tid, g * g)
    unit = 1 if bool((g == g.round()).all()) else 16              # every square is a multiple of 1 / unit
    assert torch.equal((g * g * unit).round(), g * g * unit)
    assert float(sq.sum()) * unit < X.EXACT_LIMIT, f'total sum of squares {float(sq.sum()):g}: partial sums not exact'
    return torch.cat([sq.sqrt(), sq.sum().sqrt().reshape(1)]).float(), sq


def clip_coef(norms32, clip):
    """The kernel's coefficient in float32: clip / (n + 1e-6f) where that is < 1, else 1."""
    c = torch.tensor(clip, dtype=F32) / (norms32.float() + torch.tensor(1e-6, dtype=F32))
    return torch.where(c < 1, c, torch.ones_like(c))


def _chk(exact, name, v):
    if exact:
        X.assert_fp32_exact(name, v)
    return v


def sgd_step(p, g, m, coef, lr, wd, mom, nesterov, first, exact=False):
    """One step of mt_step_kernel<false> in the dtype of the operands (float64 with exact=True asserts every intermediate
    fp32-exact, so that neither the order nor fma contraction matters)."""
    gv = _chk(exact, 'g coef', g * coef)
    gv = _chk(exact, 'g + wd p', gv + _chk(exact, 'wd p', wd * p))
    m = gv if first else _chk(exact, 'm', _chk(exact, 'mom m', mom * m) + gv)
    d = _chk(exact, 'd', gv + _chk(exact, 'mom m2', mom * m)) if nesterov else m
    return _chk(exact, 'p', p - _chk(exact, 'lr d', lr * d)), m


def adamw_step(p, g, m, v, coef, lr, wd, b1, b2, eps, bc1, bc2, exact=False):
    """One step of mt_step_kernel<true>.  exact=True (float64 operands): every product feeding an addition is asserted
    fp32-exact; the sqrt, the two divisions, the + eps and the final subtraction are then single correctly rounded float32
    operations, done in float32, and the result is the float32 replay."""
    if not exact:
        gv = g * coef
        p = p * (1 - lr * wd)
        m = b1 * m + (1 - b1) * gv
        v = b2 * v + (1 - b2) * gv * gv
        denom = torch.sqrt(v) / torch.sqrt(bc2) + eps
        return p - (lr / bc1) * (m / denom), m, v, denom
    gv = _chk(True, 'g coef', g * coef)
    p = _chk(True, 'p decay', p * _chk(True, '1 - lr wd', 1 - _chk(True, 'lr wd', lr * wd)))
    m = _chk(True, 'm', _chk(True, 'b1 m', b1 * m) + _chk(True, '(1-b1) g', (1 - b1) * gv))
    v = _chk(True, 'v', _chk(True, 'b2 v', b2 * v) + _chk(True, '(1-b2) g g', _chk(True, '(1-b2) g', (1 - b2) * gv) * gv))
    step = _chk(True, 'lr / bc1', lr / bc1)
    assert bool((torch.log2(step) % 1 == 0).all()), 'lr / bc1 must be a power of two: the product is then exact'
    s2 = _chk(True, 'sqrt bc2', torch.sqrt(bc2))
    assert bool((torch.log2(s2) % 1 == 0).all())
    f = lambda a: a.float()                                        # noqa: E731
    denom = torch.sqrt(f(v)) / f(s2) + f(torch.as_tensor(eps, dtype=F64))           # sqrt rounds; / 2^k exact; + eps rounds
    q = f(m) / denom                                                                # rounds
    return (f(p) - f(step) * q).double(), m, v, q.double()                          # product exact; subtraction rounds


def sgd_exact_expected(lay, clip, nesterov, first, steps=2):
    """[(p, m, g, norms)] after each of `steps` exact SGD steps (momentum 0.5, MT_GROUPS; the first with first_step = `first`;
    clip = 1 uses the designed-norm gradients), asserting the premise on the way."""
    p = mt_params(lay)
    m = torch.zeros_like(p)
    lr, wd = lay.hyper(MT_GROUPS)
    out = []
    for step in range(steps):
        g = mt_grads(lay, 'clip' if clip else 'ints', seed=2 + step)
        norms, _ = mt_norms_expected(lay, g)
        coef = lay.per_element(clip_coef(norms[:-1], clip).double()) if clip else torch.ones_like(p)
        p, m = sgd_step(p, g, m, coef, lr, wd, 0.5, nesterov, first and step == 0, exact=True)
        out.append((p, m, g, norms))
    return out


ADAMW_EXACT = dict(b1=0.5, b2=0.75, eps=2.0 ** -10)


def adamw_exact_case(lay, wd_on, preload):
    """Step 1 (bias corrections 0.5 and 0.25) from zero state, or from dyadic m (k/4) and v (4 k) handed in through the table."""
    p, g = mt_params(lay), mt_grads(lay, 'ints')
    m = X.ints((lay.numel,), -8, 8, 1.0, 11).double() / 4 if preload else torch.zeros_like(p)
    v = X.ints((lay.numel,), 0, 16, 1.0, 12).double() * 4 if preload else torch.zeros_like(p)
    groups = MT_GROUPS_ADAMW if wd_on else tuple((lr_, 0.0) for lr_, _ in MT_GROUPS_ADAMW)
    lr, wd = lay.hyper(groups)
    h = adamw_hyper(step=1, **ADAMW_EXACT)
    p1, m1, v1, q = adamw_step(p, g, m, v, torch.ones_like(p), lr, wd, h['b1'], h['b2'], h['eps'], torch.tensor(h['bc1'], dtype=F64),
                               torch.tensor(h['bc2'], dtype=F64), exact=True)
    return dict(p0=p, g=g, m0=m, v0=v, p=p1, m=m1, v=v1, q=q, groups=groups)


def opt_bounds(kind, ref, K):
    """ref: dict of the float64 step (p, m, v, dP, dM) -> bounds dict; module docstring."""
    b = dict(p=U24 * (ref['p'].abs() + K * ref['dP']), m=U24 * K * ref['dM'])
    if kind == 'adamw':
        b['v'] = U24 * K * ref['v']
    return b


def general_step64(kind, p, g, m, v, coef, lr, wd, h):
    """float64 reference of one general step from float32 state, and the scales of its bound."""
    if kind == 'sgd':
        p1, m1 = sgd_step(p, g, m, coef, lr, wd, h['mom'], True, False)
        dM = (g * coef).abs() + (wd * p).abs() + h['mom'] * m.abs()
        return dict(p=p1, m=m1, dM=dM, dP=lr * dM * (1 + h['mom']))
    bc2 = torch.tensor(h['bc2'], dtype=F64)
    p1, m1, v1, denom = adamw_step(p, g, m, v, coef, lr, wd, h['b1'], h['b2'], h['eps'], h['bc1'], bc2)
    dM = h['b1'] * m.abs() + (1 - h['b1']) * (g * coef).abs()
    return dict(p=p1, m=m1, v=v1, dM=dM, dP=lr * wd * p.abs() + (lr / h['bc1']) * dM / denom)


def general_step32(kind, p, g, m, v, coef, lr, wd, h):
    """The same step as float32 CPU arithmetic, operation by operation (no contraction)."""
    f = lambda a: torch.as_tensor(a, dtype=F64).float()            # noqa: E731
    if kind == 'sgd':
        p1, m1 = sgd_step(f(p), f(g), f(m), f(coef), f(lr), f(wd), f(h['mom']), True, False)
        return dict(p=p1, m=m1)
    p1, m1, v1, _ = adamw_step(f(p), f(g), f(m), f(v), f(coef), f(lr), f(wd), f(h['b1']), f(h['b2']), f(h['eps']), f(h['bc1']),
                               f(h['bc2']))
    return dict(p=p1, m=m1, v=v1)


def adamw_hyper(b1, b2, eps, step):
    """The float32 hyper-parameters as float64 and the bias corrections as vtx_mt_adamw_step forms them (double pow, then float)."""
    b1, b2, eps = (float(np.float32(v)) for v in (b1, b2, eps))
    return dict(b1=b1, b2=b2, eps=eps, bc1=float(np.float32(1.0 - b1 ** step)), bc2=float(np.float32(1.0 - b2 ** step)))


def opt_check(name, kind, got, ref, K, quiet=False, sel=None):
    """got: dict(p, m[, v]) float32 packed -> the K each needs; every element (of the mask sel) within opt_bounds(K)."""
    need, bad = {}, []
    if sel is not None:
        got = {k_: v[sel] for k_, v in got.items()}
        ref = {k_: v[sel] for k_, v in ref.items()}
    for key in ('p', 'm', 'v') if kind == 'adamw' else ('p', 'm'):
        err = (got[key].double() - ref[key]).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
        fixed = U24 * ref['p'].abs() if key == 'p' else torch.zeros_like(err)
        per_k = U24 * {'p': ref['dP'], 'm': ref['dM'], 'v': ref.get('v')}[key]
        need[key] = k_needed(err, fixed, per_k)
        if need[key] > K:
            bad.append(f'{key} needs K = {need[key]:.3g}')
    if not quiet:
        report(f'{"FAIL" if bad else "ok  "} bound {name}: ' + ', '.join(f'{k_} K={v:.2f}' for k_, v in need.items()) + f' (bar K = {K})')
    assert not bad or quiet, f'{name}: beyond the bound at K = {K}: ' + '; '.join(bad)
    return need, not bad


def general_data(lay, kind, step, seed=40):
    """randn parameters (step 0) and gradients scaled 3 / 0.3 by tensor parity, as test_gpu_optim.py uses."""
    g = torch.randn(lay.numel, generator=X.gen(seed + step), dtype=F64).float().double()
    scale = torch.tensor([0.3 if t % 2 else 3.0 for t in range(lay.n)], dtype=F64)[lay.tid]
    return (g * scale).float().double()


# ==================================================================================================== MaskFeat
def mf_mask(B, Tq, g, kind, seed=0):
    if kind == 'zeros':
        return torch.zeros(B, Tq, g, g, dtype=torch.uint8)
    if kind == 'ones':
        return torch.ones(B, Tq, g, g, dtype=torch.uint8)
    return (torch.rand(B, Tq, g, g, generator=X.gen(seed)) > 0.5).to(torch.uint8)


def mf_expand(mask, r):
    """[B, Tq, g, g] mask -> [B * Tq * (g r) * (g r)] per token row."""
    return mask.repeat_interleave(r, 2).repeat_interleave(r, 3).reshape(-1).bool()


def mf_token(C, seed=0):
    """fp32 token values of which half are exact bf16 ties and the rest inexact under bf16 (a rounding case for the store)."""
    base = X.rne_bf16(torch.randn(C, generator=X.gen(seed), dtype=F64) * 4 + 0.5).double()
    half = 2.0 ** (torch.floor(torch.log2(base.abs().clamp_min(2.0 ** -100))) - 8)      # half a bf16 ulp
    frac = torch.where(torch.arange(C) % 2 == 0, torch.ones(C, dtype=F64), torch.full((C,), 0.375, dtype=F64))
    tok = base + torch.sign(base) * half * frac
    X.assert_fp32_exact('mask token', tok)
    return tok


def mf_blend_x(rows, C, dtype, seed=0):
    """bf16: every bf16 pattern class (all finite normal values, in pattern order, repeated); fp32: random values."""
    if dtype == BF16:
        import exact_gelu
        v = exact_gelu.all_bf16()
        reps = -(-rows * C // v.numel())
        return v.repeat(reps)[:rows * C].reshape(rows, C).to(BF16)
    return torch.randn(rows, C, generator=X.gen(seed))


def mf_counts_mask(cells, count, seed=0):
    """uint8 cell mask with exactly `count` cells set, spread over the whole range (the last cell included when count > 0)."""
    cm = torch.zeros(cells, dtype=torch.uint8)
    if count:
        at = torch.linspace(0, cells - 1, count).round().long() if count > 1 else torch.tensor([cells - 1])
        assert at.unique().numel() == count
        cm[at] = 1
    return cm


def mf_loss_case(B, Tq, ts, g, Cf, count, dtype, pad=0, seed=0):
    """Dyadic pred (bf16-exact multiples of 1/4 in [-4, 4]) and target (multiples of 1/8): every squared difference is a
    multiple of 1/64 below 2^7, every sum exact in float64 in any order; with Cf a power of two e / Cf is exact too, so the
    two accumulators are unique.  pred [rows, ts Cf + pad] (ldp = ts Cf + pad, junk in the padding)."""
    rows, cells = B * Tq * g * g, B * Tq * ts * g * g
    pred = X.ints((rows, ts * Cf + pad), -16, 16, 1.0, seed).double() / 4.0
    target = X.ints((cells, Cf), -32, 32, 1.0, seed + 1).double() / 8.0
    cm = mf_counts_mask(cells, count, seed + 2)
    p5 = pred[:, :ts * Cf].reshape(B, Tq, g, g, ts, Cf).permute(0, 1, 4, 2, 3, 5).reshape(cells, Cf)
    diff = p5 - target
    e = (diff * diff).sum(1)
    lsum = (e / Cf * cm).sum()                                                      # float64; exact when Cf is a power of two
    den = (torch.tensor(float(count), dtype=F32) + torch.tensor(1e-5, dtype=F32)).double()
    return dict(B=B, Tq=Tq, ts=ts, g=g, Cf=Cf, count=count, pred=pred, target=target, cmask=cm, ldp=ts * Cf + pad,
                diff=diff, cells=cells, rows=rows, lsum=lsum, den=den, loss=lsum / den, exact=Cf & (Cf - 1) == 0)


def mf_loss_bwd_expected(c, gloss, dtype):
    """T(float32(coef (pred - target))) with coef = (gloss 2) / (Cf double(float32(n) + 1e-5f)) in [rows, ts Cf] layout: every
    operation of the kernel is one IEEE double or float operation (the file is built with contraction off)."""
    B, Tq, ts, g, Cf = c['B'], c['Tq'], c['ts'], c['g'], c['Cf']
    coef = torch.tensor(float(np.float32(gloss)), dtype=F64) * 2.0 / (float(Cf) * c['den'])
    gv = (coef * c['diff']).float() * c['cmask'][:, None].float()
    gv = gv.reshape(B, Tq, ts, g, g, Cf).permute(0, 1, 3, 4, 2, 5).reshape(c['rows'], ts * Cf)
    return gv.to(dtype)
