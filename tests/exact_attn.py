"""Exact-arithmetic cases for the attention kernels: routed scores (imported by test modules; not a conftest).

Softmax is made exact by the choice of Q and K.  In every (sequence, head) item the keys are split into groups of 1, 2
or 4, and every group gets a code: a pair (a, b) of routing dims 0..R-1.  A key has 1 at its code's two dims; a query has 0
at its group's two dims and -T_NEG at the other routing dims.  The raw score q.k is then exactly 0 for the 2^k keys of the
query's group (its winners) and -T_NEG or -2 T_NEG for every other key.  With SCALE = 2^-3, exp2 of a loser's scaled score
(<= -369) is exactly 0 in fp32, so the forward has m = 0, l = 2^k, P in {0, 2^-k} and O = (sum of the winners' v) / 2^k.
The free dims above R carry small integers: Q in the lower half, K in the upper half, so they never touch a score but make
dq and dk non-trivial.  V and dO are small integers; dO is sparse, so dS = 2^-k (dP - delta) is bf16-representable and
the bf16 packs of P and dS in the MFMA kernels are exact.  On those paths every output equals RNE(exact value).

Group codes are drawn from a small alphabet per item, independently for every item.  A key read from the wrong place (a
neighbouring sequence, the wrong frame, a stale row of the previous item, an unmasked zero-filled pad) then very likely
scores 0 with some query and adds a winner, which moves P from 2^-k to 1 / (2^k + 1).

Layouts: 'contig' (sequence s = rows [s L, (s+1) L)), 'space' (VTX_ATTN_SPACE: clip b, frame t; the cls row is shared by
the T frames of a clip, so its code, Q, K and V are drawn once per (clip, head)), 'time_cls' (VTX_ATTN_TIME_CLS: clip b,
patch position p; the cls row is shared by the P sequences of a clip), 'space_nocls' (VTX_ATTN_SPACE_NOCLS: clip b, frame
t, token rows only), 'cross' (separate q [B, Lq, C] and k, v [B, Lk, C]).  layout_rows restates the row addressing of the
three strided layouts.  The float64 reference works on the winner lists, never on a dense L x L matrix.

Kinds: 'exact' (every output representable in bf16), 'round' (forward only: V in 128..255, ties and inexact outputs at the
store) and 'graded' (forward only: winners' scores graded in steps of 8 under a scale that makes c2 exactly 2^-3, so the
rescale of the online softmax takes the factors 1/2 and 1/4; see the section "graded scores").  A case carries the scale
it is to be run with: SCALE, or SCALE_GRADED for 'graded'.
"""
import math

import numpy as np
import torch

import exact as X

T_NEG = 2048.0                      # loser scores are <= -T_NEG
SCALE = 2.0 ** -3                   # = 64^-0.5: the model's own scale for head_dim 64, and a power of two
LN2 = math.log(2.0)
assert T_NEG * SCALE * math.log2(math.e) >= 200   # exp2 of every loser's scaled score underflows to exactly 0
DS_GRAIN = 2.0 ** -4                # dS = n / 4^k, k <= 2
PROBE = -1                          # V[:, PROBE] = rank in the group - 1: distinct within a group (see _repair_dO)


def _pairs(R):
    return [(a, b) for a in range(R) for b in range(a + 1, R)]


def routing_dims(ngroups):
    """Smallest R >= 4 whose pair alphabet holds ngroups codes."""
    R = 4
    while R * (R - 1) // 2 < ngroups:
        R += 1
    return R


def edge_keys(nk):
    """Keys that must be winners with non-zero dS: the first and last key of every 32-row (and so 64-row) tile, and the
    last key."""
    e = {i for i in range(nk) if i % 32 in (0, 31)} | {nk - 1}
    return sorted(e)


def _draw_groups(nk, rng, required, first):
    """One draw of _groups; None where a required singleton finds no larger group with a key it may take."""
    perm = list(rng.permutation(nk))
    if first:
        perm.remove(0)
        perm.insert(0, 0)
    groups, i = [], 0
    while i < nk:
        s = int(rng.choice([1, 2, 4], p=[0.25, 0.45, 0.30]))
        while s > nk - i:
            s //= 2
        groups.append(perm[i:i + s])
        i += s
    req = set(required)
    if nk >= 2:
        for g in groups:
            if len(g) == 1 and g[0] in req:
                # swap the required singleton with a non-required member of a larger group (never key 0 of `first`)
                for h in groups:
                    cand = [x for x in h if x not in req and not (first and x == 0)] if len(h) >= 2 else []
                    if cand:
                        x = cand[0]
                        h[h.index(x)], g[0] = g[0], x
                        break
                else:
                    return None
    if first:
        g0 = next(g for g in groups if 0 in g)
        g0.remove(0)
        g0.insert(0, 0)
    return groups


def _groups(nk, rng, required, first):
    """Partition range(nk) into groups of 1, 2 or 4; every required key in a group of >= 2 (when nk >= 2); key 0 first in
    its group when `first`.  A draw that cannot place a required key (a few keys, most of them required: at nk = 3 only
    [0, 2], [1] serves) is drawn again; a draw that can is returned as it always was, from the same random numbers."""
    for _ in range(64):
        groups = _draw_groups(nk, rng, required, first)
        if groups is not None:
            return groups
    raise AssertionError('no group to move a required key into')


def route_item(nq, nk, R, rng, required=(), first_code=None):
    """Routing of one item.  Returns kcode [nk], qcode [nq] (code indices into _pairs(R)), win [nq, 4] (winner key
    indices, -1 padded), nwin [nq] and rank [nk] (position of the key in its group).  first_code: key 0's group gets this
    code and query 0 takes key 0's group (the shared cls row of space mode)."""
    groups = _groups(nk, rng, required, first_code is not None)
    ncodes = R * (R - 1) // 2
    assert len(groups) <= ncodes, (len(groups), ncodes)
    if first_code is None:
        codes = rng.choice(ncodes, len(groups), replace=False)
    else:
        rest = rng.permutation([c for c in range(ncodes) if c != first_code])[:len(groups) - 1]
        codes = np.array([first_code if 0 in g else 0 for g in groups])
        codes[[j for j, g in enumerate(groups) if 0 not in g]] = rest
    kcode = np.empty(nk, np.int64)
    rank = np.empty(nk, np.int64)
    for g, c in zip(groups, codes):
        kcode[g] = c
        rank[g] = np.arange(len(g))
    # queries: cover every group once (query 0 -> key 0's group when first_code), the rest at random
    order = list(rng.permutation(len(groups)))
    if first_code is not None:
        g0 = next(j for j, g in enumerate(groups) if 0 in g)
        order.remove(g0)
        order.insert(0, g0)
    qgrp = np.array((order + list(rng.integers(0, len(groups), max(0, nq - len(groups)))))[:nq])
    if first_code is None:
        qgrp = qgrp[rng.permutation(nq)]
    else:
        qgrp[1:] = qgrp[1:][rng.permutation(nq - 1)]
    win = np.full((nq, 4), -1, np.int64)
    nwin = np.empty(nq, np.int64)
    for i, gi in enumerate(qgrp):
        g = groups[gi]
        win[i, :len(g)] = g
        nwin[i] = len(g)
    return kcode, codes[qgrp], win, nwin, rank


def _ints(rng, shape, lo, hi, density=1.0):
    v = rng.integers(lo, hi + 1, shape).astype(np.float64)
    if density < 1.0:
        v *= rng.random(shape) < density
    return v


class Items:
    """Batch of I routed items with nq queries and nk keys each (float64 numpy): Q, dO [I, nq, hd]; K, V [I, nk, hd];
    win [I, nq, 4]; nwin [I, nq]; kcode / qcode; R, hd, kind ('exact' | 'round' | 'graded'), bwd.  Graded items (build_graded)
    also carry grade [I, nk], top [I, nq] and straddle."""


def build_items(I, nq, nk, hd, kind, bwd, seed, R=None, shared=None, required=None):
    """I items.  shared: dict(first_code [I], Q0 [I, hd], K0 [I, hd], V0 [I, hd]) -- row 0 of Q / K / V and its code fixed
    per item (the cls row of space mode, drawn once per clip and head)."""
    rng = np.random.default_rng(seed)
    if R is None:
        R = routing_dims(int(math.ceil(nk / 1.3)) + 2)
    required = edge_keys(nk) if required is None else required
    it = Items()
    it.I, it.nq, it.nk, it.hd, it.kind, it.bwd, it.R = I, nq, nk, hd, kind, bwd, R
    pairs = np.array(_pairs(R))
    kcode = np.empty((I, nk), np.int64)
    qcode = np.empty((I, nq), np.int64)
    win = np.empty((I, nq, 4), np.int64)
    nwin = np.empty((I, nq), np.int64)
    rank = np.empty((I, nk), np.int64)
    for n in range(I):
        fc = None if shared is None else int(shared['first_code'][n])
        kcode[n], qcode[n], win[n], nwin[n], rank[n] = route_item(nq, nk, R, rng, required, fc)
    fa = R + (hd - R) // 2                                # free dims: Q in [R, fa), K in [fa, hd)
    Q = np.full((I, nq, hd), -T_NEG)
    Q[:, :, fa:] = 0.0
    Q[:, :, R:fa] = _ints(rng, (I, nq, fa - R), -2, 2, 0.5)
    qa = pairs[qcode]                                     # [I, nq, 2]
    np.put_along_axis(Q, qa, 0.0, axis=2)
    K = np.zeros((I, nk, hd))
    K[:, :, fa:] = _ints(rng, (I, nk, hd - fa), -2, 2, 0.5)
    np.put_along_axis(K, pairs[kcode], 1.0, axis=2)
    if kind == 'round':
        V = _ints(rng, (I, nk, hd), 128, 255)
    else:
        V = _ints(rng, (I, nk, hd), -3, 3)
    if bwd:
        V[:, :, PROBE] = rank - 1
    dO = _ints(rng, (I, nq, hd), -1, 1, 4.0 / hd)
    if shared is not None:
        Q[:, 0], K[:, 0], V[:, 0] = shared['Q0'], shared['K0'], shared['V0']
    it.Q, it.K, it.V, it.dO, it.win, it.nwin, it.kcode, it.qcode = Q, K, V, dO, win, nwin, kcode, qcode
    if bwd:
        _repair_dO(it, required)
    return it


def shared_rows(I, hd, R, kind, bwd, seed):
    """Row 0 of Q / K / V and its code for I (clip, head) pairs: the shared cls row of space mode."""
    rng = np.random.default_rng(seed)
    pairs = np.array(_pairs(R))
    code = rng.integers(0, len(pairs), I)
    fa = R + (hd - R) // 2
    Q0 = np.full((I, hd), -T_NEG)
    Q0[:, fa:] = 0.0
    Q0[:, R:fa] = _ints(rng, (I, fa - R), -2, 2, 0.5)
    np.put_along_axis(Q0, pairs[code], 0.0, axis=1)
    K0 = np.zeros((I, hd))
    K0[:, fa:] = _ints(rng, (I, hd - fa), -2, 2, 0.5)
    np.put_along_axis(K0, pairs[code], 1.0, axis=1)
    V0 = _ints(rng, (I, hd), 128, 255) if kind == 'round' else _ints(rng, (I, hd), -3, 3)
    if bwd:
        V0[:, PROBE] = -1.0                               # key 0 is first in its group: rank 0
    return dict(first_code=code, Q0=Q0, K0=K0, V0=V0)


def _ds(it):
    """dS [I, nq, 4] (0 on the padding of the winner lists) and the intermediates, float64."""
    I, nq = it.I, it.nq
    wi = np.where(it.win >= 0, it.win, 0)
    valid = it.win >= 0
    Vw = it.V[np.arange(I)[:, None, None], wi]
    P = valid / it.nwin[..., None]
    O = (Vw * valid[..., None]).sum(2) / it.nwin[..., None]
    dP = (Vw * it.dO[:, :, None, :]).sum(-1)
    delta = (O * it.dO).sum(-1)
    dS = P * (dP - delta[..., None]) * valid
    return wi, valid, P, O, dP, delta, dS


def _repair_dO(it, required):
    """Every required key must be a winner with non-zero dS for some query.  Where none is, dO[i, PROBE] of one query of
    its group is reset to the value in -2..2 that leaves the fewest required keys without one (V[:, PROBE] differs within
    a group, so dS of the key is a non-constant linear function of that value)."""
    if it.nk < 2:
        return
    req = [j for j in required if j < it.nk]

    def missing(n):
        wi, valid, dS = _ds_item(it, n)
        live = valid & (np.abs(dS) > 0)
        return [j for j in req if not (live & (wi == j)).any()], wi, valid

    for n in range(it.I):
        for _ in range(8):
            miss, wi, valid = missing(n)
            if not miss:
                break
            j = miss[0]
            qs = np.nonzero(((wi == j) & valid).any(1) & (it.nwin[n] >= 2))[0]
            i = qs[_ % len(qs)]
            best = None
            for v in (1.0, -1.0, 2.0, -2.0, 0.0):
                it.dO[n, i, PROBE] = v
                m = len(missing(n)[0])
                if best is None or m < best[0]:
                    best = (m, v)
            it.dO[n, i, PROBE] = best[1]


def _ds_item(it, n):
    wi = np.where(it.win[n] >= 0, it.win[n], 0)
    valid = it.win[n] >= 0
    Vw = it.V[n][wi]
    P = valid / it.nwin[n][:, None]
    O = (Vw * valid[..., None]).sum(1) / it.nwin[n][:, None]
    dP = (Vw * it.dO[n][:, None, :]).sum(-1)
    delta = (O * it.dO[n]).sum(-1)
    return wi, valid, P * (dP - delta[:, None]) * valid


# ------------------------------------------------------------------------------------------------ graded scores
# kind 'graded' (forward only): the online softmax's rescale factor takes the values 1/2 and 1/4, not only 0 and 1.
# The kernels form c2 = scale * LOG2E in fp32; with scale = fl32(ln 2) / 8 that product is exactly 2^-3 (asserted below and in
# tests/test_exact_attn_graded_premise.py; both fp32 neighbours of fl32(ln 2) miss it), so raw scores that are multiples of 8
# are integers in the exponent and alpha and every probability are powers of two.  Two more routing dims, R and R + 1, grade
# the scores: in dim R a key carries -grade and every query 8; in dim R + 1 every key carries 1 and a query -8 top.  A winner
# scores -8 (grade + top), a loser at most -T_NEG.  Groups of 1, 2 and 4 keys hold the grades (0), (0, 0) and (2, 2, 1, 0) in
# the order of the key index, so l = sum 2^-grade is 1, 2 or 2, the final maximum is -8 top, lse = (log2 l - top) ln 2, and the
# running maximum of a four-group rises along the keys.  For every chunk boundary b (the multiples of 64 below nk: the 64-key
# chunks of attn_hd.hip, the 128-key chunks and blocks of the others) STRADDLE queries take a four-group with keys on both
# sides of b: the maximum they carry into the later chunk is lower by 8 or 16 than the one they find there.
# V holds integers 1..31: O = (sum 2^-grade v) / l is n / 8 with n <= 248, representable in bf16, and there is no
# cancellation, so an ulp on an unpacked fp32 factor (should the hardware's exp2 miss a power of two by one) stays a relative
# error of a few 2^-24 and cannot move the stored bf16 value.
LOG2E_F32 = np.float32(1.4426950408889634)         # csrc/attn_common.h
SCALE_GRADED = float(np.float32(math.log(2.0)) / np.float32(8.0))
assert np.float32(SCALE_GRADED) * LOG2E_F32 == np.float32(0.125)
GRADES = {1: (0,), 2: (0, 0), 4: (2, 2, 1, 0)}
TOPS = 3                                           # top in 0 .. TOPS - 1
STRADDLE = 8                                       # queries per chunk boundary and item
CHUNK_EDGE = 64


def chunk_bounds(nk):
    return list(range(CHUNK_EDGE, nk, CHUNK_EDGE))


def _graded_groups(nk, rng, g0):
    """Partition of range(nk) into ascending groups of 1, 2 or 4 and, per chunk boundary, the indices of the four-groups built
    to straddle it (up to STRADDLE, as many as the keys on either side allow, at least one; 1, 2 or 3 of the four keys on
    the later side).  g0 (None: no shared row): the grade of key 0 -- 2 puts it in a four-group, where the lowest key index
    has that grade, 0 in a group of 1 or 2; the third value is the index of key 0's group."""
    free = set(range(nk)) - ({0} if g0 is not None else set())
    groups, strad = [], {}
    for b in chunk_bounds(nk):
        early = [int(x) for x in rng.permutation(sorted(x for x in free if b - CHUNK_EDGE <= x < b))]
        late = [int(x) for x in rng.permutation(sorted(x for x in free if b <= x < b + CHUNK_EDGE))]
        strad[b] = []
        for j in range(STRADDLE):
            nl = min(1 + j % 3, len(late))
            if nl == 0 or len(early) < 4 - nl:
                break
            g = sorted([late.pop() for _ in range(nl)] + [early.pop() for _ in range(4 - nl)])
            free -= set(g)
            strad[b].append(len(groups))
            groups.append(g)
        assert strad[b], f'no four-group straddles key {b} of {nk}'
    first = None
    if g0 is not None:
        rest = [int(x) for x in rng.permutation(sorted(free))]
        size = 4 if g0 == 2 else int(rng.choice([1, 2]))
        assert len(rest) >= size - 1
        g = [0] + sorted(rest[:size - 1])
        free -= set(g)
        first = len(groups)
        groups.append(g)
    perm = [int(x) for x in rng.permutation(sorted(free))]
    i = 0
    while i < len(perm):
        s = int(rng.choice([1, 2, 4], p=[0.25, 0.45, 0.30]))
        while s > len(perm) - i:
            s //= 2
        groups.append(sorted(perm[i:i + s]))
        i += s
    return groups, strad, first


def build_graded(I, nq, nk, hd, seed, R=None, shared=None):
    """I graded items (see above).  shared: dict(first_code, g0, top0 [I]; Q0, K0, V0 [I, hd]) -- the shared cls row: code,
    grade entry, top, Q, K and V of row 0 fixed per item; query 0 takes key 0's group.  Items gains grade [I, nk], top
    [I, nq] and straddle {b: [I, STRADDLE] query indices}."""
    rng = np.random.default_rng(seed)
    if R is None:
        R = routing_dims(int(math.ceil(nk / 1.3)) + 2)
    R2 = R + 2
    assert R2 + 2 <= hd, (R, hd)
    bounds = chunk_bounds(nk)
    assert nq >= STRADDLE * len(bounds) + 1, 'too few queries for the straddle quota'
    it = Items()
    it.I, it.nq, it.nk, it.hd, it.kind, it.bwd, it.R = I, nq, nk, hd, 'graded', False, R
    pairs = np.array(_pairs(R))
    ncodes = len(pairs)
    kcode = np.empty((I, nk), np.int64)
    grade = np.empty((I, nk), np.int64)
    qcode = np.empty((I, nq), np.int64)
    win = np.full((I, nq, 4), -1, np.int64)
    nwin = np.empty((I, nq), np.int64)
    it.straddle = {b: np.empty((I, STRADDLE), np.int64) for b in bounds}
    for n in range(I):
        g0 = None if shared is None else int(shared['g0'][n])
        groups, strad, first = _graded_groups(nk, rng, g0)
        assert len(groups) <= ncodes, (len(groups), ncodes)
        if shared is None:
            codes = rng.choice(ncodes, len(groups), replace=False)
        else:
            fc = int(shared['first_code'][n])
            codes = np.full(len(groups), fc)
            others = [j for j in range(len(groups)) if j != first]
            codes[others] = rng.permutation([c for c in range(ncodes) if c != fc])[:len(others)]
        for g, c in zip(groups, codes):
            kcode[n, g] = c
            grade[n, g] = GRADES[len(g)]
        # queries: query 0 -> key 0's group (shared row); STRADDLE per boundary, round-robin over its groups; then every group
        # not yet taken once, as far as the queries go; the rest at random
        head = [] if first is None else [first]
        quota = [strad[b][j % len(strad[b])] for b in bounds for j in range(STRADDLE)]
        taken = set(head + quota)
        cover = [int(j) for j in rng.permutation(len(groups)) if j not in taken]
        tail = (quota + cover + [int(j) for j in rng.integers(0, len(groups), nq)])[:nq - len(head)]
        pos = rng.permutation(nq - len(head)) + len(head)                  # position of every entry of tail
        qgrp = np.empty(nq, np.int64)
        qgrp[:len(head)] = head
        qgrp[pos] = tail
        for k, b in enumerate(bounds):
            it.straddle[b][n] = pos[k * STRADDLE:(k + 1) * STRADDLE]
        for i, gi in enumerate(qgrp):
            g = groups[gi]
            win[n, i, :len(g)] = g
            nwin[n, i] = len(g)
        qcode[n] = codes[qgrp]
    top = rng.integers(0, TOPS, (I, nq))
    fa = R2 + (hd - R2) // 2                               # free dims: Q in [R2, fa), K in [fa, hd)
    Q = np.full((I, nq, hd), -T_NEG)
    Q[:, :, fa:] = 0.0
    Q[:, :, R2:fa] = _ints(rng, (I, nq, fa - R2), -2, 2, 0.5)
    np.put_along_axis(Q, pairs[qcode], 0.0, axis=2)
    K = np.zeros((I, nk, hd))
    K[:, :, fa:] = _ints(rng, (I, nk, hd - fa), -2, 2, 0.5)
    np.put_along_axis(K, pairs[kcode], 1.0, axis=2)
    V = _ints(rng, (I, nk, hd), 1, 31)
    if shared is not None:
        top[:, 0] = shared['top0']
        assert (grade[:, 0] == shared['g0']).all()
        Q[:, 0], K[:, 0], V[:, 0] = shared['Q0'], shared['K0'], shared['V0']
    Q[:, :, R], Q[:, :, R + 1] = 8.0, -8.0 * top
    K[:, :, R], K[:, :, R + 1] = -grade, 1.0
    it.Q, it.K, it.V, it.win, it.nwin, it.kcode, it.qcode, it.grade, it.top = Q, K, V, win, nwin, kcode, qcode, grade, top
    it.dO = np.zeros((I, nq, hd))
    return it


def shared_rows_graded(I, hd, R, seed):
    """Row 0 of Q / K / V, its code, its grade entry (0 or 2) and its top for I (clip, head) pairs: drawn once each."""
    rng = np.random.default_rng(seed)
    pairs = np.array(_pairs(R))
    code = rng.integers(0, len(pairs), I)
    g0 = 2 * rng.integers(0, 2, I)
    top0 = rng.integers(0, TOPS, I)
    R2 = R + 2
    fa = R2 + (hd - R2) // 2
    Q0 = np.full((I, hd), -T_NEG)
    Q0[:, fa:] = 0.0
    Q0[:, R2:fa] = _ints(rng, (I, fa - R2), -2, 2, 0.5)
    np.put_along_axis(Q0, pairs[code], 0.0, axis=1)
    K0 = np.zeros((I, hd))
    K0[:, fa:] = _ints(rng, (I, hd - fa), -2, 2, 0.5)
    np.put_along_axis(K0, pairs[code], 1.0, axis=1)
    V0 = _ints(rng, (I, hd), 1, 31)
    return dict(first_code=code, g0=g0, top0=top0, Q0=Q0, K0=K0, V0=V0)


def straddle_counts(it):
    """{b: [I] number of queries whose winners lie on both sides of key b with the strictly higher score on the later side}"""
    valid = it.win >= 0
    wi = np.where(valid, it.win, 0)
    g = np.take_along_axis(it.grade, wi.reshape(it.I, -1), 1).reshape(wi.shape).astype(np.float64)
    res = {}
    for b in chunk_bounds(it.nk):
        early = np.where(valid & (wi < b), -g, -np.inf).max(2)              # best score / 8 on either side (top is common)
        late = np.where(valid & (wi >= b), -g, -np.inf).max(2)
        res[b] = (np.isfinite(early) & np.isfinite(late) & (late > early)).sum(1)
    return res


def reference_graded(it):
    """Exact float64 results of graded items, with every premise asserted.  Returns a dict of torch float64: O, O_abs (= O: V is
    positive) [I, nq, hd], O_n (terms per output), lse, log2l, top [I, nq], nwin."""
    I, nq, nk = it.I, it.nq, it.nk
    assert not it.bwd and np.isin(it.nwin, (1, 2, 4)).all()
    for name, a in (('Q', it.Q), ('K', it.K), ('V', it.V)):
        t = torch.from_numpy(a)
        assert torch.equal(X.rne_bf16(t).double(), t), f'{name} is not bf16-representable'
    valid = it.win >= 0
    wi = np.where(valid, it.win, 0)
    gw = np.take_along_axis(it.grade, wi.reshape(I, -1), 1).reshape(wi.shape)
    # dense scores of every item: a winner scores -8 (grade + top), every other key <= -T_NEG; exponents relative to the row
    # maximum, in the kernels' fp32 arithmetic: winners are integers, losers underflow (<= -150: below the smallest denormal)
    for n in range(I):
        s = it.Q[n] @ it.K[n].T
        w = np.zeros((nq, nk), bool)
        w[np.arange(nq)[:, None].repeat(4, 1)[valid[n]], wi[n][valid[n]]] = True
        want = -8.0 * (it.grade[n][None, :] + it.top[n][:, None])
        assert (s[w] == want[w]).all() and (s[~w] <= -T_NEG).all(), 'graded scores'
        assert (w.sum(1) == it.nwin[n]).all()
        assert (s.max(1) == -8.0 * it.top[n]).all(), 'the final maximum is -8 top'
        e = (s - s.max(1, keepdims=True)) * 0.125
        assert (e[w] == np.round(e[w])).all() and e[~w].max(initial=-np.inf) <= -150.0, 'exponents'
    assert np.abs(it.Q).sum(-1).max() * 2.0 < X.EXACT_LIMIT                    # |q.k| partial sums (|k| <= 2)
    assert np.abs(it.V).sum(1).max() < X.EXACT_LIMIT                           # O accumulator of a chunk that is wiped later
    wgt = np.where(valid, 2.0 ** -gw, 0.0)
    l = wgt.sum(2)
    assert np.isin(l, (1.0, 2.0)).all() and (l == np.where(it.nwin == 1, 1.0, 2.0)).all()
    assert ((np.diff(it.win, axis=2) > 0) | ~valid[..., 1:]).all(), 'winner lists ascend'
    assert ((np.diff(gw, axis=2) <= 0) | ~valid[..., 1:]).all(), 'the grade falls as the key index rises'
    Vw = it.V[np.arange(I)[:, None, None], wi]
    O = (wgt[..., None] * Vw).sum(2) / l[..., None]
    Ot = torch.from_numpy(O)
    assert torch.equal(X.rne_bf16(Ot).double(), Ot), 'graded case: O is not bf16-representable'
    for b, cnt in straddle_counts(it).items():
        assert (cnt >= STRADDLE).all(), f'boundary {b}: {cnt.min()} queries see the maximum rise across it'
        rows = it.straddle[b]
        lo = np.take_along_axis(it.win[:, :, 0], rows, 1)
        hi = np.take_along_axis(it.win[:, :, 3], rows, 1)
        assert ((lo < b) & (hi >= b)).all(), 'a straddle query does not straddle'
    log2l = np.log2(l)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))     # noqa: E731
    return dict(O=Ot, O_abs=Ot.clone(), O_n=t(np.broadcast_to(it.nwin[..., None], O.shape)), lse=t((log2l - it.top) * LN2),
                log2l=t(log2l), top=t(it.top), nwin=torch.from_numpy(it.nwin))


def reference(it, scale=SCALE):
    """Exact float64 results of one batch of items, with every premise asserted.  Returns a dict of torch float64:
    O [I, nq, hd], lse [I, nq], nwin [I, nq]; with bwd also dq [I, nq, hd], dk, dv [I, nk, hd] and their sums of |terms|
    (dq_abs, dk_abs, dv_abs) and term counts (dq_n, dk_n, dv_n), and probs_win (the winners' probability)."""
    I, nq, nk, hd = it.I, it.nq, it.nk, it.hd
    wi, valid, P, O, dP, delta, dS = _ds(it)
    assert (it.nwin >= 1).all() and np.isin(it.nwin, (1, 2, 4)).all(), 'a query without 2^k winners'
    for name, a in (('Q', it.Q), ('K', it.K), ('V', it.V), ('dO', it.dO)):    # the kernels see the bf16 inputs
        t = torch.from_numpy(a)
        assert torch.equal(X.rne_bf16(t).double(), t), f'{name} is not bf16-representable'
    # scores by construction: winners share the query's code, every other key has another code (-T_NEG or -2 T_NEG)
    kc_w = np.take_along_axis(it.kcode, wi.reshape(I, -1), 1).reshape(wi.shape)
    assert ((kc_w == it.qcode[..., None]) | ~valid).all()
    ncode = it.R * (it.R - 1) // 2
    per_code = np.bincount((np.arange(I)[:, None] * ncode + it.kcode).reshape(-1), minlength=I * ncode).reshape(I, ncode)
    cnt = np.take_along_axis(per_code, it.qcode, 1)
    assert (cnt == it.nwin).all(), 'winner lists do not hold every key of the query code'
    # dense scores on a sample of items: winners exactly 0, losers <= -T_NEG
    for n in sorted({0, I - 1}):
        s = it.Q[n] @ it.K[n].T
        w = np.zeros((nq, nk), bool)
        w[np.arange(nq)[:, None].repeat(4, 1)[valid[n]], wi[n][valid[n]]] = True
        assert (s[w] == 0).all() and (s[~w] <= -T_NEG).all(), 'routed scores'
    assert np.abs(it.Q).sum(-1).max() * 1.0 < X.EXACT_LIMIT                    # |q.k| partial sums (|k| <= 2)
    assert (np.abs(it.V).sum(1).max()) < X.EXACT_LIMIT                         # O accumulator (P = 1 in the forward)
    out = dict(O=torch.from_numpy(O), lse=torch.from_numpy(np.log(it.nwin.astype(np.float64))),
               nwin=torch.from_numpy(it.nwin), probs_win=torch.from_numpy(1.0 / it.nwin))
    X.assert_fp32_exact('O', out['O'])
    if not it.bwd:
        return out
    Ot = torch.from_numpy(O)
    assert torch.equal(X.rne_bf16(Ot).double(), Ot), 'backward case: O is not bf16-representable'
    dSt = torch.from_numpy(dS)
    assert torch.equal(X.rne_bf16(dSt).double(), dSt), 'dS not bf16-representable'
    assert torch.equal(X.rne_bf16(dSt * scale).double(), dSt * scale), 'dS * scale not bf16-representable'
    Pt = torch.from_numpy(P)
    assert torch.equal(X.rne_bf16(Pt).double(), Pt)
    X.assert_fp32_exact('dP', torch.from_numpy(dP))
    X.assert_fp32_exact('delta', torch.from_numpy(delta))
    ar = np.arange(I)[:, None, None]
    Kw = it.K[ar, wi]                                      # [I, nq, 4, hd]
    dq = (dS[..., None] * Kw).sum(2)
    dq_abs = (np.abs(dS)[..., None] * np.abs(Kw)).sum(2)
    dq_n = np.broadcast_to((dS != 0).sum(2)[..., None], dq.shape)      # non-zero terms: at most one per non-zero dS
    flat = (np.arange(I)[:, None, None] * nk + wi).reshape(-1)
    m = valid.reshape(-1)

    def scatter(term):                                      # term [I, nq, 4, hd] -> per key [I, nk, hd]
        t = torch.from_numpy(term.reshape(-1, hd)[m])
        acc = torch.zeros(I * nk, hd, dtype=torch.float64)
        acc.index_add_(0, torch.from_numpy(flat[m]), t)
        return acc.reshape(I, nk, hd).numpy()
    tk = dS[..., None] * it.Q[:, :, None, :]
    tv = P[..., None] * it.dO[:, :, None, :]
    dk, dk_abs, dv, dv_abs = scatter(tk), scatter(np.abs(tk)), scatter(tv), scatter(np.abs(tv))
    cnt_k = np.bincount(flat[m][(dS != 0).reshape(-1)[m]], minlength=I * nk).reshape(I, nk, 1)
    cnt_v = np.bincount(flat[m], minlength=I * nk).reshape(I, nk, 1)
    dk_n, dv_n = np.broadcast_to(cnt_k, dk.shape), np.broadcast_to(cnt_v, dv.shape)
    # every fp32 partial sum is a multiple of the grain below 2^24 grains
    assert dq_abs.max() < X.EXACT_LIMIT * DS_GRAIN and dk_abs.max() < X.EXACT_LIMIT * DS_GRAIN, 'dq / dk accumulator bound'
    assert dv_abs.max() < X.EXACT_LIMIT / 4, 'dv accumulator bound'
    for name, v in (('dq', dq), ('dk', dk), ('dv', dv)):
        X.assert_fp32_exact(name, torch.from_numpy(v))
    # coverage: at least half of the keys are winners; every edge key has a non-zero dS for some query
    is_win = np.zeros((I, nk), bool)
    is_win.reshape(-1)[flat[m]] = True
    assert is_win.mean() >= 0.5, f'only {is_win.mean():.0%} of the keys are winners'
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out.update(dq=t(dq * scale), dk=t(dk * scale), dv=t(dv), dq_abs=t(dq_abs * scale), dk_abs=t(dk_abs * scale),
               dv_abs=t(dv_abs), dq_n=t(dq_n), dk_n=t(dk_n), dv_n=t(dv_n), dS=dSt, win=t(it.win))
    return out


def assert_edges(it, ref, required=None):
    """Every required key is a winner with non-zero dS for some query, in every item (needs nk >= 2)."""
    if it.nk < 2:
        return
    required = edge_keys(it.nk) if required is None else required
    dS = ref['dS'].numpy()
    for j in required:
        hit = ((it.win == j) & (np.abs(dS) > 0)).any(axis=(1, 2))
        assert hit.all(), f'edge key {j}: no non-zero dS in items {np.nonzero(~hit)[0][:5].tolist()}'


# ------------------------------------------------------------------------------------------------ cases by layout
class Case:
    """A routed case in a physical layout: layout in 'contig', 'space', 'time_cls', 'space_nocls' (self-attention) or
    'cross'.  scale is the descriptor's scale (SCALE; SCALE_GRADED for kind 'graded', whose cases also carry out_abs / out_n for
    value_bounds and log2l / top, shaped as lse, for lse_graded_ok).  Self-attention cases carry their own B, T, P (0 for contig), cls_group -- the number of sequences that share one
    cls row: T for space, P for time_cls, 0 otherwise -- and cls_rows, the cls row of every clip in qkv / dqkv.
    Tensors (float64 CPU):
    self-attention: qkv [rows, 3D] (space_nocls: cls rows NaN), dout [out_rows, D]; expected out [out_rows, D], lse
    [S, H, L], dqkv [rows, 3D] (cls rows: NaN where cls_group, for they go to dqkv_cls [S, 3D]; zeros for space_nocls) and
    the bound tensors dqkv_abs / dqkv_n (same shape);
    cross: q [B, Lq, C], k, v [B, Lk, C], dout; expected out, lse [B, heads, Lq], dq, dk, dv and their *_abs / *_n."""


def _sh(a, S, H, L, hd):
    """[S*H, L, hd] (items s-major, heads fastest) -> [S, L, H*hd]."""
    return a.reshape(S, H, L, hd).transpose(0, 2, 1, 3).reshape(S, L, H * hd)


def _routed(I, nq, nk, hd, kind, bwd, seed, R=None, shared=None):
    """Items and their reference: build_items + reference (+ assert_edges), or build_graded + reference_graded."""
    if kind == 'graded':
        assert not bwd, 'graded cases are forward only'
        it = build_graded(I, nq, nk, hd, seed, R=R, shared=shared)
        return it, reference_graded(it)
    it = build_items(I, nq, nk, hd, kind, bwd, seed, R=R, shared=shared)
    r = reference(it)
    if bwd:
        assert_edges(it, r)
    return it, r


def _graded_fields(c, r, place, lse_shape):
    """Graded case: out_abs / out_n (the operands of value_bounds, laid out as out by `place`), log2l and top (as lse)."""
    c.out_abs, c.out_n = place(r['O_abs'].numpy()), place(r['O_n'].numpy())
    c.log2l, c.top = r['log2l'].numpy().reshape(lse_shape), r['top'].numpy().reshape(lse_shape)


def contig_case(S, L, H, kind='exact', bwd=True, seed=0, hd=64):
    it, r = _routed(S * H, L, L, hd, kind, bwd, seed)
    c = Case()
    c.layout, c.S, c.L, c.H, c.hd, c.kind, c.bwd, c.items, c.ref = 'contig', S, L, H, hd, kind, bwd, it, r
    c.scale = SCALE_GRADED if kind == 'graded' else SCALE
    c.B, c.T, c.P, c.cls_group = 0, 0, 0, 0
    D = H * hd
    c.qkv = np.concatenate([_sh(it.Q, S, H, L, hd), _sh(it.K, S, H, L, hd), _sh(it.V, S, H, L, hd)], 2).reshape(S * L, 3 * D)
    c.dout = _sh(it.dO, S, H, L, hd).reshape(S * L, D)
    c.out = _sh(r['O'].numpy(), S, H, L, hd).reshape(S * L, D)
    c.lse = r['lse'].numpy().reshape(S, H, L)
    c.nwin = it.nwin.reshape(S, H, L)
    if kind == 'graded':
        _graded_fields(c, r, lambda a: _sh(a, S, H, L, hd).reshape(S * L, D), (S, H, L))
    if bwd:
        for key in ('', '_abs', '_n'):
            c.__dict__['dqkv' + key] = np.concatenate(
                [_sh(r[n + key].numpy(), S, H, L, hd) for n in ('dq', 'dk', 'dv')], 2).reshape(S * L, 3 * D)
    return c


def layout_rows(mode, B, T, P):
    """in_row / out_row of vtx_attn (attn_common.h) as [S, L] int arrays, for the layouts that read qkv in the natural token
    order [B, 1 + P T, 3D]: 'space' (s = (b, t), L = 1 + P), 'time_cls' (s = (b, p), L = 1 + T), 'space_nocls' (s = (b, t),
    L = P)."""
    S, L = {'space': (B * T, P + 1), 'time_cls': (B * P, T + 1), 'space_nocls': (B * T, P)}[mode]
    s = np.arange(S)[:, None]
    i = np.arange(L)[None, :]
    rpc = 1 + P * T
    if mode == 'time_cls':
        b = s // P
        return np.where(i == 0, b * rpc, s * T + b + i), np.where(i == 0, B * P * T + s, s * T + i - 1)
    b, t = s // T, s % T
    if mode == 'space_nocls':
        return b * rpc + 1 + i * T + t, b * P * T + i * T + t
    rin = np.where(i == 0, b * rpc, b * rpc + 1 + (i - 1) * T + t)
    rout = np.where(i == 0, B * P * T + s, b * P * T + (i - 1) * T + t)
    return rin, rout


def space_rows(B, T, P):
    return layout_rows('space', B, T, P)


def _layout_case(layout, B, T, P, H, kind, bwd, seed, hd):
    """A case of one of layout_rows' layouts.  Where the sequences of a clip share its cls row ('space': the T frames,
    'time_cls': the P patch positions) the row's code, Q, K and V are drawn once per (clip, head); 'space_nocls' has no shared
    row: its items are contig_case's, the cls rows of qkv stay NaN (no kernel may read them) and the cls rows of the
    expected dqkv are zeros."""
    rin, rout = layout_rows(layout, B, T, P)
    S, L = rin.shape
    D = H * hd
    cls_group = {'space': T, 'time_cls': P, 'space_nocls': 0}[layout]
    if cls_group:
        R = routing_dims(int(math.ceil(L / 1.3)) + 2)
        sh = shared_rows_graded(B * H, hd, R, seed + 1) if kind == 'graded' else shared_rows(B * H, hd, R, kind, bwd, seed + 1)
        # item n = s * H + h uses the shared rows of (b, h), b = s // cls_group
        idx = (np.arange(S)[:, None] // cls_group * H + np.arange(H)[None, :]).reshape(-1)
        it, r = _routed(S * H, L, L, hd, kind, bwd, seed, R=R, shared={k: v[idx] for k, v in sh.items()})
    else:
        it, r = _routed(S * H, L, L, hd, kind, bwd, seed)
    c = Case()
    c.scale = SCALE_GRADED if kind == 'graded' else SCALE
    c.layout, c.S, c.L, c.H, c.hd, c.B, c.T, c.P, c.kind, c.bwd, c.items, c.ref = \
        layout, S, L, H, hd, B, T, P, kind, bwd, it, r
    c.cls_group = cls_group
    rows, orows = B * (1 + P * T), B * P * T + (S if cls_group else 0)
    c.cls_rows = np.arange(B) * (1 + P * T)
    c.qkv = np.full((rows, 3 * D), np.nan)
    for j, a in enumerate((it.Q, it.K, it.V)):
        c.qkv[rin.reshape(-1), j * D:(j + 1) * D] = _sh(a, S, H, L, hd).reshape(S * L, D)
    assert np.isnan(c.qkv).any(1).sum() == (0 if cls_group else B)
    c.dout = np.zeros((orows, D))
    c.dout[rout.reshape(-1)] = _sh(it.dO, S, H, L, hd).reshape(S * L, D)
    c.out = np.zeros((orows, D))
    c.out[rout.reshape(-1)] = _sh(r['O'].numpy(), S, H, L, hd).reshape(S * L, D)
    c.lse = r['lse'].numpy().reshape(S, H, L)
    c.nwin = it.nwin.reshape(S, H, L)
    if kind == 'graded':
        def place(a):
            full = np.zeros((orows, D))
            full[rout.reshape(-1)] = _sh(a, S, H, L, hd).reshape(S * L, D)
            return full
        _graded_fields(c, r, place, (S, H, L))
    if bwd:
        i0 = 1 if cls_group else 0
        for key in ('', '_abs', '_n'):
            full = np.concatenate([_sh(r[n + key].numpy(), S, H, L, hd) for n in ('dq', 'dk', 'dv')], 2)   # [S, L, 3D]
            d = np.full((rows, 3 * D), np.nan if cls_group else 0.0)
            d[rin[:, i0:].reshape(-1)] = full[:, i0:].reshape(-1, 3 * D)
            c.__dict__['dqkv' + key] = d
            if cls_group:
                c.__dict__['dqkv_cls' + key] = full[:, 0].copy()
    return c


def space_case(B, T, P, H, kind='exact', bwd=True, seed=0, hd=64):
    """VTX_ATTN_SPACE."""
    return _layout_case('space', B, T, P, H, kind, bwd, seed, hd)


def time_cls_case(B, T, P, H, kind='exact', bwd=True, seed=0, hd=64):
    """VTX_ATTN_TIME_CLS: sequence s = (b, p) of L = 1 + T rows whose row 0 is the cls row that the P sequences of clip b
    share."""
    return _layout_case('time_cls', B, T, P, H, kind, bwd, seed, hd)


def space_nocls_case(B, T, P, H, kind='exact', bwd=True, seed=0, hd=64):
    """VTX_ATTN_SPACE_NOCLS: sequence s = (b, t) of the L = P token rows of frame t."""
    return _layout_case('space_nocls', B, T, P, H, kind, bwd, seed, hd)


def cross_case(B, Lq, Lk, heads, hd, kind='exact', bwd=True, seed=0):
    it, r = _routed(B * heads, Lq, Lk, hd, kind, bwd, seed)
    c = Case()
    c.layout, c.B, c.Lq, c.Lk, c.H, c.hd, c.kind, c.bwd, c.items, c.ref = 'cross', B, Lq, Lk, heads, hd, kind, bwd, it, r
    c.scale = SCALE_GRADED if kind == 'graded' else SCALE
    c.q = _sh(it.Q, B, heads, Lq, hd)
    c.k = _sh(it.K, B, heads, Lk, hd)
    c.v = _sh(it.V, B, heads, Lk, hd)
    c.dout = _sh(it.dO, B, heads, Lq, hd)
    c.out = _sh(r['O'].numpy(), B, heads, Lq, hd)
    c.lse = r['lse'].numpy().reshape(B, heads, Lq)
    c.nwin = it.nwin.reshape(B, heads, Lq)
    if kind == 'graded':
        _graded_fields(c, r, lambda a: _sh(a, B, heads, Lq, hd), (B, heads, Lq))
    if bwd:
        for key in ('', '_abs', '_n'):
            c.__dict__['dq' + key] = _sh(r['dq' + key].numpy(), B, heads, Lq, hd)
            c.__dict__['dk' + key] = _sh(r['dk' + key].numpy(), B, heads, Lk, hd)
            c.__dict__['dv' + key] = _sh(r['dv' + key].numpy(), B, heads, Lk, hd)
    return c


# ------------------------------------------------------------------------------------------------ expectations
def expect(name, v, dtype, kind='round'):
    """Expected stored output of an exact float64 value: fp32 itself, bf16 RNE.  kind 'exact' also asserts the values are
    bf16-representable, and so does 'graded'; 'round' asserts the tie / inexact shares of exact.expect_bf16; None only the
    fp32 premise."""
    v = torch.as_tensor(v).double()
    kind = 'exact' if kind == 'graded' else kind
    if dtype == torch.float32:
        X.assert_fp32_exact(name, v)
        return v.float()
    if kind is None:
        X.assert_fp32_exact(name, v)
        return X.rne_bf16(v)
    return X.expect_bf16(name, v, kind)


ULP_BOUND = 2.0 ** -24


def value_bounds(exact, abs_sum, nterms):
    """Interval for a VALU result whose P carries the lse error: |got - exact| <= (8 + n) 2^-24 sum|terms| per element (8 units
    for the exp / lse error and two product roundings of each term, one per addition of n terms)."""
    exact = torch.as_tensor(exact).double()
    b = (8.0 + torch.as_tensor(nterms).double()) * ULP_BOUND * torch.as_tensor(abs_sum).double()
    return exact - b, exact + b, b


def within(got, lo, hi, dtype):
    """Mask of elements of got (CPU) inside [lo, hi] as stored in dtype: fp32 compares in float64; bf16 compares with
    RNE(lo) .. RNE(hi) (RNE is monotonic, so the store of any fp32 value in [lo, hi] lies there)."""
    g = got.double()
    if dtype == torch.float32:
        return (g >= lo) & (g <= hi)
    return (g >= X.rne_bf16(lo).double()) & (g <= X.rne_bf16(hi).double())


def lse_ok(got, nwin, ulps=4):
    """lse: exactly 0 for one winner, within `ulps` fp32 ulps of k ln2 for 2^k winners."""
    got = got.double()
    want = torch.log(torch.as_tensor(nwin).double())
    ulp = torch.where(want > 0, 2.0 ** (torch.floor(torch.log2(want.clamp(min=1e-30))) - 23), torch.zeros_like(want))
    return torch.where(want == 0, got == 0, (got - want).abs() <= ulps * ulp)


def lse_graded_ok(got, log2l, top, ulps=4, top_ulps=2):
    """lse of a graded case against (k - top) ln 2, k = log2 l: within `ulps` fp32 ulps at |k ln 2| (lse_ok's bar: the error of
    log l) plus `top_ulps` fp32 ulps at |top ln 2| (the rounded constant in the product (m c2) LN2, which is otherwise exact
    for top = 1, 2, and the final sum); exactly 0 where k = top = 0."""
    got = got.double()
    k, top = torch.as_tensor(log2l).double(), torch.as_tensor(top).double()

    def ulp(x):
        return torch.where(x > 0, 2.0 ** (torch.floor(torch.log2(x.clamp(min=1e-30))) - 23), torch.zeros_like(x))
    bar = ulps * ulp(k * LN2) + top_ulps * ulp(top * LN2)
    return (got - (k - top) * LN2).abs() <= bar


def probs_ok(got, want, ulps=2):
    """Probabilities: zeros exact, 2^-k within `ulps` fp32 ulps (2^-k is a power of two: its ulp above is 2^-k-23)."""
    got, want = got.double(), torch.as_tensor(want).double()
    return torch.where(want == 0, got == 0, (got - want).abs() <= ulps * want * 2.0 ** -23)
