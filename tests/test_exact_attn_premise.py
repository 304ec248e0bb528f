"""CPU checks of the routed-score attention cases (tests/exact_attn.py): the premise of every case table that
test_gpu_exact_attention.py and test_gpu_exact_attn_layouts.py use, exact_attn.layout_rows against the row addressing that
include/vtx.h states, and that the exact comparison rejects the attention faults a float64 tolerance check lets through.
Faults are emulated in float64 (a dense softmax over the key set the faulty kernel would see) and stored
as the kernels store them (float64 -> float32 -> RNE bf16)."""
import math

import numpy as np
import pytest
import torch

import exact as X
import exact_attn as A
import test_gpu_exact_attn_layouts as G
from helpers import relerr, report

OUT_BAR, GRAD_BAR = 1e-2, 2e-2       # the relerr bars test_gpu_kernels.py holds bf16 attention outputs / gradients to


def test_routing_premises():
    """Every case the GPU file builds satisfies its premise (the builders assert it: 2^k winners of score 0 per query,
    losers <= -T_NEG, fp32-exact partial sums, bf16-representable P, dS, dS * scale and O in backward cases, >= 50 % of the
    keys winners, every tile-edge key and the last key a winner with non-zero dS; round cases >= 20 % ties)."""
    for S, L, H in ((37, 1, 5), (37, 5, 5), (37, 8, 5), (37, 9, 5), (37, 17, 5), (37, 32, 5), (3, 33, 3), (3, 65, 3),
                    (3, 130, 3), (3, 193, 3), (3, 197, 3), (3, 224, 3), (3, 256, 3), (5, 33, 3), (5, 130, 3), (5, 197, 3),
                    (4, 197, 3), (4, 37, 3), (4, 256, 3), (37, 8, 2), (3, 37, 2), (3, 130, 2), (3, 300, 2)):
        c = A.contig_case(S, L, H)
        A.expect('out', c.out, torch.bfloat16, 'exact')
    for B, T, P in ((2, 3, 8), (2, 3, 36), (2, 3, 196)):
        A.space_case(B, T, P, 2)
    for args in ((37, 8, 5), (3, 130, 3), (3, 197, 3)):
        A.expect('round', A.contig_case(*args, kind='round', bwd=False).out, torch.bfloat16, 'round')
    A.expect('round', A.space_case(2, 3, 36, 2, 'round', False).out, torch.bfloat16, 'round')
    for hd in (64, 96):
        A.cross_case(2, 300, 37, 2, hd)
        A.cross_case(1, 2500, 393, 2, hd)
        A.expect('round', A.cross_case(2, 300, 37, 2, hd, 'round', False).out, torch.bfloat16, 'round')
    # test_gpu_cls_order.py and every case of test_gpu_exact_attn_layouts.py (time_cls at L = 3 among them: three keys, two
    # of them required, one partition that serves), and space at P = 2
    for T, P in ((8, 7), (16, 5)):
        A.time_cls_case(3, T, P, 5)
    A.space_case(2, 3, 2, 2)
    assert {k[:4] for k in G.CASES} >= {('time_cls', 3, 2, 7), ('space_nocls', 3, 4, 1), ('space_nocls', 2, 3, 196)}
    for key in sorted(G.CASES):
        c = G.build(key)
        assert (c.layout, c.B, c.T, c.P, c.H, c.kind, c.bwd) == key
        assert c.cls_group == {'space': c.T, 'time_cls': c.P, 'space_nocls': 0}[c.layout]
        A.expect(str(key), c.out, torch.bfloat16, c.kind)


def test_routing_premise_bench_scale():
    """The bench-scale cases of the streamed kernels (840 and 1152 items) and of the fused backward on space_nocls (576)."""
    A.contig_case(70, 197, 12)
    A.space_case(6, 8, 196, 12)
    assert G.BENCH_CASES
    for key in sorted(G.BENCH_CASES):
        G.build(key)


LAYOUT_SHAPES = ((2, 3, 5), (3, 4, 2), (2, 1, 7))


@pytest.mark.parametrize('mode', ['space', 'time_cls', 'space_nocls'])
def test_layout_rows_cover_every_row_once(mode):
    for B, T, P in LAYOUT_SHAPES:
        rin, rout = A.layout_rows(mode, B, T, P)
        rpc = 1 + P * T
        share = {'space': T, 'time_cls': P, 'space_nocls': 0}[mode]
        S, L = {'space': (B * T, P + 1), 'time_cls': (B * P, T + 1), 'space_nocls': (B * T, P)}[mode]
        assert rin.shape == rout.shape == (S, L)
        want = np.ones(B * rpc, np.int64)
        want[np.arange(B) * rpc] = share            # the cls row: once per sequence that shares it; never for space_nocls
        assert np.array_equal(np.bincount(rin.reshape(-1), minlength=B * rpc), want), (mode, B, T, P)
        out_rows = B * P * T + (S if share else 0)
        assert np.array_equal(np.bincount(rout.reshape(-1), minlength=out_rows), np.ones(out_rows, np.int64)), (mode, B, T, P)
        if share:                                   # the sequences that share a cls row are those of one clip, in order
            assert np.array_equal(rin[:, 0], np.repeat(np.arange(B) * rpc, share))
            assert np.array_equal(rout[:, 0], B * P * T + np.arange(S))


def test_layout_rows_are_the_rows_of_the_header():
    """include/vtx.h, written out with loops: qkv is [B, 1 + P T, 3D] with tokens in (p t) order; out holds the token rows
    clip-major in (p t) order, then (space, time_cls) one cls row per sequence."""
    for B, T, P in LAYOUT_SHAPES:
        rpc, N = 1 + P * T, P * T
        for mode in ('space', 'time_cls', 'space_nocls'):
            rin, rout = A.layout_rows(mode, B, T, P)
            for b in range(B):
                clip_in, clip_out = b * rpc, b * N
                if mode == 'time_cls':
                    for p in range(P):
                        s = b * P + p
                        assert rin[s, 0] == clip_in and rout[s, 0] == B * N + s
                        for i in range(1, T + 1):           # row 1 + p T + (i - 1) of clip b: frame i - 1 of patch p
                            assert rin[s, i] == clip_in + 1 + p * T + (i - 1)
                            assert rout[s, i] == clip_out + p * T + (i - 1)
                    continue
                for t in range(T):
                    s = b * T + t
                    if mode == 'space':
                        assert rin[s, 0] == clip_in and rout[s, 0] == B * N + s
                        for i in range(1, P + 1):           # token 1 + (i - 1) T + t: patch i - 1 of frame t
                            assert rin[s, i] == clip_in + 1 + (i - 1) * T + t
                            assert rout[s, i] == clip_out + (i - 1) * T + t
                    else:
                        for i in range(P):                  # row 1 + i T + t: patch i of frame t
                            assert rin[s, i] == clip_in + 1 + i * T + t
                            assert rout[s, i] == clip_out + i * T + t


def test_premise_rejects_broken_routing():
    it = A.build_items(2, 9, 9, 64, 'exact', True, 0)
    it.K[0, 3, :it.R] = 0.0                    # a key without a code scores 0 with every query
    with pytest.raises(AssertionError):
        A.reference(it)
    it = A.build_items(2, 9, 9, 64, 'exact', True, 0)
    it.V[0, :, 0] = 257.0                      # O = 257: not bf16-representable, which a backward case needs
    with pytest.raises(AssertionError):
        A.reference(it)


def _dense_out(Q, K, V, scale=A.SCALE):
    """float64 softmax(Q K^T scale) V of one item over whatever key set a faulty kernel sees."""
    s = Q @ K.T * scale
    p = np.exp(s - s.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)) @ V


def _item_out(c, fn):
    """[I, nq, hd] of fn(n) -> (Q, K, V) per item."""
    return np.stack([_dense_out(*fn(n)) for n in range(c.items.I)])


def _verdict(name, got_bf16, want_bf16, exact, bar):
    nbad = int(X.mismatch(got_bf16, want_bf16).sum())
    e = relerr(got_bf16.double(), torch.as_tensor(exact).double())
    report(f'ok   exact-sensitivity [attention] {name}: rejected ({nbad} elements differ); tolerance metric {e:.2e} vs bar '
           f'{bar:g}: the old check would have {"PASSED" if e <= bar else "failed"} it')
    assert nbad > 0, f'fault "{name}" passes the exact comparison'
    return e


def _trunc_bf16(v):
    return (torch.as_tensor(v).float().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)


def _gathered_out(qkv, hd, rq, rkv, pad=0):
    """[S, L, hd] float64 outputs of a one-head kernel that gathers the query of (s, i) from row rq[s, i] of qkv [rows, 3 hd]
    and its key / value from row rkv[s, i], with `pad` unmasked zero rows after the keys."""
    z = np.zeros((pad, hd))
    return np.stack([_dense_out(qkv[q, :hd], np.vstack([qkv[k, hd:2 * hd], z]), np.vstack([qkv[k, 2 * hd:], z]))
                     for q, k in zip(rq, rkv)])


def _layout_addressing_faults():
    """Addressing faults of VTX_ATTN_TIME_CLS and VTX_ATTN_SPACE_NOCLS, one head (so a row of qkv is q | k | v of one item).
    The outputs land where they belong; the operands come from the rows the faulty kernel would compute."""
    # ---- time_cls: B = 2 clips of P = 3 sequences, L = 1 + 8
    c = A.time_cls_case(2, 8, 3, 1)
    hd, rpc = c.hd, 1 + c.P * c.T
    rin, _ = A.layout_rows('time_cls', c.B, c.T, c.P)
    b = np.arange(c.S)[:, None] // c.P
    want, exact = X.rne_bf16(c.ref['O']), c.ref['O']
    clean = lambda got, ref: not X.mismatch(X.rne_bf16(torch.from_numpy(got)), ref).any()          # noqa: E731
    assert clean(_gathered_out(c.qkv, hd, rin, rin), want)            # the emulation itself, without a fault
    bad = rin.copy()
    bad[:, 1:] -= b                                                   # s T + i instead of s T + b + i
    got = _gathered_out(c.qkv, hd, bad, bad)
    assert clean(got[:c.P], want[:c.P])                               # clip 0 has no offset to lose
    _verdict('time_cls: token rows without the clip offset (clips b >= 1)', X.rne_bf16(torch.from_numpy(got)), want, exact,
             OUT_BAR)
    bad = rin.copy()
    bad[:, 0] = np.maximum(b[:, 0] - 1, 0) * rpc                      # the cls key / value of clip b - 1
    _verdict('time_cls: cls key taken from clip b - 1', X.rne_bf16(torch.from_numpy(_gathered_out(c.qkv, hd, rin, bad))),
             want, exact, OUT_BAR)
    # the per-sequence cls gradient of (b, p) stored in the row of (b, p + 1): what vtx_cls_qkv_reduce folds is unchanged
    W = 3 * hd
    good = c.dqkv_cls.reshape(c.B, c.P, W)
    moved = np.roll(good, 1, axis=1)
    assert np.array_equal(moved.sum(1), good.sum(1)), 'the reduced cls row sees the fault'
    _verdict('time_cls: dqkv_cls row of sequence s written to row s + 1 (reduced row unchanged)',
             X.rne_bf16(torch.from_numpy(moved.reshape(c.S, W))), X.rne_bf16(torch.from_numpy(c.dqkv_cls)),
             torch.from_numpy(c.dqkv_cls), GRAD_BAR)
    # ---- space_nocls: B = 2 clips of T = 3 frames, P = 16.  The cls rows of the case are NaN; a model's hold data, so here
    # they hold a copy of the clip's last token row (routed like every other row)
    c = A.space_nocls_case(2, 3, 16, 1)
    hd, rpc = c.hd, 1 + c.P * c.T
    rin, _ = A.layout_rows('space_nocls', c.B, c.T, c.P)
    qkv = c.qkv.copy()
    qkv[c.cls_rows] = qkv[c.cls_rows + rpc - 1]
    want, exact = X.rne_bf16(c.ref['O']), c.ref['O']
    assert clean(_gathered_out(qkv, hd, rin, rin), want)
    got = _gathered_out(qkv, hd, rin - 1, rin - 1)                    # i T + t: the cls row is token 0 of frame 0
    _verdict('space_nocls: rows without the + 1 that skips the cls row', X.rne_bf16(torch.from_numpy(got)), want, exact,
             OUT_BAR)
    s = np.arange(c.S)[:, None]
    i = np.arange(c.L)[None, :]
    bad = s // c.T * rpc + 1 + i * (c.T + 1) + s % c.T                 # stride T + 1
    first = slice(0, c.T)                                             # clip 0: its overrun stays inside the buffer (clip 1)
    assert bad[first].max() < c.qkv.shape[0]
    got = _gathered_out(qkv, hd, bad[first], bad[first])
    _verdict('space_nocls: rows read with stride T + 1', X.rne_bf16(torch.from_numpy(got)), want[first], exact[first],
             OUT_BAR)
    got = _gathered_out(qkv, hd, rin, rin, pad=32 - c.P)
    _verdict('space_nocls: the 32 - P zero pad rows of the single tile unmasked', X.rne_bf16(torch.from_numpy(got)), want,
             exact, OUT_BAR)


def test_check_exact_rejects_attention_faults():
    """Each emulated kernel fault is rejected by the exact comparison; its float64 tolerance metric is reported next to the
    bar of the old tests (not asserted: it is the gap these tests close)."""
    bf = torch.bfloat16
    # an unmasked zero-filled padded key: L = 197, the ragged tile holds 27 zero rows that score 0
    c = A.contig_case(3, 197, 2, seed=5)
    it = c.items
    npad = 224 - 197
    z = np.zeros((npad, it.hd))
    bad = _item_out(c, lambda n: (it.Q[n], np.vstack([it.K[n], z]), np.vstack([it.V[n], z])))
    want = X.rne_bf16(c.ref['O'])
    _verdict('forward: padded keys unmasked (L = 197)', X.rne_bf16(torch.from_numpy(bad)), want, c.ref['O'], OUT_BAR)
    # stale K / V rows of the previous item in the pad rows of a persistent kernel, unmasked
    bad = _item_out(c, lambda n: (it.Q[n], np.vstack([it.K[n], it.K[n - 1][:npad]]), np.vstack([it.V[n], it.V[n - 1][:npad]])))
    _verdict('forward: stale rows of the previous item in the pad rows', X.rne_bf16(torch.from_numpy(bad)), want,
             c.ref['O'], OUT_BAR)
    # a key of the neighbouring sequence inside a packed 32-row tile (L = 8: four sequences per tile, one head)
    c = A.contig_case(37, 8, 1)
    it = c.items

    def neighbour(n):                                   # the tile's next sequence leaks its first key
        m = n + 1 if n % 4 != 3 and n + 1 < it.I else n - 1
        return it.Q[n], np.vstack([it.K[n], it.K[m][:1]]), np.vstack([it.V[n], it.V[m][:1]])
    bad = _item_out(c, neighbour)
    _verdict('packed tile: a key of the neighbouring sequence', X.rne_bf16(torch.from_numpy(bad)),
             X.rne_bf16(c.ref['O']), c.ref['O'], OUT_BAR)
    # space mode: token keys read with the frame stride off by one (frame t + 1 instead of t; the cls key is right)
    c = A.space_case(2, 3, 36, 1)
    it = c.items
    T = c.T

    def stride(n):
        b, t = divmod(n, T)
        m = b * T + (t + 1) % T
        return it.Q[n], np.vstack([it.K[n][:1], it.K[m][1:]]), np.vstack([it.V[n][:1], it.V[m][1:]])
    bad = _item_out(c, stride)
    _verdict('space mode: frame stride off by one', X.rne_bf16(torch.from_numpy(bad)), X.rne_bf16(c.ref['O']),
             c.ref['O'], OUT_BAR)
    _layout_addressing_faults()
    # backward faults on L = 197: the last key tile dropped from dk / dv; a dS mask one row early drops the last real key
    c = A.contig_case(3, 197, 2, seed=5)
    it, r = c.items, c.ref
    for key in ('dk', 'dv'):
        bad = r[key].clone()
        bad[:, 192:] = 0.0
        _verdict(f'backward: last key tile dropped from {key}', X.rne_bf16(bad), X.rne_bf16(r[key]), r[key], GRAD_BAR)
    last = it.nk - 1
    dS = r['dS'].numpy()
    hit = (it.win == last) * dS                                           # [I, nq, 4]: dS of the last key
    bad = r['dq'] - torch.from_numpy(A.SCALE * hit.sum(2)[..., None] * it.K[:, last][:, None, :])
    _verdict('backward: dS mask one row early (last key dropped from dq)', X.rne_bf16(bad), X.rne_bf16(r['dq']), r['dq'],
             GRAD_BAR)
    # lse in log2 units instead of natural log
    lse2 = torch.log2(r['nwin'].double())
    ok = A.lse_ok(lse2.float(), r['nwin'])
    e = relerr(lse2, r['lse'])
    report(f'ok   exact-sensitivity [attention] lse in log2 units: rejected ({int((~ok).sum())} elements outside 4 ulps); '
           f'tolerance metric {e:.2e} vs bar {OUT_BAR:g}: the old check would have {"PASSED" if e <= OUT_BAR else "failed"} it')
    assert not ok.all()
    # a truncating bf16 store: visible on the round cases only (exact-range outputs are representable)
    c = A.contig_case(3, 197, 3, kind='round', bwd=False)
    want = A.expect('round', c.out, bf, 'round')
    _verdict('truncating bf16 store of O (round case)', _trunc_bf16(torch.from_numpy(c.out)), want,
             torch.from_numpy(c.out), OUT_BAR)
    c = A.contig_case(3, 197, 2, seed=5)
    assert not X.mismatch(_trunc_bf16(c.ref['O']), X.rne_bf16(c.ref['O'])).any()


def test_bounds_and_lse_helpers():
    lo, hi, b = A.value_bounds(torch.tensor([0.0, 1.0, 3.0]), torch.tensor([0.0, 4.0, 4.0]), torch.tensor([0.0, 2.0, 2.0]))
    assert b[0] == 0 and b[1] == 10 * 4 * 2.0 ** -24
    got = torch.tensor([0.0, 1.0 + 2.0 ** -22, 3.0 - 2.0 ** -17], dtype=torch.float32)
    assert A.within(got, lo, hi, torch.float32).tolist() == [True, True, False]
    assert A.within(got.to(torch.bfloat16), lo, hi, torch.bfloat16).all()
    nwin = torch.tensor([1, 2, 4, 2])
    lse = torch.tensor([0.0, math.log(2), math.log(4), math.log(2) + 5 * 2.0 ** -24], dtype=torch.float32)
    assert A.lse_ok(lse, nwin).tolist() == [True, True, True, False]
    assert A.probs_ok(torch.tensor([0.0, 0.5, 0.25 * (1 + 2.0 ** -23), 1e-30]),
                      torch.tensor([0.0, 0.5, 0.25, 0.0])).tolist() == [True, True, True, False]
