"""CPU checks of the routed-score attention cases (tests/exact_attn.py): the premise of every case table that
test_gpu_exact_attention.py uses, and that the exact comparison rejects the attention faults a float64 tolerance check
lets through.  Faults are emulated in float64 (a dense softmax over the key set the faulty kernel would see) and stored
as the kernels store them (float64 -> float32 -> RNE bf16)."""
import math

import numpy as np
import pytest
import torch

import exact as X
import exact_attn as A
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


def test_routing_premise_bench_scale():
    """The bench-scale cases of the streamed kernels (840 and 1152 items)."""
    A.contig_case(70, 197, 12)
    A.space_case(6, 8, 196, 12)


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
