"""CPU checks of the graded attention cases (tests/exact_attn.py: kind 'graded') and of the case tables of
tests/test_gpu_attn_graded.py and tests/test_gpu_attn_hd_layouts.py.

  1. the premise of the graded scale: c2 = fl32(scale) * fl32(log2 e) is exactly 2^-3 in float32, for fl32(ln 2) / 2^k at every
     k = 0..5, and for neither fp32 neighbour of fl32(ln 2);
  2. every case of the two GPU modules builds (the builders assert the rest: winners score -8 (grade + top), losers' exponents
     <= -150, every output bf16-representable, at least 8 queries per chunk boundary and item whose maximum rises across it);
  3. the existing kinds are unchanged: a hash of the inputs and expectations of a few cases, computed before 'graded' existed;
  4. a numpy emulation of the chunked forward (fp32 throughout, P packed to bf16, the chunk size a parameter) passes every
     graded contig case, and fails each of them once a fault is put into the rescale; the 'exact' kind passes under two of the
     three faults, which is the gap the graded kind closes.
"""
import hashlib

import numpy as np
import pytest
import torch

import exact as X
import exact_attn as A
import test_gpu_attn_graded as G
import test_gpu_attn_hd_layouts as HL

f32 = np.float32


# ------------------------------------------------------------------------------------------------ 1. the scale
def test_c2_is_exactly_an_eighth():
    ln2 = f32(np.log(2.0))
    assert f32(A.SCALE_GRADED) == ln2 / f32(8) and float(f32(A.SCALE_GRADED)) == A.SCALE_GRADED
    assert abs(A.SCALE_GRADED - 0.0866434) < 1e-7
    assert A.LOG2E_F32 == f32(1.4426950408889634)
    assert f32(A.SCALE_GRADED) * A.LOG2E_F32 == f32(0.125)
    for k in range(6):
        assert (ln2 / f32(2 ** k)) * A.LOG2E_F32 == f32(2.0 ** -k)
    for neighbour in (np.nextafter(ln2, f32(0)), np.nextafter(ln2, f32(1))):      # the value has to be pinned
        assert neighbour * A.LOG2E_F32 != f32(1)
    assert f32(0.6931471805599453) == ln2                                         # LN2 of the kernels' lse


# ------------------------------------------------------------------------------------------------ 2. the case tables
def test_graded_cases_build():
    """Every case of test_gpu_attn_graded.py; the table holds the smallest shapes that cross a block of each forward: contig
    L = 129 and 256, 257 and 385, 65 / 129 / 257 at 32, 96, 128; the four layouts; cross attention at head_dim 64 and 96."""
    keys = {k[:2] + k[3:] for k in G.CASES}
    assert keys >= {('contig', (2, 129), 64), ('contig', (2, 256), 64), ('space', (2, 2, 196), 64), ('time_cls', (2, 129, 2), 64),
                    ('space_nocls', (2, 2, 130), 64), ('contig', (2, 257), 64), ('contig', (2, 385), 64), ('space', (1, 2, 300), 64),
                    ('cross', (2, 40, 129), 64), ('cross', (1, 70, 393), 96)}
    for hd in (32, 96, 128):
        assert keys >= {('contig', (2, 65), hd), ('contig', (2, 129), hd), ('contig', (2, 257), hd), ('space', (1, 2, 64), hd),
                        ('time_cls', (1, 64, 3), hd), ('space_nocls', (1, 2, 65), hd)}
    for key in sorted(G.CASES):
        c = G.build(key)
        it = c.items
        assert c.kind == 'graded' and not c.bwd and c.scale == A.SCALE_GRADED and c.H in (2, 3)
        A.expect(str(key), c.out, torch.bfloat16, 'graded')                       # representable in bf16
        bounds = A.chunk_bounds(it.nk)
        assert bounds and bounds == [b for b in range(64, it.nk, 64)]             # every case crosses a chunk
        counts = A.straddle_counts(it)
        for b in bounds:
            assert counts[b].shape == (it.I,) and counts[b].min() >= 8, (key, b, counts[b].min())
        assert set(np.unique(it.top)) == {0, 1, 2}                                # the final maximum is not always 0
        assert set(np.unique(c.lse / A.LN2).round().astype(int)) == {-2, -1, 0, 1}
        if getattr(c, 'cls_group', 0):                                            # the shared cls row: one draw per (clip, head)
            grp = c.cls_group
            for a in (it.grade[:, 0], it.top[:, 0], it.kcode[:, 0], it.qcode[:, 0]):
                a = a.reshape(c.S // grp, grp, c.H)
                assert (a == a[:, :1]).all()
            assert (c.qkv[c.cls_rows] == c.qkv[c.cls_rows]).all()                 # no NaN: every cls row was written


def test_graded_shared_row_takes_both_grades():
    """Over the cases with a shared cls row, key 0 carries grade 0 in some (clip, head) pairs and grade 2 in others."""
    g0 = np.concatenate([G.build(k).items.grade[:, 0] for k in sorted(G.CASES) if k[0] in ('space', 'time_cls')])
    assert set(np.unique(g0)) == {0, 2}


def test_hd_layout_cases_build():
    """Every case of test_gpu_attn_hd_layouts.py at head_dim 32 (the routing does not depend on the head dim; the round cases
    at all three: their share of ties does)."""
    assert len(HL.CASES) == 3 * (10 + 12 + 2)
    for key in sorted(HL.CASES):
        layout, dims, H, hd, kind, bwd = key
        if hd == 32 or kind == 'round':
            c = HL.build(key)
            assert c.L > 32 and c.scale == A.SCALE
            A.expect(str(key), c.out, torch.bfloat16, kind)


# ------------------------------------------------------------------------------------------------ 3. the old kinds
def _digest(c):
    names = ('q', 'k', 'v', 'dout', 'out', 'lse') if c.layout == 'cross' else ('qkv', 'dout', 'out', 'lse')
    if c.bwd:
        grads = ('dq', 'dk', 'dv') if c.layout == 'cross' else ('dqkv',) + (('dqkv_cls',) if c.cls_group else ())
        names += tuple(g + s for g in grads for s in ('', '_abs', '_n'))
    h = hashlib.sha256()
    for n in names:
        h.update(np.ascontiguousarray(getattr(c, n), dtype=np.float64).tobytes())
    return h.hexdigest()[:16]


PINNED = {                                                                        # computed at the commit before the graded kind
    'contig 3x130x3': (lambda: A.contig_case(3, 130, 3), '2b58322e1c923bbe'),
    'contig 2x129x2 hd32': (lambda: A.contig_case(2, 129, 2, hd=32), 'aba9298c6f9c94bc'),
    'contig 3x130x3 round': (lambda: A.contig_case(3, 130, 3, 'round', False), 'e47818a3e816e306'),
    'space 2,3,36 H2': (lambda: A.space_case(2, 3, 36, 2), '4cab19562e0aeb71'),
    'time_cls 2,32,3 H3': (lambda: A.time_cls_case(2, 32, 3, 3), 'cde39c2f9a0b4cb8'),
    'space_nocls 2,3,33 H3': (lambda: A.space_nocls_case(2, 3, 33, 3), '992660dc54b0a761'),
    'cross 2,300,37 H2 hd96': (lambda: A.cross_case(2, 300, 37, 2, 96), '631e613bc08d10db'),
}


@pytest.mark.parametrize('name', list(PINNED))
def test_existing_kinds_are_unchanged(name):
    make, want = PINNED[name]
    c = make()
    assert c.scale == A.SCALE == 0.125
    assert _digest(c) == want, f'{name}: the inputs or expectations of an existing case moved'


# ------------------------------------------------------------------------------------------------ 4. emulated faults
def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(torch.bfloat16).float().numpy()


def _exp2(x):
    """fp32 exp2 that flushes below the smallest normal, as the hardware instruction does"""
    x = x.astype(f32)
    with np.errstate(under='ignore'):
        return np.where(x < f32(-126), f32(0), np.exp2(np.maximum(x, f32(-200)))).astype(f32)


def emulate(Q, K, V, scale, chunk, fault=None):
    """The chunked forward of one item as the bf16 kernels state it, in fp32 numpy: returns (out as stored in bf16, lse).
    fault: None, 'alpha=1' (alpha replaced by 1 wherever it is not 0), 'l' (l not rescaled), 'no c2' (alpha = exp2(m - mn))."""
    c2 = f32(scale) * A.LOG2E_F32
    s = (Q @ K.T).astype(f32)                                  # integers below 2^24: exact
    assert np.array_equal(s.astype(np.float64), Q @ K.T)
    nq, nk = s.shape
    V = V.astype(f32)
    m, l, acc = np.full(nq, f32(-1e30)), np.zeros(nq, f32), np.zeros((nq, V.shape[1]), f32)
    for k0 in range(0, nk, chunk):
        st = s[:, k0:k0 + chunk]
        mn = np.maximum(m, st.max(1))
        alpha = _exp2(m - mn) if fault == 'no c2' else _exp2((m - mn) * c2)
        if fault == 'alpha=1':
            alpha = np.where(alpha != 0, f32(1), alpha)
        mc = mn * c2
        e = _exp2((st.astype(np.float64) * np.float64(c2) - mc[:, None].astype(np.float64)).astype(f32))      # one rounding: the fma
        bl = e.sum(1, dtype=f32)
        l = l * (f32(1) if fault == 'l' else alpha) + bl
        acc = acc * alpha[:, None] + (_bf16(e).astype(np.float64) @ V[k0:k0 + chunk].astype(np.float64)).astype(f32)
        m = mn
    out = _bf16(acc * (f32(1) / l)[:, None])
    lse = (m * c2) * f32(A.LN2) + np.log(l.astype(np.float64)).astype(f32)
    return out, lse.astype(f32)


def _emulated_case_passes(c, chunk, fault):
    """Whether the emulation of every item of the contig case c meets the bf16 standard of the GPU tests: out equal, lse by
    lse_graded_ok (graded) or lse_ok."""
    it = c.items
    ok = True
    for n in range(it.I):
        out, lse = emulate(it.Q[n], it.K[n], it.V[n], c.scale, chunk, fault)
        want = c.ref['O'][n].numpy()
        ok &= np.array_equal(out.astype(np.float64), want)
        if c.kind == 'graded':
            ok &= bool(A.lse_graded_ok(torch.from_numpy(lse), c.ref['log2l'][n], c.ref['top'][n]).all())
        else:
            ok &= bool(A.lse_ok(torch.from_numpy(lse), it.nwin[n]).all())
    return ok


FAULTS = ('alpha=1', 'l', 'no c2')
GRADED_CONTIG = sorted(k for k in G.CASES if k[0] == 'contig')


def _chunks(L):
    return [ch for ch in (32, 64, 128) if ch < L]


@pytest.mark.parametrize('key', GRADED_CONTIG, ids=G._id)
def test_emulated_faults_fail_every_graded_contig_case(key):
    """At every chunk size in use (32 and 64: the fp32 policy and attn_hd.hip; 128: the others) the sound emulation passes the
    case, out and lse, and each fault fails it."""
    c = G.build(key)
    for chunk in _chunks(c.L):
        assert _emulated_case_passes(c, chunk, None), f'{key}: the emulation without a fault fails at chunk {chunk}'
        for fault in FAULTS:
            assert not _emulated_case_passes(c, chunk, fault), f'{key}: fault "{fault}" passes at chunk {chunk}'


def test_the_exact_kind_passes_under_two_of_the_faults():
    """The gap, written down: with every winner at score 0 alpha is 0 or 1, so replacing it by 1 where it is not 0, or leaving c2
    out of it, changes nothing that the 'exact' kind can see.  (Not rescaling l keeps the losers of a wiped chunk: seen.)"""
    for L, chunk in ((129, 64), (257, 128)):
        c = A.contig_case(2, L, 2, bwd=False, hd=32)
        assert _emulated_case_passes(c, chunk, None)
        assert _emulated_case_passes(c, chunk, 'alpha=1') and _emulated_case_passes(c, chunk, 'no c2')
        assert not _emulated_case_passes(c, chunk, 'l')


def test_lse_graded_ok():
    ln2 = A.LN2
    k = torch.tensor([0.0, 0.0, 1.0, 1.0, 1.0, 0.0])
    top = torch.tensor([0.0, 1.0, 0.0, 2.0, 1.0, 2.0])
    good = torch.tensor([0.0, -ln2, ln2, -ln2, 0.0, -2 * ln2], dtype=torch.float64)
    assert A.lse_graded_ok(good, k, top).all()
    ulp = 2.0 ** -24                                                                # of ln 2 (in [0.5, 1))
    assert A.lse_graded_ok(good + torch.tensor([0, 2, 4, 8, 6, 4]) * ulp * 0.99, k, top).all()
    bad = good + torch.tensor([1e-30, 3, 5, 9, 7, 5]) * ulp
    assert not A.lse_graded_ok(bad, k, top).any()
    assert not A.lse_graded_ok(good * 1.4426950408889634, k, top)[1:4].any()        # log2 units
    assert X.EXACT_LIMIT == 2 ** 24
