"""CPU checks of the exact LayerNorm test machinery (tests/exact_ln.py): the premise of every case that
test_gpu_exact_layernorm.py runs, and that the new checks reject the kernel faults the float64 tolerance tests let through
(emulated on the CPU: float64 -> float32 -> RNE bf16, the arithmetic of the kernels)."""
import functools

import pytest
import torch

import exact as X
import exact_ln as L
from helpers import relerr, report

F32_BAR, BF16_BAR = 1e-3, 1e-2        # max|got - ref| / max|ref| bars of the tolerance tests of LayerNorm
ROWS = 24581                          # the largest row count of the backward tables: several trips of any backward grid
GRID = 1024                           # workgroups of the emulated backward launch (4 waves each, two rows per wave and trip)


def test_backward_case_premises():
    """The builders assert it: every intermediate fp32-exact on the exactly checked rows, column sums exact in any order,
    rounding cases >= 20 % ties and >= 40 % inexact."""
    for rows, D, kind, res in L.bwd_table():
        c = L.bwd_case(rows, D, kind, res, L.case_seed(rows, D))
        L.bwd_expected_dx(c)
        X.assert_fp32_exact(c['name'] + ' dgamma', c['dgamma'])
        X.assert_fp32_exact(c['name'] + ' dbeta', c['dbeta'])
        assert bool((c['dg0'] != 0).all()) and bool((c['db0'] != 0).all())
        if rows > 1:
            assert bool(c['mirrored'].any()) and not bool(c['mirrored'].all())
        if not L.is_pow2(D):       # the bound is far below the values it guards
            um = ~c['exact_rows']
            assert float((c['bound'][um] / c['dx'][um].abs().clamp_min(1.0)).max()) < 1e-4


def test_forward_case_premises():
    """Sums exact, mean exact, and bf16 y a rounding case with the float64 rstd standing in for the kernel's."""
    for rows, D, kind in L.fwd_table():
        c = L.fwd_case(rows, D, kind, L.case_seed(rows, D))
        L.fwd_expected_y(c, c['rstd'].float())
        X.assert_fp32_exact(c['name'] + ' mean', c['mean'])
        if kind in ('acc', 'acc0'):
            assert torch.equal(X.rne_bf16(c['d'].double()).float(), c['d']), 'd is bf16-representable'
            if c['xs'] is not None:
                assert torch.equal((c['xs'].double() + c['d'].double()).float(), c['x'])


def test_ulp_distance_and_tie_offsets():
    one = torch.tensor([1.0, 1.0, 0.75, 3.0], dtype=torch.float64)
    got = torch.tensor([1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 0.75 + 2.0 ** -22, 3.0])
    assert L.ulp_distance(got, one).tolist() == [1.0, 0.5, 4.0, 0.0]
    u = torch.tensor([0.125, -0.375, 1.0, 6.0, 0.0, -2.5])
    r = L.tie_offsets(u, 3)
    assert torch.equal(X.rne_bf16(r).double(), r), 'offsets are bf16 values'
    ties, _ = X.bf16_stats((u.double() + r)[u != 0])
    assert ties == 1.0
    assert L.half_bf16_ulp(torch.tensor([1.0, 300.0, 0.0], dtype=torch.float64)).tolist() == [2.0 ** -8, 1.0, 0.0]


# ------------------------------------------------------------------------------------------- fault emulation
@functools.lru_cache(maxsize=None)
def _case(D, kind):
    return L.bwd_case(ROWS, D, kind, True, L.case_seed(ROWS, D))


def _dx_of(c, c1, c2, with_res=True):
    """The backward formula in float64 with the given c1 / c2 ([rows, 1])."""
    v = c['rs'].double()[:, None] * (c['g'] - c1 - c['xh'] * c2)
    return v + c['dres'].double() if with_res else v


def _dgamma_of(c, weight):
    """dgamma / dbeta with row r counted weight[r] times."""
    w = weight.double()[:, None]
    return (c['dg0'].double() + (w * c['dy'].double() * c['xh']).sum(0), c['db0'].double() + (w * c['dy'].double()).sum(0))


def _grad_faults(c):
    """(name, dgamma, dbeta) of the faults in the row loop and the partial reduce."""
    rows, D = c['rows'], c['D']
    out = []
    r = int((c['dy'] != 0).sum(1).argmax())
    w = torch.ones(rows)
    w[r] = 0
    out.append(('one row missing', *_dgamma_of(c, w)))
    w[r] = 2
    out.append(('one row counted twice', *_dgamma_of(c, w)))
    trip = 2 * 4 * GRID
    w = (torch.arange(rows) < (rows // trip) * trip).float()
    assert 0 < rows - int(w.sum()) < trip
    out.append(('last ragged trip skipped', *_dgamma_of(c, w)))
    slab = (torch.arange(rows) % (4 * GRID)) // 4
    out.append(('slabs >= 128 dropped by the partial reduce', *_dgamma_of(c, (slab < 128).float())))
    both = torch.cat([c['dgamma'] - c['dg0'].double(), c['dbeta'] - c['db0'].double()])
    dg = c['dg0'].double().clone()
    dg[:D - 1] += both[:D - 1]
    out.append(('dgamma / dbeta split one column off', dg, c['db0'].double() + both[D - 1:2 * D - 1]))
    dg, db = c['dgamma'].clone(), c['dbeta'].clone()
    dg[D - 4:], db[D - 4:] = c['dg0'].double()[D - 4:], c['db0'].double()[D - 4:]
    out.append(('last 4-column group skipped', dg, db))
    return out


def test_gradient_faults_rejected():
    """dgamma / dbeta at 24 581 rows: every fault moves at least one element, which equality sees; the tolerance metric of
    each is reported next to the bars it is held to today.  On these cases (column sums of random sign, so max|ref| is only
    a few hundred) one row missing or counted twice measures 4.9e-3: the 1e-2 bar of the bf16 tests lets it through
    (asserted below), the 1e-3 bar of the fp32 ones catches it.  The skipped ragged trip measures 1.06e-2, at the edge of the 1e-2 bar, and
    is not asserted either way.  Dropped slabs, the split one column off and the skipped column group measure 0.7 ... 2.2:
    the old bars catch those whenever the path runs at all -- the wide reduce and D > 1024 did not."""
    c = _case(128, 'f32')
    want_g, want_b = c['dgamma'].float(), c['dbeta'].float()
    passes_old = {}
    for name, dg, db in _grad_faults(c):
        nbad = int(X.mismatch(dg.float(), want_g).sum()) + int(X.mismatch(db.float(), want_b).sum())
        e = max(relerr(dg, c['dgamma']), relerr(db, c['dbeta']))
        passes_old[name] = e <= BF16_BAR
        report(f'ok   exact-sensitivity [ln dgamma/dbeta] {name}: rejected ({nbad} elements differ); tolerance metric {e:.2e} '
               f'vs bars {F32_BAR:g} / {BF16_BAR:g}')
        assert nbad > 0, f'fault "{name}" passes the exact comparison'
    # a single row is what the bf16 bar cannot see (the sums of these cases cancel, so max|ref| is small and the fp32 bar does)
    for name in ('one row missing', 'one row counted twice'):
        assert passes_old[name], f'{name}: expected to pass the {BF16_BAR:g} bar'


@pytest.mark.parametrize('D', [128, 200])
def test_dx_faults_rejected(D):
    """dx (bf16, with residual): a wrong 1/D, a skipped column group, a missing residual and a truncating store.  D = 128: the
    equality check; D = 200: equality on the mirrored rows, the derived bound on the others.  The wrong 1/D, the skipped
    group and the truncating store measure 2e-3 ... 3e-3 and pass the 1e-2 bar (asserted); the missing residual measures
    1.0 and does not."""
    c = _case(D, 'bf16')
    ex = c['exact_rows']
    _, want = L.bwd_expected_dx(c)
    ref = c['dx']
    assert not X.mismatch(X.rne_bf16(ref[ex]), want).any()
    lim = c['bound'] + L.half_bf16_ulp(ref)

    def rejected(bad_bf16):
        n = int(X.mismatch(bad_bf16[ex], want).sum())
        return n + int(((bad_bf16[~ex].double() - ref[~ex]).abs() > lim[~ex]).sum())

    # the good result passes both checks
    assert rejected(X.rne_bf16(ref)) == 0
    nch_d = 256.0 * ((D + 255) // 256)
    s1, s2 = c['c1'] * D, c['c2'] * D
    faults = [('1/(256 NCH) for 1/D', X.rne_bf16(_dx_of(c, s1 / nch_d, s2 / nch_d)))]
    # the last column group left out of the row sums (its own outputs are never stored: the sentinel check)
    gl, gxl = c['g'][:, D - 4:].sum(1, keepdim=True), (c['g'] * c['xh'])[:, D - 4:].sum(1, keepdim=True)
    faults.append(('last 4-column group skipped', X.rne_bf16(_dx_of(c, (s1 - gl) / D, (s2 - gxl) / D))))
    faults.append(('residual not added', X.rne_bf16(_dx_of(c, c['c1'], c['c2'], with_res=False))))
    faults.append(('truncating bf16 store', (ref.float().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)))
    for name, bad in faults:
        n = rejected(bad)
        e = relerr(bad.double(), ref)
        report(f'ok   exact-sensitivity [ln dx D={D}] {name}: rejected ({n} elements); tolerance metric {e:.2e} vs bf16 bar {BF16_BAR:g}')
        assert n > 0, f'D={D}: fault "{name}" passes the new check'
        if name != 'residual not added':
            assert e <= BF16_BAR, f'{name}: expected to pass the {BF16_BAR:g} bar'


def test_check_bounded_and_rstd_reject(monkeypatch):
    monkeypatch.setattr(L, 'report', lambda line: None)          # deliberate failures stay out of the report
    ref = torch.tensor([1.0, 2.0], dtype=torch.float64)
    bound = torch.tensor([1e-6, 1e-6], dtype=torch.float64)
    assert L.check_bounded('self-test', torch.tensor([1.0, 2.0 + 5e-7], dtype=torch.float64), ref, bound) == pytest.approx(0.5)
    half = torch.tensor([0.0, 2.0 ** -8], dtype=torch.float64)             # a bf16 store: the half ulp is allowed on top
    L.check_bounded('self-test', torch.tensor([1.0, 2.0 + 2.0 ** -8], dtype=torch.float64), ref, bound, half)
    with pytest.raises(AssertionError, match='beyond their bound'):
        L.check_bounded('self-test', torch.tensor([1.0 + 2e-6, 2.0], dtype=torch.float64), ref, bound, half)
    zero = torch.zeros(2, dtype=torch.float64)
    assert L.check_bounded('self-test', ref, ref, zero) == 0.0              # nothing allowed, nothing used
    with pytest.raises(AssertionError, match='beyond their bound'):
        L.check_bounded('self-test', ref + 1e-9, ref, zero)
    with pytest.raises(AssertionError, match='beyond their bound'):
        L.check_bounded('self-test', torch.tensor([1.0, 2.0 + 2e-6], dtype=torch.float64), ref, bound)
    with pytest.raises(AssertionError, match='beyond their bound'):
        L.check_bounded('self-test', torch.tensor([float('nan'), 2.0], dtype=torch.float64), ref, bound)
    r = torch.tensor([0.5, 0.3], dtype=torch.float64)
    assert L.check_rstd('self-test', r.float(), r) <= 0.5
    with pytest.raises(AssertionError, match='ulp from float64'):
        L.check_rstd('self-test', r.float() * (1 + 2.0 ** -20), r)
