"""CPU checks of the pointwise GELU test machinery (tests/exact_gelu.py): the premises of every case that
test_gpu_exact_gelu.py runs, the bound held against the formula's own float64 and fp32 transcriptions, and that the interval
check rejects the kernel faults the whole-tensor tolerance of helpers.check lets through (emulated on the CPU)."""
import functools

import torch

import exact as X
import exact_gelu as G
from helpers import relerr, report


@functools.lru_cache(maxsize=None)
def _points():
    """f32_grid() and 2 * 10^6 points of linspace(-12, 12)."""
    return torch.cat([G.f32_grid(), torch.linspace(-12.0, 12.0, 2_000_000)])


def test_generators():
    v = G.all_bf16()
    assert v.numel() == 65026 and torch.unique(v.view(torch.int32)).numel() == 65026
    assert torch.equal(v.to(G.BF16).float(), v) and bool(torch.isfinite(v).all())
    nz = v[v != 0]
    assert bool((nz.abs() >= 2.0 ** -126).all()), 'no subnormals'
    assert int((v == 0).sum()) == 2 and bool(torch.signbit(v[v == 0]).any())
    s = G.bf16_subnormals()
    assert s.numel() == 254 and bool((s.abs() < 2.0 ** -126).all()) and bool((s != 0).all())
    assert G.bf16_range(2.0 ** -20, 8.0).numel() == 5890
    for K in G.GELU_KS:
        A = G.fill(v, G.GELU_M, K)
        assert bool((A[:, 1:] != A[:, :-1]).all()), 'adjacent columns hold different values'
    r = G.random_f32_normals(1 << 16)
    assert bool(torch.isfinite(r).all()) and bool((r.abs() >= 2.0 ** -126).all())
    g = G.f32_grid()
    assert bool(torch.isfinite(g).all())
    assert int(((g >= -14) & (g <= -12.5)).sum()) >= 1 << 14 and int(((g >= 5) & (g <= 6)).sum()) >= 1 << 14


def test_fine_premises():
    """Every pre-activation of the `fine` generator is fp32-exact whatever the summation order (asserted by the builder), and
    the bf16 store of the pre-activation copy is a rounding case: >= 20 % ties, >= 40 % inexact, both tie directions."""
    for K in G.GELU_KS:
        A, W, pre = G.fine_operands(G.GELU_M, K)
        X.expect_bf16(f'fine K={K}', pre, 'round')
        low = pre.float().view(torch.int32)
        tie = (low & 0xFFFF) == 0x8000
        odd = ((low >> 16) & 1) == 1
        assert int((tie & odd).sum()) > 1000 and int((tie & ~odd).sum()) > 1000, 'ties round up and down'
        assert int(((low & 0x03FF) != 0).sum()) > 0.2 * pre.numel(), '15 and 16 significant bits (fp32 bits 9 and 8)'
        ties, inexact = X.bf16_stats(pre)
        report(f'ok   premise gelu fine K={K}: {ties:.1%} ties, {inexact:.1%} inexact of {pre.numel()} pre-activations')
    A, W, pre = G.identity_operands(G.GELU_M, 192)
    X.assert_acc_bound('identity', A.abs().clamp_max(1.0), W)          # one non-zero term per dot product
    assert torch.equal(A.double(), pre)


def test_unit_accumulators():
    """The dgelu_kind = 0 cases: every accumulator is exactly 1, -2 and 0.5."""
    for K in G.GELU_KS:
        for c in (1.0, -2.0, 0.5):
            A, W = G.unit_operands(G.GELU_M, K, c)
            v = X.nt_reference(f'unit {c}', A, W)
            assert torch.equal(v, torch.full_like(v, c))


def test_float64_transcription_inside_bound_k0():
    """The formula itself (constants, branch structure) stays inside the bound with k = 0, up to the float64 evaluation's own
    roundings: at most eight of 2^-53 each, which is k = 8 * 2^-29 = 1.5e-8 in the bound's units of 2^-24."""
    x = _points()
    tg, td, _, _ = G.truth(x)
    g, d = G.gelu_f64(x)
    kg, kd = G.k_needed(x, g, d)
    assert kg <= 8 * 2.0 ** -29 and kd <= 8 * 2.0 ** -29, (kg, kd)
    ax = x.double().abs()
    eg = ((g - tg).abs() / ax.clamp_min(1e-300))[ax > 0].max().item()
    report(f'ok   premise gelu float64 transcription: max |err|/|x| {eg:.3e}, gelu\' max |err| {(d - td).abs().max().item():.3e}, '
           f'k needed {max(kg, kd):.1e} on {x.numel()} points')
    assert eg <= 7.5e-8 and (d - td).abs().max().item() <= 7.5e-8


def test_float32_transcription_inside_bound_k8():
    """The fp32 transcription with correctly rounded 1/x and exp2 stays inside the bound at K_REF = 8; the smallest k it
    needs is printed."""
    x = _points()
    g, d = G.gelu_f32(x)
    kg, kd = G.k_needed(x, g, d)
    print(f'fp32 transcription: smallest k: gelu {kg:.2f}, gelu\' {kd:.2f}')
    report(f'ok   premise gelu fp32 transcription: smallest k gelu {kg:.2f} gelu\' {kd:.2f} on {x.numel()} points')
    assert kg <= G.K_REF and kd <= G.K_REF, (kg, kd)
    tg, td, _, _ = G.truth(x)
    bg, bd = G.bounds(x, G.K_REF)
    assert bool(G.within(g, tg, bg, torch.float32).all()) and bool(G.within(d, td, bd, torch.float32).all())


def test_bound_pins_bf16_outputs():
    """At the GPU bar K_GPU the interval pins >= 95 % of the bf16 outputs with 2^-20 <= |x| <= 8 to one value, for gelu and
    gelu': the interval check cannot degenerate into a tolerance."""
    x = G.bf16_range(2.0 ** -20, 8.0)
    tg, td, _, _ = G.truth(x)
    bg, bd = G.bounds(x, G.K_GPU)
    pg, pd = G.pinned_share(tg, bg), G.pinned_share(td, bd)
    report(f'ok   premise gelu pinned shares at k={G.K_GPU}: gelu {pg:.1%} gelu\' {pd:.1%} of {x.numel()} bf16 inputs')
    assert pg >= 0.95 and pd >= 0.95, (pg, pd)
    g, d = G.gelu_f32(x)
    assert bool(G.within(g.to(G.BF16), tg, bg, G.BF16).all()) and bool(G.within(d.to(G.BF16), td, bd, G.BF16).all())


def test_interval_check_rejects_what_the_tolerance_passes():
    """Faults of a kernel emulated on the CPU over all_bf16(): each passes max|a - b| / max|b| <= 1e-2 on N(0, 1)-like inputs
    (the bar every GELU check had) and fails the interval check or the identity check."""
    x = G.all_bf16()
    g32, d32 = G.gelu_f32(x)
    tg, td, _, _ = G.truth(x)
    bg, bd = G.bounds(x, G.K_GPU)
    normal = x.abs() <= 4.0                                             # what a tolerance test samples
    faults = {
        'zero below -2.5': (torch.where(x < -2.5, torch.zeros_like(g32), g32), d32),
        'the wrong branch of the cdf on -0.05 < x < 0': (torch.where((x > -0.05) & (x < 0), x - g32, g32), d32),
        'Gaussian term of the derivative dropped for |x| > 3.2': (g32, torch.where(x.abs() > 3.2, (x >= 0).float(), d32)),
    }
    for name, (g, d) in faults.items():
        gb, db = g.to(G.BF16), d.to(G.BF16)
        assert relerr(gb.float()[normal], tg[normal]) <= 1e-2 and relerr(db.float()[normal], td[normal]) <= 1e-2, name
        ok = G.within(gb, tg, bg, G.BF16).all() and G.within(db, td, bd, G.BF16).all()
        assert not bool(ok), f'{name}: not rejected'
    # a packed pair swapped where the values are small: inside the tolerance, caught by equality with the canonical values
    sw = g32.clone().reshape(-1, 2)
    small = (g32.reshape(-1, 2).abs() < 0.02).all(1)
    sw[small] = sw[small].flip(1)
    swb = sw.reshape(-1).to(G.BF16)
    assert relerr(swb.float()[normal], tg[normal]) <= 1e-2
    assert bool(X.mismatch(swb, g32.to(G.BF16)).any())
