"""CPU checks of the second-trip cases (tests/exact_trip.py) that test_gpu_exact_trips.py runs: every case crosses its cap with a
ragged last trip, its expected buffer passes its own comparison, and that comparison REJECTS what a kernel would give that wrote
only its first trip or, for the two-pass kernels, reduced only its first trip (or everything but the ragged last one) -- each
emulation a restatement of the kernel's index arithmetic with the loop cut.  The caps themselves are read back from the
launchers' source text.

Why the tails are planted: without one, such a fault can go unseen.  On randaug_ref.planted_clip as it comes (224 x 224, no
planted tail) the random frames reach 0 and 255 long before their last 1024 pixels, so autocontrast with its min / max reduced
over everything but the ragged last trip gives exactly the expected clip: the comparison passes
(test_without_a_planted_tail_a_dropped_trip_goes_unseen).  With the frame's only minimum and maximum planted in the tail it is
rejected (test_two_pass_cases)."""
import pytest
import torch

import exact as X
import exact_trip as E
import randaug_ref as R
from helpers import report


def _rejects(c, label, emu):
    with pytest.raises(AssertionError):
        c.compare(emu)
    report(f'ok   {c.name}: the comparison rejects "{label}"')


def _sound(c):
    """The expected buffer passes; every emulation is rejected."""
    assert c.compare(c.full_expected())
    for label, make in c.emus.items():
        _rejects(c, label, make())


# -------------------------------------------------------------------------------------------------- the trip table
def test_caps_are_tracked():
    """Every launcher text of the table is still in its source file: a changed cap must come with a changed case."""
    for kernel, (fname, texts, cap, per) in E.TRIPS.items():
        with open(f'{E.CSRC}/{fname}') as f:
            src = f.read()
        for t in texts:
            assert t in src, f'{kernel}: csrc/{fname} no longer holds "{t}" -- the cap of {cap} workgroups in exact_trip.TRIPS is stale'
    assert E.trip('cast_from_f32') == 1048576 and E.trip('patch_rows') == 4194304 and E.trip('im2col3d_u8') == 2097152


def test_hog_grid_restates_the_launcher():
    """MI355X: 2 workgroups per CU on the three-channel path (wave-limited), 3 on 272-wide frames (LDS-limited; never above 8)."""
    assert E.hog_grid(32, 256, 10 ** 6) == (512, 2) and E.hog_grid(272, 256, 10 ** 6) == (768, 3)
    assert E.hog_grid(1024, 256, 10 ** 6)[1] <= 8 and E.hog_grid(32, 256, 100)[0] == 100


# -------------------------------------------------------------------------------------------- elementwise.hip
def test_cast_cases():
    for kind in ('from_f32', 'to_f32'):
        c = E.cast_case(kind)
        assert c.n > E.trip(f'cast_{kind}') and c.n % 256 and (c.n - E.trip(f'cast_{kind}')) % 256
        _sound(c)


@pytest.mark.parametrize('dtn', ['f32', 'bf16'])
def test_glue_cases(dtn):
    """fact_glue_bwd, space_grad_prep in both token orders (the second trip is exactly the cls rows), row_scale_copy."""
    _sound(E.fact_glue_bwd_case(dtn))
    for seq_major in (False, True):
        c = E.space_grad_prep_case(dtn, seq_major)
        _sound(c)
        first = c.emus["first trip only"]()
        assert X.sentinel_touched(c.view(first, 'da')[-8:]) == 0 and X.sentinel_touched(c.view(first, 'da')[:-8]) == c.view(first, 'da')[:-8].numel()
    a, b = E.space_grad_prep_case(dtn, False), E.space_grad_prep_case(dtn, True)
    assert not torch.equal(a.expected['da'], b.expected['da']), 'the two token orders give the same rows'
    _sound(E.row_scale_copy_case(dtn))


@pytest.mark.parametrize('dtn', ['f32', 'bf16'])
def test_embed_table_cases(dtn):
    for fm in (False, True):
        c = E.embed_table_case(dtn, fm)
        _sound(c)
        assert int(c.tail[-1]) == c.cls_off + c.D - 1                      # the cls row is the last item
    assert not torch.equal(E.embed_table_case(dtn, False).expected['E'], E.embed_table_case(dtn, True).expected['E'])


@pytest.mark.parametrize('key,dtn', [('w4', 'f32'), ('w4', 'bf16'), ('s8-token', 'f32'), ('s8-frame', 'f32')])
def test_patch_rows_cases(key, dtn):
    """The restated destination of every run covers the rows exactly once (first and later trips together), and cutting the
    later ones is rejected."""
    c = E.patch_rows_case(key, dtn)
    assert c.items == 4205568
    _sound(c)
    g = E.PATCH[key]
    allo = E.patch_run_offsets(torch.arange(c.items), g['B'], g['T'], g['C'], g['H'], g['W'], g['ps'], g['ts'], g['frame_major'], c.ld)
    hit = torch.zeros(c.numel, dtype=torch.int32)
    hit.index_add_(0, allo, torch.ones_like(allo, dtype=torch.int32))
    assert bool((c.view(hit, 'rows') == 1).all()) and int(hit.sum()) == c.M * c.K


def test_patch_rows_u8_case():
    c = E.patch_rows_u8_case()
    assert c.items == 4205568
    _sound(c)


def test_mixed_gather_tail():
    """The mixed gather is compared on the device with the float route; here: the items behind its first trip write distinct
    elements of the rows, 24 each, and all items together as many as the rows hold -- so a kernel without its second trip
    leaves that many NaN sentinels in the compared rows, which no torch.equal accepts."""
    for fm in (False, True):
        items, tail, M, K = E.mix_tail(fm)
        assert items == 4205568 and items * 24 == M * K
        assert len(tail) == (items - E.trip('patch_rows_mix_u8')) * 24 and len(torch.unique(tail)) == len(tail)
        assert 0 <= int(tail.min()) and int(tail.max()) < M * K


def test_cutmix_case():
    c = E.cutmix_case()
    assert c.compare(c.want)
    emu = c.emus['first trip only']()
    assert int((emu != c.want).sum()) > 100000
    _rejects(c, 'first trip only', emu)
    with pytest.raises(AssertionError):
        c.compare(c.clip.flip(0))                                           # the whole frame swapped: column 0 moved


def test_im2col_u8_case():
    for dtn in ('f32', 'bf16'):
        _sound(E.im2col_u8_case(dtn))


# ------------------------------------------------------------------------------------------------- colour jitter
@pytest.mark.parametrize('hw', E.JIT_SHAPES, ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_jitter_cases(hw):
    """The builder asserts every grey sum below 2^24 (torch.mean of the float32 greys is then order-independent and equals the
    exact-sum form).  The tail moves the contrast mean: an emulated sum pass without it changes the clips that draw contrast,
    an emulated apply pass without its second trip every clip with an op."""
    c = E.jitter_case(hw)
    npix = hw[0] * hw[1]
    vec, per = E.per_trip(hw)
    assert c.crosses == (npix > 64 * per) and (not c.crosses or (npix - 64 * per) % per)
    assert c.compare(c.want)
    assert set(c.emus) == ({'first-trip sum', 'first trip only'} if c.crosses else {'first-trip sum'})
    for label, emu in c.emus.items():
        for b in c.affected[label]:
            assert not torch.equal(emu[b], c.want[b]), f'{c.name}: "{label}" leaves clip {b} as expected'
        print(f'{c.name}: "{label}" changes {int((emu != c.want).sum())} bytes')
        _rejects(c, label, emu)
    guard = c.want.clone()
    guard[c.B, 0, 0, 0, 0] ^= 1
    _rejects(c, 'a byte of the guard clip written', guard)


def test_jitter_contract_beyond_65793_pixels():
    """At 448 x 448 the exact-sum mean and this CPU's torch.mean of the float32 greys give different bytes on some frames (counted
    and reported, not asserted: torch.mean's value there depends on its summation order)."""
    c = E.jitter_big_case()
    assert c.compare(c.want)
    means, of, frames, nbytes = E.jitter_torch_mean_differences(c)
    report(f'jitter 448x448: torch.mean of the float32 greys differs from the exact-sum mean on {means} of {of} frames; the two '
           f'restatements differ on {frames} of 12 frames, {nbytes} bytes')


# --------------------------------------------------------------------------------------------------- RandAugment
@pytest.mark.parametrize('op,hw', [(op, hw) for op in ('autocontrast', 'equalize') for hw in E.TWO_PASS_SHAPES],
                         ids=lambda v: v if isinstance(v, str) else f'{v[0]}x{v[1]}')
def test_two_pass_cases(op, hw):
    """Under every sel pattern: the expected clip passes; the reductions cut to their first trip, and to everything but the
    ragged last trip, are rejected; where the apply pass crosses its cap (equalize everywhere, autocontrast at 258 x 256 and
    127 x 131), so is the apply pass cut to its first trip.  Clip 2 (and clip 0) carry the planted tails."""
    _, per = E.per_trip(hw)
    npix = hw[0] * hw[1]
    cap = 64 if op == 'autocontrast' else 8
    for sel in E.SELS:
        c = E.two_pass_case(op, hw, tuple(sel))
        assert c.compare(c.want)
        assert ('first trip only' in c.emus) == (npix > cap * per)
        for label, emu in c.emus.items():
            for b in (0, 2):
                if sel[b]:
                    assert not torch.equal(emu[b], c.want[b]), f'{c.name}: "{label}" leaves clip {b} as expected'
            _rejects(c, label, emu)


def test_without_a_planted_tail_a_dropped_trip_goes_unseen():
    c = E.two_pass_case('autocontrast', (224, 224), (0, 1, 1), planted=False)
    assert c.compare(c.emus['reduction without the last trip'])


@pytest.mark.parametrize('hw', E.PW_SHAPES, ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_pointwise_cases(hw):
    for shift in range(3):
        c = E.pointwise_case(hw, shift)
        assert c.compare(c.want)
        emu = c.emus['first trip only']
        for b in c.processed:
            assert not torch.equal(emu[b], c.want[b])
        _rejects(c, 'first trip only', emu)
    n = 2 * hw[0] * hw[1] * 3
    assert (n % 16 == 0) == (hw == (840, 840)) and n > 1024 * 256 * (16 if n % 16 == 0 else 1)


def test_warp_tie_shares():
    """The ten warp cases at the frames the device tests use stay far below TIE_SHARE (measured: 0.0041 at 224 x 224, 0.0057
    at 47 x 45, 0.0041 at 258 x 256)."""
    for hw in ((224, 224), (47, 45), (258, 256)):
        worst = max(float(R.near_tie(*R.warp_coords64(R.matrix_of(op, mag, hw), hw)).mean()) for op, mag in R.signed_cases(hw))
        report(f'warp tie share at {hw}: {worst:.4f}')
        assert worst <= R.TIE_SHARE


# ----------------------------------------------------------------------------------------------------------- HOG
@pytest.mark.parametrize('select', [False, True])
@pytest.mark.parametrize('path', list(E.HOG_KINDS))
def test_hog_cases(path, select):
    """More than two trips of the persistent grid with a ragged rest; workgroups that meet a constant frame right behind a busy
    one; strips cut to the first trip, and a constant frame's strip that repeats its workgroup's previous output, are rejected."""
    c = E.hog_case(path, E.MI355X_CUS, select)
    assert c.items > 2 * c.grid and c.items % c.grid and c.stale >= 8
    assert c.compare(c.want)
    for label, make in c.emus.items():
        _rejects(c, label, make())
    for cus in (64, 304):                                 # the device test sizes the case by the CU count it finds
        o = E.hog_case(path, cus, select)
        assert o.items > 2 * o.grid and o.items % o.grid and o.stale >= 8
    if select:
        assert c.n == c.F - 2 and not torch.equal(c.sel, c.sel.sort().values)
        other = c.want.clone()
        other[5] = c.want[6]
        _rejects(c, 'a frame that was not selected written', other)
