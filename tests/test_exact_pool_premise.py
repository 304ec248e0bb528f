"""CPU checks of the exact pooling / position / stem test machinery (tests/exact_pool.py): the premise of every case that
test_gpu_exact_pool.py runs, the float64 references against each other, and that the equality checks reject kernel faults
emulated on the CPU by a literal restatement of each kernel's index arithmetic."""
import pytest
import torch
import torch.nn.functional as TF

import exact as X
import exact_ln as L
import exact_pool as P
from helpers import relerr, report

SMALL = [t[:5] for t in P.TABLE[:7]]
LN_TRIP_SHAPE, PB_SHAPES = P.TABLE[6][:5], (P.TABLE[7][:5], P.TABLE[8][:5])


def _differ(got, want):
    return int(X.mismatch(got.float(), want.float()).sum())


# ----------------------------------------------------------------------------------------------- references
def test_references_agree():
    """conv_T_ref and dw_ref against the float64 autograd of the conv3d reference, and the literal restatements without a
    fault against the references, at asymmetric strides."""
    for shape in SMALL[:4]:
        c = P.bwd_case(shape, 'f32', 'mirrored')
        d = c['d']
        xr = c['x'].double().requires_grad_(True)
        wr = c['w'].double().requires_grad_(True)
        g = xr[:, 1:].reshape(d['B'], d['T'], d['H'], d['W'], d['C']).permute(0, 4, 1, 2, 3)
        o = TF.conv3d(g, wr.reshape(-1, 1, 3, 3, 3).repeat(d['heads'], 1, 1, 1, 1), stride=(1, d['sh'], d['sw']), padding=1, groups=d['C'])
        pre = torch.cat([xr[:, :1], o.flatten(2).transpose(1, 2)], 1)
        pre.backward(c['stored'])
        assert torch.equal(xr.grad, c['dx']) and torch.equal(wr.grad, c['dw'])
        assert torch.equal(P.emu_dx(c['stored'], c['w'], shape), c['dx'])
        assert torch.equal(P.emu_pre(c['x'], c['w'], shape), P.conv_ref(c['x'], c['w'], shape))
    for geom in P.IM2COL_GEOMS:
        clip = X.ints(geom[4], 1, 99, 1.0, 5)
        assert torch.equal(P.emu_im2col(clip, geom), P.im2col_ref(clip, geom))


# -------------------------------------------------------------------------------------------- case premises
def test_forward_case_premises():
    """Built for every table entry (the builder asserts integer pre within +-256, exact mean / deviations / sums of squares on
    the exact rows): non-zero cls rows that differ per clip, about one hd-96 output row in four unmirrored, the y bound
    below 1e-4 of what it guards, and the bf16 'round' case meeting the tie / inexact floors with the float64 rstd."""
    for shape, dt, kind in P.fwd_table():
        c = P.fwd_case(shape, dt, kind)
        d = c['d']
        cls = c['x'][:, 0]
        assert bool((cls != 0).all()) and (d['B'] == 1 or not torch.equal(cls[0], cls[1]))
        y, ystar, bound = P.fwd_expected_y(c, c['rstd'].float())
        ex = c['exact']
        if d['hd'] == 96 and kind == 'plain':
            frac = 1 - float(ex.double().mean())
            assert 0.08 <= frac <= 0.5 and int((~ex).sum()) >= 2, (c['name'], frac)
            assert float((bound / ystar.abs().clamp_min(0.25)).max()) < 1e-4
            m32 = c['mean32'][~ex].double()                 # fl32(S / 96): within half an ulp of S / 96, and not S / 96 itself
            assert bool((L.ulp_distance(m32, c['mean'][~ex])[c['S'][~ex] != 0] <= 0.5).all())
            assert bool((c['S'][~ex] != 0).any())
        else:
            assert bool(ex.all())
        assert bool((c['pre'][:, 1:] != 0).any())


def test_backward_case_premises():
    """Built for every table entry (the builder asserts the exact intermediates): dgamma / dbeta fp32-exact, both kinds of row in
    'mixed', exact dx / dw sums in every 'mirrored' case, bounds far below the values they guard."""
    for shape, dt, mode in P.bwd_table():
        c = P.bwd_case(shape, dt, mode)
        P.bwd_expected_dpre(c)
        X.assert_fp32_exact(c['name'] + ' dgamma', c['dgamma'])
        X.assert_fp32_exact(c['name'] + ' dbeta', c['dbeta'])
        assert bool((c['x'][:, 0] != 0).all())
        if mode == 'mixed':
            assert bool(c['mirrored'].any()) and not bool(c['mirrored'].all())
            um = ~c['exact_rows']
            if bool(um.any()):
                assert float((c['bound'][um] / c['dpre'][um].abs().clamp_min(1.0)).max()) < 1e-4
        else:
            assert c['sums_exact'], (c['name'], c.get('sum_units'))
        if not c['sums_exact']:
            # fp32: the worst-case summation term dominates (a lost pair moves dw by a unit of dpre or more); bf16: the stored dpre of an inexact row may sit one bf16 ulp away, times |w| <= 2 per tap
            # (the sharp check of dx / dw is the equality of the 'mirrored' launch of the same shape; this one is worst-case)
            assert float(c['dx_bound'].max()) < (1e-3 if dt == 'f32' else 0.5), c['name']
            assert float((c['dw_bound'] / c['dw'].abs().clamp_min(1.0)).max()) < (0.05 if dt == 'f32' else 0.5), c['name']
        report(f"ok   premise {c['name']}: dx / dw held with {'equality' if c['sums_exact'] else 'the carried bound'}")


def test_other_case_premises():
    for C in (96, 40):
        for kind in ('exact', 'round'):
            out = P.pos_reference(P.pos_case(C, kind))[0]
            X.expect_bf16(f'pos_encoding {C} {kind}', out, kind)
    s = P.stem_case()
    assert bool((s['out'] != 0).any()) and bool((s['d_w'] != 0).any())


# ----------------------------------------------------------------------------------------- fault emulation
@pytest.mark.parametrize('fault,needs', [('swap', 'sh != sw'), ('flip', None), ('far_edge', 'a window whose last row is h = H - 1'),
                                         ('cls_conv', None)])
def test_forward_faults_rejected(fault, needs):
    """pre under each emulated fault differs from the reference on at least one table shape; 'swap' on exactly the shapes
    with sh != sw."""
    hits = []
    for shape in SMALL:
        c = P.fwd_case(shape, 'f32')
        n = _differ(P.emu_pre(c['x'], c['w'], shape, fault), c['pre'])
        e = relerr(P.emu_pre(c['x'], c['w'], shape, fault), c['pre'])
        if n:
            hits.append(shape)
        report(f'ok   exact-sensitivity [pool fwd] {fault} {shape}: {n} elements differ; tolerance metric {e:.2e}')
        if fault == 'swap':
            assert (n > 0) == (shape[4][0] != shape[4][1]), shape
    assert hits, f'{fault} passes every table shape'
    assert P.TABLE[0][:5] in hits            # the first shape (sh != sw, (H - 1) % sh == 0) sees all four


def test_swap_passes_the_old_shapes():
    """Why the table exists: every shape of test_gpu_mvit.test_pool_conv_ln has sh == sw, so the swap is invisible there."""
    for shape in P.OLD_SHAPES:
        x, w = X.ints((shape[0], P.dims(shape)['n_in'], P.dims(shape)['C']), -2, 2, 0.3, 1), X.ints((shape[2], 27), -2, 2, 1.0, 2)
        ref = P.conv_ref(x, w, shape)
        assert torch.equal(P.emu_pre(x, w, shape, 'swap'), ref)
        assert torch.equal(P.emu_dx(ref, w, shape, 'swap'), P.emu_dx(ref, w, shape))


def test_backward_data_faults_rejected():
    """dx with the strides swapped (the shapes with sh != sw) and with the head offset left in the weight index (heads > 1)."""
    for fault in ('swap', 'head_offset'):
        hits = []
        for shape in SMALL:
            c = P.bwd_case(shape, 'f32', 'mirrored')
            if _differ(P.emu_dx(c['stored'], c['w'], shape, fault), c['dx']):
                hits.append(shape)
        want = [s for s in SMALL if (s[4][0] != s[4][1] if fault == 'swap' else s[1] > 1)]
        assert hits == want, (fault, hits)
        report(f'ok   exact-sensitivity [pool bwd data] {fault}: rejected on {len(hits)} shapes')


def test_second_ln_trip_dropped_is_rejected():
    """8196 units over 1024 workgroups of 8: units 8192 .. 8195 belong to the second trip.  Without them dgamma / dbeta change
    (needs the 8196-unit shape; every other shape has one trip)."""
    c = P.bwd_case(LN_TRIP_SHAPE, 'f32', 'mixed')
    units, D = c['d']['units'], c['d']['hd']
    assert P.LN_GRID * 8 < units < 2 * P.LN_GRID * 8
    assert all(P.dims(s)['units'] <= P.LN_GRID * 8 for s in SMALL if s != LN_TRIP_SHAPE)
    keep = (torch.arange(units) < P.LN_GRID * 8).double()[:, None]
    dy = c['dy'].reshape(units, D).double()
    xh = (c['pre'].reshape(units, D).double() - c['mu'].double()[:, None]) * c['rs'].double()[:, None]
    n = _differ((keep * dy * xh).sum(0), c['dgamma']) + _differ((keep * dy).sum(0), c['dbeta'])
    e = max(relerr((keep * dy * xh).sum(0), c['dgamma']), relerr((keep * dy).sum(0), c['dbeta']))
    report(f'ok   exact-sensitivity [pool ln bwd] second trip dropped: {n} elements differ; tolerance metric {e:.2e}')
    assert n > 0


@pytest.mark.parametrize('shape', PB_SHAPES)
def test_weight_batching_faults_rejected(shape):
    """135 200 pairs over 2048 blocks: 67 pairs per block, batches of 64 and 3, and trailing blocks with an empty slice (needs
    these shapes: every other has at most 32 pairs per block and no empty block).  Dropping the second batch moves dw; an
    empty block that leaves its partials unwritten adds whatever the workspace held (the GPU test fills it with NaN)."""
    nb, per = P.w_block_slices(shape)
    assert (nb, per) == (P.W_BLOCKS, 67) and per > P.PB and per % P.PB != 0 and P.empty_w_blocks(shape) >= 1
    assert all(P.w_block_slices(s)[1] <= 32 and P.empty_w_blocks(s) == 0 for s in SMALL)
    c = P.bwd_case(shape, 'bf16' if shape[2] == 64 else 'f32', 'mirrored')
    bad = P.dw_ref(c['stored'], c['x'], shape, P.pair_weight_without_second_batch(shape))
    n, e = _differ(bad, c['dw']), relerr(bad, c['dw'])
    report(f'ok   exact-sensitivity [pool bwd weight] second batch dropped {shape}: {n} elements differ; tolerance metric {e:.2e}')
    assert n > 0
    assert _differ(c['dw'] + P.empty_w_blocks(shape) * float('nan'), c['dw']) == c['dw'].numel()


def test_im2col_carry_fault_rejected():
    for geom in P.IM2COL_GEOMS:
        clip = X.ints(geom[4], 1, 99, 1.0, 5)
        assert _differ(P.emu_im2col(clip, geom, 'kh_carry'), P.im2col_ref(clip, geom)) > 0


def test_maxpool_reference_rule_and_fault():
    """The CPU reference on hand-made windows: the gradient goes to the first maximum in (kh, kw) order -- also when every
    in-range tap is -inf, where it is the first in-range tap -- and a NaN is propagated and takes the gradient.  Then: the
    cases hold such windows, and the last-maximum scan is rejected."""
    def run(frame):
        x = torch.cat([torch.zeros(1, 1, 8), torch.tensor(frame).reshape(1, 9, 1).repeat(1, 1, 8)], 1)
        dy = torch.ones(1, 1 + 4, 8)
        y, dx = P.maxpool_ref(x, dy, (1, 3, 3))
        return y[0, 1:, 0].tolist(), dx[0, 1:, 0].reshape(3, 3).tolist()
    # 3 x 3 frame, outputs 2 x 2; output (i, j) sees rows 2i-1 .. 2i+1 and columns 2j-1 .. 2j+1 inside the frame
    y, dx = run([[1., 5., 5.], [5., 5., 0.], [0., 0., 5.]])         # (0,0) and (0,1): first 5 at (0,1); (1,0): (1,0); (1,1): (1,1), not (2,2)
    assert y == [5., 5., 5., 5.] and dx == [[0., 2., 0.], [1., 1., 0.], [0., 0., 0.]]
    ninf = float('-inf')
    y, dx = run([[ninf] * 3] * 3)                                    # every tap -inf: the first IN-RANGE tap, tap (1, 1) for output (0, 0)
    assert y == [ninf] * 4 and dx == [[1., 1., 0.], [1., 1., 0.], [0., 0., 0.]]
    y, dx = run([[1., 2., 3.], [4., float('nan'), 9.], [7., 8., 6.]])
    assert all(v != v for v in y) and dx[1][1] == 4. and sum(map(sum, dx)) == 4.
    for thw in P.MAXPOOL_GRIDS:
        x, dy = P.maxpool_case(thw)
        y, dx = P.maxpool_ref(x, dy, thw)
        yl, dxl = P.maxpool_ref(x, dy, thw, last=True)
        assert bool(torch.isnan(y).any()) and bool((y[:, 1:] == ninf).any()) and bool((y[:, 1:].abs() <= 2).any())
        assert X.mismatch(yl, y).sum() == 0, 'the scan differs from MaxPool3d in the values'
        assert _differ(dxl, dx) > 0, f'{thw}: last-maximum placement passes'
        X.assert_fp32_exact('maxpool dx', dx)
