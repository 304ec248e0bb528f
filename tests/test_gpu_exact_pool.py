"""Exact-arithmetic parity of the MViT pooling, position and stem kernels (csrc/mvit.hip; helpers: tests/exact_pool.py).

The raw entry points run on sentinel-filled buffers with trailing rows (pre, y, dpre, dx) or trailing elements (mean, rstd, dw,
dgamma, dbeta) that must stay bit-unchanged; the backward workspace is NaN on entry, so a partial slab that is read without
having been written shows.  What is compared how is in the docstring of exact_pool.py.

Shapes (B, heads, hd, (T, H, W), (sh, sw)) and the loop property each is there for:
  (2, 2, 96, (2, 7, 12), (2, 4))     sh != sw, H != W; (H-1) % sh == 0 but (W-1) % sw != 0; 16-lane groups with 4 idle lanes; units no
                                     multiple of 16; W * C/8 = 288 items per row: the second trip of backward-data's thread loop
  (2, 3, 64, (3, 8, 5), (4, 2))      the opposite asymmetry; 3 heads (c0 % HD); input rows no output row reaches (zero fill);
                                     units no multiple of 32
  (2, 1, 96, (1, 5, 6), (8, 8))      T == 1 (both outer kt taps out); H, W < s: one output per frame, its window mostly padding
  (1, 2, 64, (2, 1, 9), (1, 2))      H == 1; stride 1 in one axis; 10 pairs: the weight kernel runs one block with a short batch
  (2, 4, 96, (2, 5, 7), (1, 1)), (2, 2, 64, (2, 8, 8), (2, 2))   the model's stride classes (the tolerance shapes, held exactly)
  (2, 2, 64, (2, 32, 32), (1, 1))    8196 units: the second trip of pool_ln_bwd_kernel, taken by four waves only; 1024 partial slabs
  (2, 1, 64, (4, 130, 130), (1, 1))  bf16 only: 135 200 pairs, 67 per block: batches of 64 and 3, trailing blocks with an empty slice
  (2, 1, 96, (4, 130, 130), (1, 1))  fp32 only: the same in the 12-chunk instantiation
Every backward shape runs with all rows mirrored (dx, dw with equality) and, but for the last two, with mixed rows.
Not run: temporal strides (the launcher refuses them); head dims other than 64 and 96 (not instantiated); the two large shapes
in the other dtype and with mixed rows; grids beyond the 32-bit index checks of the launchers.
"""
import ctypes

import pytest
import torch

import exact as X
import exact_ln as L
import exact_pool as P
from helpers import report

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16
TDT = {'f32': F32, 'bf16': BF16}
TAIL = 2                    # guard rows behind a row buffer
ids = lambda t: '-'.join(str(v) for v in t).replace(' ', '')   # noqa: E731


def dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _desc(shape, dt):
    from vtx import ops
    from vtx._lib import PoolDesc
    B, heads, hd, (T, H, W), (sh, sw) = shape
    d = PoolDesc()
    d.dtype = ops._DT[TDT[dt]]
    d.B, d.T, d.H, d.W, d.heads, d.hd, d.sh, d.sw = B, T, H, W, heads, hd, sh, sw
    return d


def _rows(n_rows, C, dtype):
    """Sentinel-filled [n_rows + TAIL, C] buffer."""
    return X.sentinel_fill(torch.empty(n_rows + TAIL, C, dtype=dtype, device=DEV))


def _vec(n, extra=8):
    return X.sentinel_fill(torch.empty(n + extra, dtype=F32, device=DEV))


def check_fwd(c, pre, y, mean, rstd, tag=''):
    """The four outputs of one forward launch (row buffers [rows (+ TAIL), C], statistics [units (+ extra)])."""
    d, name, tdt = c['d'], c['name'] + tag, TDT[c['dt']]
    rows, units, hd, ex = d['B'] * d['n_out'], d['units'], d['hd'], c['exact']
    X.check_exact(f'{name} pre', pre[:rows], c['pre'].reshape(rows, -1).to(tdt), {'trailing rows': pre[rows:]})
    m = mean[:units].cpu()
    X.check_exact(f'{name} mean', m[ex], c['mean'][ex].float(), {'beyond units': mean[units:]})
    r = rstd[:units].cpu()
    worst = L.check_rstd(name, r[ex], c['rstd'][ex])
    want, ystar, bound = P.fwd_expected_y(c, r)
    got = y[:rows].reshape(units, hd).cpu()
    X.check_exact(f'{name} y', got[ex], want, {'trailing rows': y[rows:], 'rstd beyond units': rstd[units:]})
    if bool((~ex).any()):
        X.check_exact(f'{name} mean = fl32(S / 96) (unmirrored rows)', m[~ex], c['mean32'][~ex])
        dist = L.ulp_distance(r[~ex], c['rstd'][~ex])
        w2 = float(dist.nan_to_num(nan=float('inf')).max())
        report(f'{"ok  " if w2 <= P.RSTD_ULPS_UNMIRRORED else "FAIL"} rstd {name} (unmirrored rows): {int((~ex).sum())} rows, largest '
               f'distance {w2:.3f} ulp (bar {P.RSTD_ULPS_UNMIRRORED:g})')
        assert w2 <= P.RSTD_ULPS_UNMIRRORED, f'{name}: rstd of an unmirrored row {w2:.3f} ulp from float64'
        L.check_bounded(f'{name} y (unmirrored rows)', got[~ex], ystar, bound, None if c['dt'] == 'f32' else L.half_bf16_ulp(ystar))
    return worst


@pytest.mark.parametrize('case', P.fwd_table(), ids=ids)
def test_pool_conv_ln_fwd(case):
    """vtx_pool_conv_ln_fwd: pre with equality against float64 conv3d; mean with equality, rstd within 4 ulp, y with equality
    given rstd (unmirrored hd-96 rows: fl32(S / 96), the derived bounds)."""
    from vtx import ops
    shape, dt, kind = case
    c = P.fwd_case(shape, dt, kind)
    d, tdt = c['d'], TDT[dt]
    rows = d['B'] * d['n_out']
    pre, y = _rows(rows, d['C'], tdt), _rows(rows, d['C'], tdt)
    mean, rstd = _vec(d['units']), _vec(d['units'])
    x, w, gamma, beta = dev(c['x'], tdt), dev(c['w']), dev(c['gamma']), dev(c['beta'])
    ops.call('vtx_pool_conv_ln_fwd', ctypes.byref(_desc(shape, dt)), ops.ptr(x), ops.ptr(w), ops.ptr(gamma), ops.ptr(beta), L.eps32(),
             ops.ptr(pre), ops.ptr(y), ops.ptr(mean), ops.ptr(rstd), ops.stream())
    torch.cuda.synchronize()
    check_fwd(c, pre, y, mean, rstd)


def test_pool_conv_ln_function_forward():
    """PoolConvLNFn.apply at an hd-64 shape: the Function hands the same buffers over (y returned, pre / mean / rstd saved)."""
    from vtx import functions as F_
    shape = P.TABLE[1][:5]
    c = P.fwd_case(shape, 'f32', 'plain')
    d = c['d']
    x = dev(c['x']).requires_grad_(True)
    y = F_.PoolConvLNFn.apply(x, dev(c['w']).reshape(d['hd'], 1, 3, 3, 3), dev(c['gamma']), dev(c['beta']), list(shape[3]), d['heads'],
                              (1,) + tuple(shape[4]), L.eps32())
    _, pre, mean, rstd, _, _ = y.grad_fn.saved_tensors
    assert tuple(y.shape) == (d['B'], d['n_out'], d['C'])
    check_fwd(c, pre.reshape(-1, d['C']), y.detach().reshape(-1, d['C']), mean, rstd, ' via PoolConvLNFn')


def check_bwd(c, dpre, dx, dw, dg, db):
    """The five outputs of one backward launch (row buffers with TAIL guard rows, vectors with guard elements)."""
    d, dt, name = c['d'], c['dt'], c['name']
    tdt = TDT[dt]
    rows_out, rows_in, C, hd, units = d['B'] * d['n_out'], d['B'] * d['n_in'], d['C'], d['hd'], d['units']
    X.check_exact(f'{name} dgamma', dg[:hd], c['dgamma'].float(), {'beyond hd': dg[hd:]})
    X.check_exact(f'{name} dbeta', db[:hd], c['dbeta'].float(), {'beyond hd': db[hd:]})
    ex = c['exact_rows']
    got = dpre[:rows_out].reshape(units, hd).cpu()
    X.check_exact(f'{name} dpre', got[ex], P.bwd_expected_dpre(c), {'trailing rows': dpre[rows_out:]})
    if bool((~ex).any()):
        ref = c['dpre'][~ex]
        L.check_bounded(f'{name} dpre (unmirrored rows)', got[~ex], ref, c['bound'][~ex], None if dt == 'f32' else L.half_bf16_ulp(ref))
    gdx, gdw = dx[:rows_in].reshape(d['B'], d['n_in'], C), dw[:hd * 27].reshape(hd, 27)
    guards = {'dx trailing rows': dx[rows_in:], 'dw beyond hd * 27': dw[hd * 27:]}
    if c['sums_exact']:
        X.check_exact(f'{name} dx', gdx, c['dx'].to(tdt), guards)
        X.check_exact(f'{name} dw', gdw, c['dw'].float())
    else:
        L.check_bounded(f'{name} dx (carried bound)', gdx, c['dx'], c['dx_bound'], None if dt == 'f32' else L.half_bf16_ulp(c['dx']))
        L.check_bounded(f'{name} dw (carried bound)', gdw, c['dw'], c['dw_bound'])
        X.check_exact(f'{name} guards', dx[:0], dx[:0].cpu(), guards)


@pytest.mark.parametrize('case', P.bwd_table(), ids=ids)
def test_pool_conv_ln_bwd(case):
    """vtx_pool_conv_ln_bwd as PoolConvLNFn.backward calls it: dpre, dgamma, dbeta, dx, dw."""
    from vtx import ops
    from vtx import _lib
    shape, dt, mode = case
    c = P.bwd_case(shape, dt, mode)
    d, tdt, name = c['d'], TDT[dt], c['name']
    rows_out, rows_in, C, hd, units = d['B'] * d['n_out'], d['B'] * d['n_in'], d['C'], d['hd'], d['units']
    junk = torch.full((3,), 77.0)
    mean, rstd = dev(torch.cat([c['mu'], junk])), dev(torch.cat([c['rs'], junk]))
    dy, x, pre = dev(c['dy'], tdt), dev(c['x'], tdt), dev(c['pre'], tdt)
    w, gamma = dev(c['w']), dev(c['gamma'])
    dpre, dx = _rows(rows_out, C, tdt), _rows(rows_in, C, tdt)
    dw, dg, db = _vec(hd * 27), _vec(hd), _vec(hd)
    desc = _desc(shape, dt)
    ws_bytes = _lib.load().vtx_pool_conv_ln_bwd_workspace(ctypes.byref(desc))
    ws = torch.full((ws_bytes // 4 + 8,), float('nan'), device=DEV)
    ops.call('vtx_pool_conv_ln_bwd', ctypes.byref(desc), ops.ptr(dy), ops.ptr(x), ops.ptr(pre), ops.ptr(mean), ops.ptr(rstd), ops.ptr(w),
             ops.ptr(gamma), ops.ptr(dpre), ops.ptr(dx), ops.ptr(dw), ops.ptr(dg), ops.ptr(db), ops.ptr(ws), ws_bytes, ops.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[ws_bytes // 4:]).all()), f'{name}: the workspace was written beyond its stated size'
    check_bwd(c, dpre, dx, dw, dg, db)


# ------------------------------------------------------------------------------------------ position encoding
@pytest.mark.parametrize('C', [96, 40])
@pytest.mark.parametrize('dt,kind', [('f32', 'exact'), ('bf16', 'exact'), ('bf16', 'round')])
def test_pos_encoding_exact(dt, kind, C):
    """PosEncodingFn forward and backward on integers against float64 autograd of the oracle module.  The kernel adds spatial +
    temporal first and x last; with integers every grouping is exact, so the order is not observable here."""
    from vtx import functions as F_
    c = P.pos_case(C, kind)
    out, dx, d_cls, d_pc, d_sp, d_tp = P.pos_reference(c)
    tdt = TDT[dt]
    ps = [dev(c[k]).requires_grad_(True) for k in ('cls', 'pos_class', 'spatial', 'temporal')]
    x = dev(c['x'], tdt).requires_grad_(True)
    y = F_.PosEncodingFn.apply(x, *ps)
    y.backward(dev(c['dy'], tdt))
    name = f'pos_encoding {dt} {kind} C={C}'
    X.check_exact(f'{name} out', y.detach(), X.expect_bf16(name, out, kind) if dt == 'bf16' else out.float())
    X.check_exact(f'{name} dx', x.grad, dx.to(tdt))
    for nm, p, ref in zip(('d_cls', 'd_pos_class', 'd_spatial', 'd_temporal'), ps, (d_cls, d_pc, d_sp, d_tp)):
        X.check_exact(f'{name} {nm}', p.grad, ref.float())


# ------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize('geom', range(len(P.IM2COL_GEOMS)))
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_im2col3d_bitexact(dt, geom):
    """vtx_im2col3d is a pure gather: bit for bit against pad + unfold on the CPU (a NaN only has to stay a NaN), on the fp32
    special patterns, including the padding positions (+0) and the zero columns K .. Kp - 1; sentinel rows behind row M."""
    from vtx import ops
    from test_gpu_exact_arith import _check_cast, _f32_specials
    g = P.IM2COL_GEOMS[geom]
    k3, s3, p3, Cc, cs, Kp = g
    n = cs[0] * cs[1] * cs[2] * cs[3] * cs[4]
    clip = _f32_specials()[:n].reshape(cs).contiguous()
    want = P.im2col_ref(clip, g)
    M, tdt = want.shape[0], TDT[dt]
    rows = _rows(M, Kp, tdt)
    i3 = lambda t: (ctypes.c_int * 3)(*t)   # noqa: E731
    ops.call('vtx_im2col3d', ops._DT[tdt], cs[0], cs[1], Cc, cs[3], cs[4], i3(k3), i3(s3), i3(p3), Kp, ops.ptr(dev(clip)), ops.ptr(rows),
             ops.stream())
    torch.cuda.synchronize()
    _check_cast(f'im2col3d {dt} geometry {geom}', rows[:M], want.to(tdt))
    X.check_exact(f'im2col3d {dt} geometry {geom} guard rows', rows[:0], rows[:0].cpu(), {'rows behind M': rows[M:]})


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_conv_stem_exact(dt):
    """ConvStemFn end to end on sparse integers: output, d_w and d_b with equality."""
    from vtx import functions as F_
    s, tdt = P.stem_case(), TDT[dt]
    w, b = dev(s['w']).requires_grad_(True), dev(s['b']).requires_grad_(True)
    y = F_.ConvStemFn.apply(dev(s['clip']), w, b, (2, 4, 4), (1, 3, 3), tdt)
    y.backward(dev(s['dy'], tdt))
    X.check_exact(f'conv stem {dt} out', y.detach(), s['out'].to(tdt))
    X.check_exact(f'conv stem {dt} d_w', w.grad, s['d_w'].float())
    X.check_exact(f'conv stem {dt} d_b', b.grad, s['d_b'].float())


# -------------------------------------------------------------------------------------------- max pool
@pytest.mark.parametrize('thw', P.MAXPOOL_GRIDS, ids=ids)
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_maxpool_skip_ties_nan_inf(dt, thw):
    """MaxPoolSkipFn on windows with repeated maxima, NaNs and all -inf in-range taps, grids with H or W of 1: values and the
    gradient placement with equality against torch.nn.MaxPool3d on the CPU (first maximum wins; a NaN is propagated)."""
    from vtx import functions as F_
    x, dy = P.maxpool_case(thw)
    yr, dxr = P.maxpool_ref(x, dy, thw)
    tdt = TDT[dt]
    xd = dev(x, tdt).requires_grad_(True)
    y = F_.MaxPoolSkipFn.apply(xd, list(thw))
    y.backward(dev(dy, tdt))
    X.check_exact(f'maxpool_skip {dt} {thw} fwd', y.detach(), yr.to(tdt))
    X.check_exact(f'maxpool_skip {dt} {thw} bwd', xd.grad, dxr.to(tdt))
