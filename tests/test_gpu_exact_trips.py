"""The second trip of every capped grid-stride kernel, bit for bit against a CPU reference (cases, trip table and the faults the
comparisons are known to reject: tests/exact_trip.py, tests/test_exact_trip_premise.py).

Each case has more items than `cap` workgroups x 256 threads take in one pass of the grid, a ragged last trip, outputs that
are filled with sentinels and followed by guards (a guard clip behind the last one where the kernel works in place), and a
tail whose loss the comparison would see.  What is not run, and why, is listed at the head of exact_trip.py."""
import ctypes

import numpy as np
import pytest
import torch

import exact as X
import exact_trip as E
import randaug_ref as R
from helpers import report

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16
DTN = ['f32', 'bf16']
I3 = ctypes.c_int * 3
F3 = ctypes.c_float * 3


def dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _at(buf, off=0):
    return buf.data_ptr() + off * buf.element_size()


def _launch(c, fn):
    """fn(buf) launches on the sentinel-filled device buffer of the case; then the case's own comparison."""
    buf = c.blank(DEV)
    fn(buf)
    torch.cuda.synchronize()
    c.compare(buf)


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _f32(x):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64).float().to(DEV)


def _hw_id(hw):
    return f'{hw[0]}x{hw[1]}'


# -------------------------------------------------------------------------------------------- elementwise.hip
def test_casts_second_trip():
    """cast_from_f32 / cast_to_f32 at n = 4096 * 256 + 4097: the special patterns again behind the first trip, 64 guard elements."""
    from vtx import ops
    c = E.cast_case('from_f32')
    src = dev(c.src)
    _launch(c, lambda buf: ops.call('vtx_cast_from_f32', ops._DT[BF16], c.n, ops.ptr(src), _at(buf), ops.stream()))
    c = E.cast_case('to_f32')
    src16 = dev(c.src)
    _launch(c, lambda buf: ops.call('vtx_cast_to_f32', ops._DT[BF16], c.n, ops.ptr(src16), _at(buf), ops.stream()))


@pytest.mark.parametrize('dtn', DTN)
def test_fact_glue_bwd_second_trip(dtn):
    """65 544 rows x 16 items: the last 8 rows of dx belong to the second trip; 8 guard rows behind them."""
    from vtx import ops
    c = E.fact_glue_bwd_case(dtn)
    dh = dev(c.dh, c.dt)
    _launch(c, lambda buf: ops.call('vtx_fact_glue_bwd', ops._DT[c.dt], c.B, c.T, c.P, c.D, ops.ptr(dh), _at(buf), None, 0, ops.stream()))


@pytest.mark.parametrize('seq_major', [False, True], ids=['frame-tokens', 'sequence-major'])
@pytest.mark.parametrize('dtn', DTN)
def test_space_grad_prep_second_trip(dtn, seq_major):
    """Both token orders (the P < 0 form too): the second trip is exactly the 8 cls rows; ldda = D + 8, 4 guard rows."""
    from vtx import ops
    c = E.space_grad_prep_case(dtn, seq_major)
    dout, s = dev(c.dout, c.dt), dev(c.s)
    _launch(c, lambda buf: ops.call('vtx_space_grad_prep', ops._DT[c.dt], c.B, c.T, -c.P if seq_major else c.P, c.D, ops.ptr(dout), c.D,
                                    ops.ptr(s), _at(buf), c.ld, ops.stream()))


@pytest.mark.parametrize('dtn', DTN)
def test_row_scale_copy_second_trip(dtn):
    """65 544 rows through the token map with the spatial scale index rs = (N, T, T, 1); cls rows and pad columns are guards."""
    from vtx import ops
    c = E.row_scale_copy_case(dtn)
    src, s = dev(c.src, c.dt), dev(c.s)
    _launch(c, lambda buf: ops.row_scale_copy(src, buf, c.M, c.D, ldd=c.ld, dmap=ops.tokmap(c.N), s=s, rs=(c.N, c.T, c.T, 1)))


@pytest.mark.parametrize('frame_major', [False, True], ids=['token-major', 'frame-major'])
@pytest.mark.parametrize('dtn', DTN)
def test_embed_table_second_trip(dtn, frame_major):
    """TimeSformer-B's table (1 204 992 elements): the cls row is the last item of the second trip."""
    from vtx import ops
    c = E.embed_table_case(dtn, frame_major)
    bias, pos, te, cls = dev(c.bias), dev(c.pos), dev(c.te), dev(c.cls)
    _launch(c, lambda buf: ops.call('vtx_embed_table', ops._DT[c.dt], c.P, c.T, c.D, ops.ptr(bias), ops.ptr(pos), ops.ptr(te), ops.ptr(cls),
                                    _at(buf), _at(buf, c.cls_off), int(frame_major), ops.stream()))


@pytest.mark.parametrize('dtn', DTN)
@pytest.mark.parametrize('key', list(E.PATCH))
def test_patch_rows_second_trip(key, dtn):
    """4 205 568 runs against 4 194 304 threads: the 4-wide stores (ps = 4) and the store8 path (ps = 8) in both row orders, ldr =
    K + 8 and 4 guard rows."""
    from vtx import ops
    c = E.patch_rows_case(key, dtn)
    clip = dev(c.clip)
    _launch(c, lambda buf: ops.call('vtx_patch_rows', ops._DT[c.dt], c.B, c.T, c.C, c.H, c.W, c.ps, c.ts, ops.ptr(clip), _at(buf), c.ld,
                                    int(c.frame_major), ops.stream()))


def test_patch_rows_u8_second_trip():
    """fp32 rows of the uint8 gather against ToTensor + Normalize + the oracle's gather on the CPU."""
    from vtx import ops
    c = E.patch_rows_u8_case()
    clip = dev(c.clip)
    _launch(c, lambda buf: ops.call('vtx_patch_rows_u8', ops._DT[F32], c.B, c.T, c.H, c.W, c.ps, c.ts, ops.ptr(clip), F3(*E.MEAN), F3(*E.STD),
                                    _at(buf), c.ld, int(c.frame_major), ops.stream()))


# ------------------------------------------------------------------------------------------------------ mix.hip
@pytest.mark.parametrize('frame_major', [False, True], ids=['token-major', 'frame-major'])
def test_mixed_gather_second_trip(frame_major):
    """vtx_patch_rows_mix_u8 at B = 4, T = 6, 1184^2, ps = 4 (4 205 568 items) into sentinel rows with 4 guard rows: bit for bit
    the float route on the device -- the CPU-normalised clip, vtx_mixup_batch, vtx_patch_rows -- in fp32 and bf16."""
    from vtx import _lib, ops
    g = E.MIX
    _, _, M, K = E.mix_tail(frame_major)
    u8 = E.mix_clip()
    clip = u8.to(DEV)
    xf = E.normalised(u8).to(DEV)
    ops.mixup_batch_(xf.view(g['B'], -1, g['H'], g['W']), g['lam'])
    lam, oml = float(np.float32(g['lam'])), float(np.float32(1. - g['lam']))
    for dt in (F32, BF16):
        rows = X.sentinel_fill(torch.empty(M + 4, K, dtype=dt, device=DEV))
        _lib.mix_call('vtx_patch_rows_mix_u8', ops._DT[dt], g['B'], g['T'], g['H'], g['W'], g['ps'], g['ts'], ops.ptr(clip), F3(*E.MEAN),
                      F3(*E.STD), lam, oml, ops.ptr(rows), K, int(frame_major), ops.stream())
        ref = ops.patch_rows(xf, dt, g['ps'], g['ts'], frame_major=frame_major)
        torch.cuda.synchronize()
        assert ref.shape == (M, K) and not bool(torch.isnan(ref).any())
        ib = X._INT[dt]
        bad = int((rows[:M].view(ib) != ref.view(ib)).sum())
        report(f'{"FAIL" if bad else "ok  "} exact mixed gather {dt} frame_major={frame_major}: {M * K} elements, {bad} differ')
        assert bad == 0, f'{bad} of {M * K} elements differ from the float route'
        assert X.sentinel_touched(rows[M:]) == 0, 'guard rows written'
        del rows, ref
    assert torch.equal(clip.cpu(), u8), 'the uint8 clip was modified'


def test_cutmix_second_trip():
    """223 pieces per box row, 4 224 512 items: the byte swap on the CPU; column 0 (outside the box) and the guard bytes stay."""
    from vtx import ops
    c = E.cutmix_case()
    n = c.clip.numel()
    buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    clip = buf[:n].view(c.clip.shape)
    clip.copy_(c.clip)
    assert clip.data_ptr() % 16 == 0
    ops.cutmix_batch_u8_(clip, *c.box)
    torch.cuda.synchronize()
    c.compare(clip)
    assert bool((buf[n:] == 0xA5).all()), 'guard bytes written'


# ----------------------------------------------------------------------------------------------------- stem.hip
@pytest.mark.parametrize('dtn', DTN)
def test_im2col_u8_second_trip(dtn):
    """MaskFeat's stem geometry on 2 x 16 x 224^2: 2 809 856 items against 2 097 152 threads, 2 guard rows."""
    from vtx import _lib, ops
    c = E.im2col_u8_case(dtn)
    clip = dev(c.clip)
    _launch(c, lambda buf: _lib.stem_call('vtx_im2col3d_u8', ops._DT[c.dt], c.B, c.T, c.H, c.W, I3(*c.k3), I3(*c.s3), I3(*c.p3), c.Kp,
                                          ops.ptr(clip), F3(*E.MEAN), F3(*E.STD), _at(buf), ops.stream()))


# ------------------------------------------------------------------------------------------------ colour jitter
def _jitter(c):
    from test_gpu_aug import _jit_records
    from vtx import ops
    buf = c.buf.to(DEV)
    jo, jf = _jit_records(c.recs)
    out = ops.clip_jitter_u8_(buf[:c.B], jo, jf)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    return buf


@pytest.mark.parametrize('hw', E.JIT_SHAPES, ids=_hw_id)
def test_jitter_second_trip(hw):
    """20 x 3400: the word path, 2464 pixels behind the first trip of the 64 workgroups; 127 x 131: the byte path, 253 pixels
    behind; 224 x 224: 49 workgroups add to one frame's grey sum.  Contrast first, last and absent and a clip without ops in
    one launch; the tail is bright enough to move the contrast mean; a guard clip behind the last one."""
    c = E.jitter_case(hw)
    c.compare(_jitter(c))


def test_jitter_contract_beyond_65793_pixels():
    """448 x 448: the bytes equal the restatement whose contrast mean is float32(int64 grey sum) / float32(npix), bit for bit.
    torch.mean of the float32 greys is no reference here (its value depends on the summation order).  Measured on the CPU that
    wrote this test (8 threads, and the same with 1): torch.mean differs from the exact-sum mean on 3 of the 8 frames that open
    with contrast, and the two restatements differ on 0 of the 12 frames, 0 bytes -- a mean one ulp off moves a byte only where
    the blend lands within that ulp of an integer.  Each run reports the figures of its own CPU; they are not asserted."""
    c = E.jitter_big_case()
    c.compare(_jitter(c))
    means, of, frames, nbytes = E.jitter_torch_mean_differences(c)
    report(f'jitter 448x448: torch.mean of the float32 greys differs from the exact-sum mean on {means} of {of} frames; the two '
           f'restatements differ on {frames} of 12 frames, {nbytes} bytes')


# -------------------------------------------------------------------------------------------------- RandAugment
def _two_pass(op, hw):
    from vtx import ops
    fn = {'autocontrast': ops.clip_autocontrast_u8_, 'equalize': ops.clip_equalize_u8_}[op]
    for sel in E.SELS:
        c = E.two_pass_case(op, hw, tuple(sel))
        buf = c.buf.to(DEV)
        fn(buf[:3], _i32(sel))
        torch.cuda.synchronize()
        c.compare(buf)


@pytest.mark.parametrize('hw', E.TWO_PASS_SHAPES, ids=_hw_id)
def test_autocontrast_second_trip(hw):
    """224 x 224 (word path) and 47 x 45 (byte path, 67 pixels behind the first trip): the min / max pass makes ragged trips,
    the frames' only minima and maxima lie in the last one.  258 x 256 and 127 x 131: the apply pass crosses its cap of 64 too."""
    _two_pass('autocontrast', hw)


@pytest.mark.parametrize('hw', E.TWO_PASS_SHAPES[:2], ids=_hw_id)
def test_equalize_second_trip(hw):
    """Histogram and apply pass at cap 8: 7 ragged trips at 224 x 224, a second trip of 67 pixels at 47 x 45; the last trip's
    pixels move the table."""
    _two_pass('equalize', hw)


@pytest.mark.parametrize('hw', E.PW_SHAPES, ids=_hw_id)
def test_pointwise_second_trip(hw):
    """840 x 840: the 16-byte path, 4 233 600 bytes per clip against 1024 x 256 x 16; 209 x 211: the byte path, 264 594 bytes."""
    from vtx import ops
    for shift in range(3):
        c = E.pointwise_case(hw, shift)
        buf = c.buf.to(DEV)
        ops.clip_pointwise_u8_(buf[:3], _i32(c.rec))
        torch.cuda.synchronize()
        c.compare(buf)


def test_warp_and_sharpness_at_the_workload_frame():
    """Neither can reach its cap; 224 x 224 for the index arithmetic at the workload's frame: the ten warp cases under the tie
    rule of test_gpu_randaug, the sharpness bit for bit in both signs."""
    from vtx import ops
    hw = (224, 224)
    clip = R.planted_clip(hw, seed=41 + hw[0])
    d = clip.to(DEV)
    far = [1.0, 0.0, 1e9, 0.0, 1.0, 0.0]
    for n, (op, mag) in enumerate(R.signed_cases(hw)):
        m = R.matrix_of(op, mag, hw)
        sel = E.SELS[n % 3]
        got = ops.clip_warp_nearest_u8(d, _f32([m if s else far for s in sel]), _i32(sel)).cpu()
        tie = R.near_tie(*R.warp_coords64(m, hw))
        assert tie.mean() <= R.TIE_SHARE
        for b, s in enumerate(sel):
            if not s:
                assert torch.equal(got[b], clip[b])
                continue
            same = np.all(got[b].numpy() == R.warp_grid_sample(clip[b], m).numpy(), axis=(0, 3))
            assert np.all(same | tie), f'{R.OPS[op]} {mag:+.4f} clip {b}: {int((~same & ~tie).sum())} pixels differ outside ties'
            assert np.all(R.warp_matches(got[b].numpy(), clip[b], m))
    mg = R.magnitudes(hw)[9]
    for n, sel in enumerate(E.SELS):
        fac = [1.0 + mg, 1.0 - mg, 1.0 + mg] if n % 2 == 0 else [1.0 - mg, 1.0 + mg, 1.0 - mg]
        got = ops.clip_sharpness_u8(d, _f32([[r, 1.0 - r] for r in fac]), _i32(sel)).cpu()
        for b, s in enumerate(sel):
            want = R.sharpness(clip[b], fac[b]) if s else clip[b]
            assert torch.equal(got[b], want), f'sharpness sel {sel} clip {b}: {int((got[b] != want).sum())} bytes differ'


# ----------------------------------------------------------------------------------------------------------- HOG
@pytest.mark.parametrize('select', [False, True], ids=['dense', 'selected'])
@pytest.mark.parametrize('path', list(E.HOG_KINDS))
def test_hog_persistent_strip_loop(path, select):
    """More than two trips of the persistent grid (CU count of the device at hand) with a ragged rest, against hog_oracle bit for
    bit: 32 x 32 frames on the three-channel path, 16 x 272 on the wide one.  Random, gradient and constant frames alternate so
    that workgroups take a constant frame's strip right after a busy one: it must come out all zeros.  'selected': an
    out-of-order subset through vtx_hog_fwd_sel; the two frames left out keep their sentinel, as do two guard frames."""
    from vtx import _lib, ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = E.hog_case(path, cus, select)
    H, W = c.hw
    frames = c.frames.to(DEV)
    out = torch.from_numpy(np.full(c.shape, E.SENT_F64, dtype=np.int64)).view(torch.float64).to(DEV)
    table = ops.hog_table(frames.device)
    if select:
        idx = ops.upload_i32(c.sel.tolist(), frames.device)
        _lib.stem_call('vtx_hog_fwd_sel', ops.ptr(frames), c.F, H, W, ops.ptr(idx), c.n, ops.ptr(table), table.numel() * 8, ops.ptr(out),
                       ops.stream())
    else:
        ops.call('vtx_hog_fwd', ops.ptr(frames), c.F, H, W, ops.ptr(table), table.numel() * 8, ops.ptr(out), None, ops.stream())
    torch.cuda.synchronize()
    report(f'hog {path} select={select}: {c.items} strips over {c.grid} workgroups ({cus} CUs), {c.stale} constant strips behind a busy one')
    c.compare(out)
