"""Cases for the SECOND TRIP of every capped grid-stride kernel: builders, the trip table and CPU fault emulations; importable
without a GPU.  No tests here (tests/test_exact_trip_premise.py, tests/test_gpu_exact_trips.py).

Many launchers start at most `cap` workgroups and let the kernel walk the rest of its work in a loop
`for (i = ...; i < total; i += gridDim.x * 256)`.  A case here has more items than cap * 256 threads take in one trip, with a
ragged last trip, a plain CPU reference compared bit for bit, sentinel-filled outputs with guards behind them (in-place kernels:
a guard clip behind the last one), and a tail that MATTERS: beside the expected result every builder produces what a kernel
would give that
  (a) wrote only its first trip -- the tail left as the sentinel, or as the input where the kernel works in place -- and
  (b) for the two-pass kernels, reduced only its first trip (the jitter's grey sum, min / max, the histogram), or everything
      but the ragged last one,
each by restating the kernel's index arithmetic with the loop cut.  The premise tests assert that the case's own comparison
rejects every one of them; that forces planted tails (tail bytes the op changes, a frame's only minimum and maximum in the
tail, a tail whose removal changes the equalize table, a tail bright enough to move the contrast mean).

TRIPS lists, per kernel, the source file, the text of the launcher that sets the cap, the cap and what one thread takes per
trip.  The premise test reads the sources and fails if a listed text is gone, so that a changed cap cannot silently turn these
cases into first-trip tests.

Not run, and why:
  * maxpool, pos_encoding, im2col3d and xattn_reduce of csrc/mvit.hip: cap 65 536 workgroups, the smallest crossing is 16.8 M
    eight-element items (a 0.5 GB output);
  * the warp and the sharpness beyond their cap (2^20 workgroups per frame: a frame of 2^30 pixels, which RA_SHAPE rejects);
    they run at 224 x 224 for the index arithmetic at the workload's frame only;
  * the resampler, the views and the ragged kernels: their grids cover their work without a loop.
"""
import functools
import os
import types

import numpy as np
import torch

import aug_ref as A
import exact as X
import randaug_ref as R

NS = types.SimpleNamespace
F32, BF16 = torch.float32, torch.bfloat16
DTS = {'f32': F32, 'bf16': BF16}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'videotransformer-pytorch_amd', 'csrc')
MEAN, STD = [0.45, 0.456, 0.406], [0.225, 0.224, 0.229]

_EW = 'static inline int grid_for(long work, int block, int cap = 4096) {'
# kernel -> (file, the launcher's text that fixes the cap (every string must occur in the file), cap in workgroups, what a
# thread takes per trip).  One trip = cap * 256 threads.
TRIPS = {
    'cast_from_f32': ('elementwise.hip', (_EW, 'dim3 grid(grid_for((long)n, 256)), block(256);'), 4096, '1 element'),
    'cast_to_f32': ('elementwise.hip', (_EW, 'dim3 grid(grid_for((long)n, 256)), block(256);'), 4096, '1 element'),
    'fact_glue_bwd': ('elementwise.hip', (_EW, 'dim3 grid(grid_for(total, 256)), block(256);'), 4096, '8 columns of a row'),
    'space_grad_prep': ('elementwise.hip', (_EW, 'dim3 grid(grid_for(work, 256)), block(256);'), 4096, '8 columns of a row'),
    'row_scale_copy': ('elementwise.hip', (_EW, 'dim3 grid(grid_for((long)rows * (D / 8), 256)), block(256);'), 4096, '8 columns of a row'),
    'embed_table': ('elementwise.hip', (_EW, 'dim3 grid(grid_for(((long)P * T + 1) * D, 256)), block(256);'), 4096, '1 element'),
    'patch_rows': ('elementwise.hip', ('const long work = (long)B * (T / ts) * (H / ps) * (W / ps) * C * ts * ps;\n  dim3 grid(grid_for(work, 256, 16384)), block(256);',),
                   16384, 'a run of ps pixels'),
    'patch_rows_u8': ('elementwise.hip', ('const long work = (long)B * (T / ts) * (H / ps) * (W / ps) * ts * ps;\n  dim3 grid(grid_for(work, 256, 16384)), block(256);',),
                      16384, 'a run of ps pixels x 3 channels'),
    'patch_rows_mix_u8': ('mix.hip', ('dim3 grid(grid_for(work, 16384)), block(256);',), 16384, 'a run of ps pixels x 3 channels of both partners'),
    'cutmix_batch_u8': ('mix.hip', ('dim3(grid_for((long)(B / 2) * T * (yh - yl) * pieces, 16384))',), 16384, 'a 16-byte piece of a box row, both partners'),
    'im2col3d_u8': ('stem.hip', ('const dim3 grid(grid_for(total, 8192)), block(256);',), 8192, '8 columns of a row'),
    'clip_jitter': ('aug.hip', ('const int per = vec ? 1024 : 256;', 'if (gx > 64) gx = 64;'), 64, '4 pixels (word path) or 1 (byte path), per frame'),
    'clip_minmax': ('randaug.hip', ('const long per = vec ? 1024 : 256;', 'dim3 grid1(groups(npix, vec, 8), (unsigned)(B * T))'), 8, '4 pixels or 1, per frame'),
    'clip_autocontrast': ('randaug.hip', ('const long per = vec ? 1024 : 256;', 'grid(groups(npix, vec, 64), (unsigned)(B * T));'), 64, '4 pixels or 1, per frame'),
    'clip_equalize': ('randaug.hip', ('const long per = vec ? 1024 : 256;', '  dim3 grid(groups(npix, vec, 8), (unsigned)(B * T));\n  if (vec) {\n    hipLaunchKernelGGL(clip_hist_kernel<true>'),
                      8, '4 pixels or 1, per frame (histogram and apply pass)'),
    'clip_pointwise': ('randaug.hip', ('long g = ((vec ? n / 16 : n) + 255) / 256;', 'if (g > 1024) g = 1024;'), 1024, '16 bytes or 1, per clip'),
    'clip_warp_sharpness': ('randaug.hip', ('dim3 grid(groups(npix, vec, 1L << 20), (unsigned)(B * T));',), 1 << 20, '4 pixels or 1, per frame (never reached)'),
    'hog': ('hog_kernel.h', ('long per_cu = (long)(160 * 1024) / (long)lds; if (per_cu < 1) per_cu = 1;', 'const long wave_cap = 32 / (4 * cp); if (per_cu > wave_cap) per_cu = wave_cap;',
                             'long grid = per_cu * device_cus(); if (grid > items) grid = items;'), None, 'a strip of 8 rows, one workgroup'),
}


def trip(kernel):
    return TRIPS[kernel][2] * 256


def crossing(kernel, items):
    """(threads of a trip, items of the ragged last trip); asserts that the loop makes a second trip."""
    t = trip(kernel)
    assert items > t, f'{kernel}: {items} items fit the first trip of {t}'
    return t, items - (items - 1) // t * t


# --------------------------------------------------------------------------------- out-of-place kernels: one sentinel buffer
def _sent(dt):
    return X.SENT_BF16 if dt == BF16 else X.SENT_F32


def _out(name, v, dt):
    """float64 expected values -> the stored dtype (exact in it: asserted)."""
    if dt == BF16:
        return X.expect_bf16(name, v, 'exact')
    X.assert_fp32_exact(name, v)
    return v.float()


def _case(name, dt, numel, views, expected, tail, check=None, **kw):
    """A case whose outputs live in ONE flat sentinel-filled buffer of `numel` elements.  views: {label: (offset, shape,
    stride)} of the compared regions, expected: {label: CPU tensor}; everything else in the buffer is guard.  tail: the flat
    element offsets that the items behind the first trip write."""
    labels = list(views)

    def view(buf, k):
        off, shape, stride = views[k]
        return buf.as_strided(shape, stride, buf.storage_offset() + off)

    def blank(device='cpu'):
        return X.sentinel_fill(torch.empty(numel, dtype=dt, device=device))

    def full_expected():
        buf = blank()
        for k in labels:
            view(buf, k).copy_(expected[k])
        return buf

    def first_trip_only():
        buf = full_expected()
        buf.view(X._INT[dt])[tail] = _sent(dt)
        return buf

    def guards(buf):
        buf = buf.detach().cpu()
        m = torch.ones(numel, dtype=torch.bool)
        for k in labels:
            view(m, k).fill_(False)
        return {'outside the output': buf[m]}

    def compare(buf):
        """buf: the whole buffer after the launch (device or CPU)."""
        g = guards(buf)
        for i, k in enumerate(labels):
            (check or X.check_exact)(f'{name} {k}', view(buf.detach().cpu(), k), expected[k], g if i == 0 else ())
        return True

    written = torch.zeros(numel, dtype=torch.bool)
    for k in labels:
        view(written, k).fill_(True)
    assert bool(written[tail].all()) and len(torch.unique(tail)) == len(tail), f'{name}: the tail offsets leave the output'
    return NS(name=name, dt=dt, numel=numel, views=views, view=view, blank=blank, expected=expected, tail=tail,
              full_expected=full_expected, emus={'first trip only': first_trip_only}, compare=compare, **kw)


def _rows8_tail(first, items, per, ld, rowmap=None):
    """Element offsets of items [first, items) of a kernel whose item idx writes columns (idx % per) * 8 .. + 8 of row idx / per
    (physical row rowmap(row)) of a buffer with leading dimension ld."""
    idx = torch.arange(first, items)
    row, c = idx // per, (idx % per) * 8
    if rowmap is not None:
        row = rowmap(row)
    return ((row * ld + c)[:, None] + torch.arange(8)[None]).reshape(-1)


def _cast_check(name, got, want, guards=()):
    """test_gpu_exact_arith._check_cast with the guard regions: bit equality except that a NaN only has to stay a NaN."""
    got = got.detach().cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f'{name}: NaN positions differ'
    ib = X._INT[got.dtype]
    X.check_exact(f'{name} (bit patterns)', got.view(ib)[~nan], want.view(ib)[~nan], guards)


CAST_N = 1052673                                   # 4096 * 256 + 4097


@functools.lru_cache(maxsize=None)
def cast_case(kind):
    """cast_from_f32 / cast_to_f32 over CAST_N elements with 64 guard elements behind: the special patterns of
    test_gpu_exact_arith._f32_specials (every bf16 pattern for cast_to_f32) repeated, the hand-made ones again in the tail."""
    from test_gpu_exact_arith import _f32_specials
    t, ragged = crossing(f'cast_{kind}', CAST_N)
    assert ragged % 256 and CAST_N % 256
    if kind == 'from_f32':
        f = _f32_specials()
        src = f.repeat(CAST_N // f.numel() + 1)[:CAST_N].clone()
        src[t:] = f[:CAST_N - t]                                     # the 519 hand-made patterns open the tail
        want, dt = src.to(BF16), BF16
    else:
        pat = (torch.arange(CAST_N, dtype=torch.int64) + (0x7F80 - 2048 - t)) & 0xFFFF        # the tail straddles +Inf / the NaNs
        src = (pat - ((pat >= 0x8000).long() << 16)).to(torch.int16).view(BF16)
        want, dt = src.float(), F32
    assert bool(torch.isnan(want[t:]).any()) and bool(torch.isinf(want[t:]).any()) and bool((want[t:] == 0).any())
    return _case(f'cast_{kind} n={CAST_N}', dt, CAST_N + 64, {'dst': (0, (CAST_N,), (1,))}, {'dst': want}, torch.arange(t, CAST_N),
                 check=_cast_check, src=src, n=CAST_N)


GLUE = dict(B=2, T=4, P=8192, D=128)


@functools.lru_cache(maxsize=2)
def fact_glue_bwd_case(dtn):
    """dx [(B T), 1 + P, D] = 65 544 rows x 16 items = 1 048 704: the second trip is the last 8 rows.  1 / P = 2^-13 is exact."""
    dt = DTS[dtn]
    B, T, P, D = (GLUE[k] for k in 'BTPD')
    rows, per = B * T * (1 + P), D // 8
    t, ragged = crossing('fact_glue_bwd', rows * per)
    assert ragged % 256 and (rows * per) % 256
    dh = X.ints((B, 1 + T, D), 1, 16, 1.0, 11) * (X.ints((B, 1 + T, D), 0, 1, 1.0, 12) * 2 - 1)
    dx = torch.zeros(B * T, 1 + P, D, dtype=torch.float64)
    dx[:B, 0] = dh[:, 0].double()
    dx[:, 1:] = (dh[:, 1:].double().reshape(B * T, 1, D) / P)
    want = _out('fact_glue_bwd dx', dx, dt)
    n = rows * D
    return _case(f'fact_glue_bwd {dtn}', dt, n + 8 * D, {'dx': (0, (B * T, 1 + P, D), ((1 + P) * D, D, 1))}, {'dx': want},
                 _rows8_tail(t, rows * per, per, D), dh=dh, **GLUE)


@functools.lru_cache(maxsize=2)
def space_grad_prep_case(dtn, seq_major):
    """da [B N + B T, D] with ldda = D + 8 and 4 guard rows: 65 536 token rows, then the 8 cls rows -- which are exactly the
    second trip.  seq_major: the P < 0 form of the entry point (T sequences of P consecutive tokens)."""
    dt = DTS[dtn]
    B, T, P, D = (GLUE[k] for k in 'BTPD')
    N, per, ld = P * T, D // 8, D + 8
    rows = B * N + B * T
    t, ragged = crossing('space_grad_prep', rows * per)
    assert t == B * N * per and ragged == B * T * per
    dout = X.ints((B, 1 + N, D), 1, 8, 1.0, 21) * (X.ints((B, 1 + N, D), 0, 1, 1.0, 22) * 2 - 1)
    s = X.dyadic_scales(B * T, 23, choices=(0.5, 1.0, 2.0))
    n = torch.arange(N)
    seq = n // P if seq_major else n % T
    tok = dout[:, 1:].double() * s.double().reshape(B, T)[:, seq][:, :, None]
    cls = dout[:, :1].double() * s.double().reshape(B, T, 1) / T
    want = _out('space_grad_prep', torch.cat([tok.reshape(B * N, D), cls.reshape(B * T, D)]), dt)
    return _case(f'space_grad_prep {dtn} seq_major={seq_major}', dt, (rows + 4) * ld, {'da': (0, (rows, D), (ld, 1))}, {'da': want},
                 _rows8_tail(t, rows * per, per, ld), dout=dout, s=s, ld=ld, seq_major=seq_major, **GLUE)


RSC = dict(B=3, P=5462, T=4, D=128)


@functools.lru_cache(maxsize=2)
def row_scale_copy_case(dtn):
    """65 544 logical rows through the token map into [B, 1 + N, D + 8] (cls rows and pad columns are guards), scale index
    rs = (N, T, T, 1): s[(m / N) T + m % T]."""
    dt = DTS[dtn]
    B, P, T, D = (RSC[k] for k in 'BPTD')
    N, per, ld = P * T, D // 8, D + 8
    M = B * N
    assert M == 65544
    t, ragged = crossing('row_scale_copy', M * per)
    assert ragged % 256 and (M * per) % 256
    src = X.ints((M, D), 1, 16, 1.0, 31) * (X.ints((M, D), 0, 1, 1.0, 32) * 2 - 1)
    s = X.dyadic_scales(B * T, 33, choices=(0.5, 1.0, 2.0))
    m = torch.arange(M)
    want = _out('row_scale_copy', src.double() * s.double()[(m // N) * T + m % T][:, None], dt).reshape(B, N, D)
    views = {'dst': (ld, (B, N, D), ((1 + N) * ld, ld, 1))}
    return _case(f'row_scale_copy {dtn}', dt, B * (1 + N) * ld, views, {'dst': want},
                 _rows8_tail(t, M * per, per, ld, rowmap=lambda r: r + r // N + 1), src=src, s=s, ld=ld, N=N, M=M, **RSC)


EMB = dict(P=196, T=8, D=768)


@functools.lru_cache(maxsize=4)
def embed_table_case(dtn, frame_major):
    """TimeSformer-B's table: (P T + 1) D = 1 204 992 elements, the cls row the last item.  E and cls_row share one buffer with
    64 guard elements behind each."""
    dt = DTS[dtn]
    P, T, D = (EMB[k] for k in 'PTD')
    total = (P * T + 1) * D
    t, _ = crossing('embed_table', total)
    bias, pos = X.ints((D,), -32, 32, 1.0, 41), X.ints((1 + P, D), -32, 32, 1.0, 42)
    te, cls = X.ints((T, D), -32, 32, 1.0, 43), X.ints((D,), -32, 32, 1.0, 44)
    ref = (bias.double() + pos.double()[1:, None, :] + te.double()[None]).expand(P, T, D)
    ref = (ref.transpose(0, 1) if frame_major else ref).reshape(P * T, D)
    cls_off = P * T * D + 64
    idx = torch.arange(t, total)
    tail = torch.where(idx < P * T * D, idx, idx - P * T * D + cls_off)
    return _case(f'embed_table {dtn} frame_major={frame_major}', dt, cls_off + D + 64,
                 {'E': (0, (P * T, D), (D, 1)), 'cls_row': (cls_off, (D,), (1,))},
                 {'E': _out('embed_table', ref, dt), 'cls_row': _out('embed_table cls', cls.double() + pos.double()[0], dt)}, tail,
                 bias=bias, pos=pos, te=te, cls=cls, cls_off=cls_off, frame_major=frame_major, **EMB)


# ---- the patch gathers
def _oracle_rows(x, ps, ts, frame_major):
    from oracle import vt_oracle as O
    B, T = x.shape[:2]
    Tq = T // ts
    want = O.patch_rows_2d(x, ps) if ts == 1 else O.patch_rows_3d(x, ps, ts)
    Pn, K = want.shape[1], want.shape[2]
    if frame_major:
        return want.reshape(B * Tq * Pn, K)
    return want.reshape(B, Tq, Pn, K).permute(0, 2, 1, 3).reshape(B * Pn * Tq, K)


def patch_run_offsets(idx, B, Tn, C, H, W, ps, ts, frame_major, ldr, u8=False, pair=False):
    """patch_rows_kernel's item -> destination: idx -> (b, tq, ph, c, kt, kh, pw), pw fastest, the run's ps elements at row
    (b, tq, p) or (b, p, tq), column ((c ts + kt) ps + kh) ps.  u8: no c in the index, the run goes to all three channels;
    pair (the mixed gather): b < B / 2, and the same run of clip B - 1 - b."""
    gh, gw = H // ps, W // ps
    Pn, Tq = gh * gw, Tn // ts
    r = idx.clone()
    pw = r % gw; r //= gw
    kh = r % ps; r //= ps
    kt = r % ts; r //= ts
    if not u8:
        c = r % C; r //= C
    ph = r % gh; r //= gh
    tq = r % Tq; r //= Tq
    b = r
    assert int(b.max()) < (B // 2 if pair else B)
    p = ph * gw + pw
    out = []
    for bb in ((b, B - 1 - b) if pair else (b,)):
        row = (bb * Tq + tq) * Pn + p if frame_major else (bb * Pn + p) * Tq + tq
        for cc in (range(3) if u8 else (c,)):
            col = ((cc * ts + kt) * ps + kh) * ps
            out.append((row * ldr + col)[:, None] + torch.arange(ps)[None])
    return torch.cat(out, 1).reshape(-1)


PATCH = {'w4': dict(B=2, T=2, C=3, H=1184, W=1184, ps=4, ts=1, frame_major=False),
         's8-token': dict(B=2, T=4, C=3, H=1184, W=1184, ps=8, ts=2, frame_major=False),
         's8-frame': dict(B=2, T=4, C=3, H=1184, W=1184, ps=8, ts=2, frame_major=True)}


def patch_rows_case(key, dtn):
    """vtx_patch_rows at 4 205 568 runs (one trip: 4 194 304): integers within +-128 (bf16 keeps them), rows with ldr = K + 8 and
    4 guard rows.  'w4': ps = 4, the 4-wide stores; 's8-*': ps = 8, ldr % 8 == 0, the store8 path in both row orders."""
    dt = DTS[dtn]
    g = PATCH[key]
    B, T, C, H, W, ps, ts, fm = (g[k] for k in ('B', 'T', 'C', 'H', 'W', 'ps', 'ts', 'frame_major'))
    items = B * (T // ts) * (H // ps) * (W // ps) * C * ts * ps
    t, _ = crossing('patch_rows', items)
    clip = torch.randint(-128, 129, (B, T, C, H, W), generator=X.gen(51 + ps), dtype=torch.int16).float()
    want = _oracle_rows(clip, ps, ts, fm).to(dt)
    M, K = want.shape
    ld = K + 8
    assert (ps == 8) == (ld % 8 == 0 and ps % 8 == 0)
    tail = patch_run_offsets(torch.arange(t, items), B, T, C, H, W, ps, ts, fm, ld)
    return _case(f'patch_rows {key} {dtn}', dt, (M + 4) * ld, {'rows': (0, (M, K), (ld, 1))}, {'rows': want}, tail, clip=clip, ld=ld,
                 M=M, K=K, items=items, **g)


def normalised(u8):
    """ToTensor + Normalize of the reference on a uint8 [B,T,H,W,3] clip -> float [B,T,3,H,W] (as test_gpu_mix restates them)."""
    x = u8.permute(0, 1, 4, 2, 3).float().div(255)
    return x.sub(torch.tensor(MEAN).view(1, 1, 3, 1, 1)).div(torch.tensor(STD).view(1, 1, 3, 1, 1)).contiguous()


PATCH_U8 = dict(B=2, T=6, C=3, H=1184, W=1184, ps=4, ts=1, frame_major=False)


def patch_rows_u8_case():
    """vtx_patch_rows_u8, fp32 rows, 4 205 568 runs: ToTensor + Normalize + the oracle's gather on the CPU."""
    g = PATCH_U8
    B, T, H, W, ps, ts, fm = (g[k] for k in ('B', 'T', 'H', 'W', 'ps', 'ts', 'frame_major'))
    items = B * (T // ts) * (H // ps) * (W // ps) * ts * ps
    t, _ = crossing('patch_rows_u8', items)
    u8 = torch.randint(0, 256, (B, T, H, W, 3), generator=X.gen(61), dtype=torch.uint8)
    want = _oracle_rows(normalised(u8), ps, ts, fm)
    M, K = want.shape
    ld = K + 8
    tail = patch_run_offsets(torch.arange(t, items), B, T, 3, H, W, ps, ts, fm, ld, u8=True)
    return _case('patch_rows_u8 f32', F32, (M + 4) * ld, {'rows': (0, (M, K), (ld, 1))}, {'rows': want}, tail, clip=u8, ld=ld, M=M, K=K,
                 items=items, **g)


MIX = dict(B=4, T=6, H=1184, W=1184, ps=4, ts=1, lam=0.3)


def mix_tail(frame_major):
    """(items, element offsets of the items behind the first trip, rows M, K) of the mixed gather at MIX, ldr = K."""
    g = MIX
    items = (g['B'] // 2) * g['T'] * (g['H'] // 4) * (g['W'] // 4) * 4
    t, _ = crossing('patch_rows_mix_u8', items)
    K = 48
    M = g['B'] * g['T'] * (g['H'] // 4) * (g['W'] // 4)
    return items, patch_run_offsets(torch.arange(t, items), g['B'], g['T'], 3, g['H'], g['W'], 4, 1, frame_major, K, u8=True, pair=True), M, K


def mix_clip():
    g = MIX
    return torch.randint(0, 256, (g['B'], g['T'], g['H'], g['W'], 3), generator=X.gen(71), dtype=torch.uint8)


CUTMIX = dict(B=2, T=16, H=1184, W=1184, box=(0, 1184, 1, 1184))


def swap_reference(u8, box):
    """mixup.py:109 on the [B,T,3,H,W] permutation of the clip: x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]."""
    yl, yh, xl, xh = box
    out = u8.clone()
    out[:, :, yl:yh, xl:xh] = u8.flip(0)[:, :, yl:yh, xl:xh]
    return out


def cutmix_case():
    """vtx_cutmix_batch_u8 at 223 pieces per box row, 4 224 512 items; the clip is 16-byte aligned (the test asserts it), so
    piece k of a row covers row bytes [16 k - first, 16 k - first + 16), first = (offset of the box row) & 15.  Emulation: the
    pieces of the items behind the first trip are not swapped.  Column 0 lies outside the box and must stay."""
    g = CUTMIX
    B, T, H, W = (g[k] for k in 'BTHW')
    yl, yh, xl, xh = g['box']
    u8 = torch.randint(0, 256, (B, T, H, W, 3), generator=X.gen(81), dtype=torch.uint8)
    want = swap_reference(u8, g['box'])
    n, bh = (xh - xl) * 3, yh - yl
    pieces = (n + 15) // 16 + 1
    items = (B // 2) * T * bh * pieces
    t, _ = crossing('cutmix_batch_u8', items)
    assert pieces == 223 and items == 4224512

    def first_trip_only():
        emu = want.clone()
        r = torch.arange(t, items)
        k = r % pieces; r //= pieces
        y = yl + r % bh; r //= bh
        tt = r % T; r //= T
        b = r
        row_bytes, per_clip = W * 3, T * H * W * 3
        off = ((b * T + tt) * H + y) * row_bytes + xl * 3
        dist = (B - 1 - 2 * b) * per_clip
        lo = 16 * k - (off & 15)
        j = lo[:, None] + torch.arange(16)[None]
        ok = (j >= 0) & (j < n)
        pa = (off[:, None] + j)[ok]
        pc = pa + dist[:, None].expand_as(j)[ok]
        fe, fi = emu.view(-1), u8.view(-1)
        fe[pa], fe[pc] = fi[pa], fi[pc]
        return emu

    def compare(got):
        got = got.detach().cpu()
        assert torch.equal(got, want), f'cutmix: {int((got != want).sum())} bytes differ'
        assert torch.equal(got[:, :, :, 0], u8[:, :, :, 0]), 'cutmix: a byte outside the box changed'
        return True

    return NS(name='cutmix_batch_u8', clip=u8, want=want, emus={'first trip only': first_trip_only}, compare=compare, items=items, **g)


STEM = dict(k3=(3, 7, 7), s3=(2, 4, 4), p3=(1, 3, 3), B=2, T=16, H=224, W=224, Kp=448)


@functools.lru_cache(maxsize=1)
def _stem_ref():
    import exact_pool as P
    g = STEM
    u8 = torch.randint(0, 256, (g['B'], g['T'], g['H'], g['W'], 3), generator=X.gen(91), dtype=torch.uint8)
    return u8, P.im2col_ref(normalised(u8), (g['k3'], g['s3'], g['p3'], 3, None, g['Kp']))


def im2col_u8_case(dtn):
    """vtx_im2col3d_u8 at MaskFeat's geometry on 2 x 16 x 224^2: 50 176 rows x 56 items = 2 809 856 (one trip: 2 097 152); against
    pad + unfold of the CPU-normalised clip (exact_pool.im2col_ref, the reference of test_gpu_stem_u8), bf16 rounded once."""
    dt = DTS[dtn]
    u8, want = _stem_ref()
    M, Kp = want.shape
    items = M * (Kp // 8)
    t, ragged = crossing('im2col3d_u8', items)
    assert M == 50176 and items == 2809856 and ragged % 256 == 0 and ragged != t
    return _case(f'im2col3d_u8 {dtn}', dt, (M + 2) * Kp, {'rows': (0, (M, Kp), (Kp, 1))}, {'rows': want.to(dt)},
                 _rows8_tail(t, items, Kp // 8, Kp), check=_bits_check, clip=u8, M=M, **STEM)


def _bits_check(name, got, want, guards=()):
    ib = X._INT[got.dtype]
    X.check_exact(name + ' (bit patterns)', got.contiguous().view(ib), want.contiguous().view(ib), guards)


# ------------------------------------------------------------------------------------------- in-place uint8 clip kernels
GUARD_BYTE = 0xA5


def _with_guard(clip):
    """[B, ...] -> [B + 1, ...]: a guard clip of 0xA5 behind the last one (the kernel is launched on buf[:B])."""
    return torch.cat([clip, torch.full_like(clip[:1], GUARD_BYTE)])


def _clip_compare(name, want):
    """want: the whole expected buffer, guard clip included; compared clip by clip, as the existing tests do."""
    def compare(got):
        got = got.detach().cpu()
        B = want.shape[0] - 1
        for b in range(B):
            assert torch.equal(got[b], want[b]), f'{name} clip {b}: {int((got[b] != want[b]).sum())} bytes differ'
        assert torch.equal(got[B], want[B]), f'{name}: the guard clip behind the last one was written'
        return True
    return compare


def per_trip(hw):
    """(word path?, pixels one workgroup takes per trip) of the per-frame kernels of aug.hip and randaug.hip."""
    vec = (hw[0] * hw[1]) % 4 == 0
    return vec, 1024 if vec else 256


# ---- colour jitter
JIT_SHAPES = [(20, 3400), (127, 131), (224, 224)]
JIT_RECS = [((1, 0, 2), (1.4, 0.6, 1.3)), ((0, 2, 1), (1.3, 0.7, 1.4)), ((0, 2), (0.6, 1.4)), ((), ())]     # contrast first, last, absent; no op


def jitter_emu(frames, jit_ops, factors, sum_px=None, write_px=None):
    """The two kernels of vtx_clip_jitter_u8 on uint8 [T,H,W,3]: the contrast mean is float32(integer grey sum) / float32(npix)
    with the sum taken over the frame's first sum_px pixels only (None: all), and only the first write_px pixels are written
    back (None: all)."""
    img = frames.permute(0, 3, 1, 2).contiguous()
    T, _, H, W = img.shape
    npix = H * W
    for op, f in zip(jit_ops, factors):
        if op == 0:
            img = A._blend(img, torch.zeros_like(img), f)
        elif op == 1:
            grey = A._grey(img).to(torch.int64).reshape(T, npix)
            s = grey[:, :sum_px].sum(1)
            assert int(grey.sum(1).max()) < 2 ** 24, 'a grey sum reaches 2^24: torch.mean of the float32 greys is no reference'
            mean = (s.to(torch.float32) / torch.tensor(float(npix), dtype=torch.float32)).view(T, 1, 1, 1)
            img = A._blend(img, mean, f)
        else:
            img = A._blend(img, A._grey(img), f)
    out = img.permute(0, 2, 3, 1).contiguous()
    if write_px is not None:
        out.view(T, npix, 3)[:, write_px:] = frames.reshape(T, npix, 3)[:, write_px:]
    return out


def jitter_clip(hw, planted=True):
    """[4, 2, H, W, 3]: body bytes 0 .. 120, the pixels behind the first trip of the 64 workgroups (where the grid covers the
    frame: the last 1024 pixels) 200 .. 240 -- bright enough to move the contrast mean, and every grey sum below 2^24."""
    H, W = hw
    npix = H * W
    _, per = per_trip(hw)
    first = 64 * per if npix > 64 * per else npix - 1024
    g = X.gen(101 + H)
    clip = torch.randint(0, 121, (len(JIT_RECS), 2, npix, 3), generator=g, dtype=torch.uint8)
    if planted:
        clip[:, :, first:] = torch.randint(200, 241, (len(JIT_RECS), 2, npix - first, 3), generator=g, dtype=torch.uint8)
    return clip.view(len(JIT_RECS), 2, H, W, 3), first


@functools.lru_cache(maxsize=None)
def jitter_case(hw, planted=True):
    """One launch of vtx_clip_jitter_u8 over the four records.  Expected: aug_ref.jitter_ref (torch.mean of the float32 greys: every
    grey sum is an integer below 2^24 -- asserted in jitter_emu -- so its value does not depend on the summation order).
    Emulations: 'first trip only' (apply pass), 'first-trip sum' (sum pass; at 224 x 224, where 49 workgroups share a frame's sum
    and none makes a second trip: the sum of workgroup 0 alone)."""
    clip, first = jitter_clip(hw, planted)
    B = clip.shape[0]
    npix = hw[0] * hw[1]
    _, per = per_trip(hw)
    crosses = npix > 64 * per
    want = torch.stack([A.jitter_ref(clip[b], *JIT_RECS[b]) for b in range(B)])
    assert torch.equal(want, torch.stack([jitter_emu(clip[b], *JIT_RECS[b]) for b in range(B)]))
    assert torch.equal(want, torch.stack([A.jitter_ref(clip[b], *JIT_RECS[b], exact_mean=True) for b in range(B)]))
    assert torch.equal(want[3], clip[3])
    emus = {'first-trip sum': torch.stack([jitter_emu(clip[b], *JIT_RECS[b], sum_px=first if crosses else per) for b in range(B)])}
    if crosses:
        emus['first trip only'] = torch.stack([jitter_emu(clip[b], *JIT_RECS[b], write_px=first) for b in range(B)])
    full = _with_guard(want)
    return NS(name=f'jitter {hw}', hw=hw, buf=_with_guard(clip), B=B, recs=JIT_RECS, want=full, crosses=crosses, first=first,
              emus={k: _with_guard(v) for k, v in emus.items()}, affected={'first-trip sum': (0, 1), 'first trip only': (0, 1, 2)},
              compare=_clip_compare(f'jitter {hw}', full))


BIG_HW = (448, 448)


@functools.lru_cache(maxsize=1)
def jitter_big_case():
    """448 x 448 (200 704 pixels, TimeSformer's other supported frame): above 65 793 pixels the grey sum passes 2^24, the float32
    torch.mean depends on its summation order and is no reference; the kernel's contract is the exact integer sum, rounded to
    float32 and divided once -- aug_ref.jitter_ref(exact_mean=True)."""
    g = X.gen(111)
    clip = torch.randint(0, 256, (3, 4) + BIG_HW + (3,), generator=g, dtype=torch.uint8)
    recs = JIT_RECS[:2] + [((1,), (1.4,))]
    want = torch.stack([A.jitter_ref(clip[b], *recs[b], exact_mean=True) for b in range(3)])
    full = _with_guard(want)
    return NS(name='jitter 448x448', buf=_with_guard(clip), B=3, recs=recs, want=full, compare=_clip_compare('jitter 448x448', full))


def jitter_torch_mean_differences(c):
    """On this CPU: (frames of the clips that open with contrast whose float32 torch.mean differs from the exact-sum mean, how
    many such frames there are, frames and bytes of the whole case that differ between the two restatements).  A mean one ulp
    off moves a byte only where the blend lands within that ulp of an integer, so few bytes differ, if any."""
    B = c.B
    first = [b for b in range(B) if c.recs[b][0][:1] == (1,)]
    grey = torch.stack([A._grey(c.buf[b].permute(0, 3, 1, 2)) for b in first])
    exact = grey.to(torch.int64).sum(dim=(-3, -2, -1)).to(torch.float32) / torch.tensor(float(grey[0, 0].numel()), dtype=torch.float32)
    means = int((torch.mean(grey.to(torch.float32), dim=(-3, -2, -1)) != exact).sum())
    tm = torch.stack([A.jitter_ref(c.buf[b], *c.recs[b]) for b in range(B)])
    d = tm != c.want[:B]
    return means, exact.numel(), int(d.flatten(2).any(2).sum()), int(d.sum())


# ---- RandAugment: two-pass ops
SELS = [[1, 1, 0], [0, 1, 1], [1, 0, 1]]
TWO_PASS_SHAPES = [(224, 224), (47, 45), (258, 256), (127, 131)]


def tail_start(hw):
    """First pixel of the ragged last trip of the cap-8 kernels (min / max, histogram, equalize)."""
    _, per = per_trip(hw)
    t8 = 8 * per
    npix = hw[0] * hw[1]
    assert npix > t8 and npix % t8
    return (npix - 1) // t8 * t8


@functools.lru_cache(maxsize=None)
def planted_tail_clip(hw, planted=True):
    """randaug_ref.planted_clip plus planted tails (pixels from tail_start on): frame [0,1] (values 100 .. 110) gets a tail drawn
    from 90 .. 99 with one pixel of 120; the random frames [2,0] and [2,1] get a body within 45 .. 220 and a tail drawn from
    0 .. 39 with one pixel of 250 ([2,0] keeps its constant green channel).  So each of these frames has its only minimum and
    maximum in the tail, and a tail whose removal from the histogram moves the equalize table."""
    clip = R.planted_clip(hw, seed=41 + hw[0])
    if not planted:
        return clip
    H, W = hw
    ts_ = tail_start(hw)
    n = H * W - ts_
    g = X.gen(500 + H)
    f = clip[0, 1].view(H * W, 3)
    f[ts_:] = torch.randint(90, 100, (n, 3), generator=g, dtype=torch.uint8)
    f[ts_ + n // 2] = 120
    for t in (0, 1):
        f = clip[2, t].view(H * W, 3)
        f[:ts_] = f[:ts_].clamp(45, 220)
        f[ts_:] = torch.randint(0, 40, (n, 3), generator=g, dtype=torch.uint8)
        f[ts_ + n // 3] = 250
    clip[2, 0, :, :, 1] = 77
    return clip


def autocontrast_emu(frames, mm_px=None, write_px=None):
    """clip_minmax_kernel + clip_autocontrast_kernel on uint8 [T,H,W,3]: min / max over the first mm_px pixels, the first
    write_px pixels written."""
    T, H, W, _ = frames.shape
    x = frames.reshape(T, H * W, 3)
    lo, hi = x[:, :mm_px].amin(1, keepdim=True).float(), x[:, :mm_px].amax(1, keepdim=True).float()
    flat = hi <= lo
    sc = torch.where(flat, torch.ones_like(lo), torch.tensor(255.0) / (hi - lo))
    lo = torch.where(flat, torch.zeros_like(lo), lo)
    out = ((x.float() - lo) * sc).clamp(0, 255).to(torch.uint8)
    if write_px is not None:
        out[:, write_px:] = x[:, write_px:]
    return out.view(T, H, W, 3)


def equalize_emu(frames, hist_px=None, write_px=None):
    """clip_hist_kernel + clip_equalize_kernel on uint8 [T,H,W,3]: the histogram over the first hist_px pixels (the kernel's
    `last` is the count of the bin whose prefix sum reaches npix, 0 if none does), the first write_px pixels written."""
    T, H, W, _ = frames.shape
    npix = H * W
    x = frames.reshape(T, npix, 3)
    out = x.clone()
    for t in range(T):
        for c in range(3):
            hist = torch.bincount(x[t, :hist_px, c].long(), minlength=256)
            cum = torch.cumsum(hist, 0)
            reach = (cum == npix).nonzero()
            last = int(hist[int(reach[0])]) if len(reach) else 0
            step = (npix - last) // 255
            if step == 0:
                continue
            lut = torch.cat([torch.zeros(1, dtype=torch.long), (cum[:-1] + step // 2) // step]).clamp(max=255).to(torch.uint8)
            out[t, :write_px, c] = lut[x[t, :write_px, c].long()]
    return out.view(T, H, W, 3)


_TWO_PASS = {'autocontrast': (R.autocontrast, autocontrast_emu, 64), 'equalize': (R.equalize, equalize_emu, 8)}


@functools.lru_cache(maxsize=None)
def _two_pass_refs(op, hw, planted):
    ref, emu, cap = _TWO_PASS[op]
    clip = planted_tail_clip(hw, planted)
    _, per = per_trip(hw)
    npix = hw[0] * hw[1]
    want = [ref(clip[b]) for b in range(3)]
    for b in range(3):
        assert torch.equal(emu(clip[b]), want[b]), f'{op} {hw}: the restatement of the kernel differs from the reference'
    emus = {'first-trip reduction': [emu(clip[b], 8 * per) for b in range(3)],
            'reduction without the last trip': [emu(clip[b], tail_start(hw)) for b in range(3)]}
    if npix > cap * per:
        emus['first trip only'] = [emu(clip[b], None, cap * per) for b in range(3)]
    return clip, want, emus


def two_pass_case(op, hw, sel, planted=True):
    """vtx_clip_autocontrast_u8 / vtx_clip_equalize_u8 on the planted clip under one sel pattern."""
    clip, want, emus = _two_pass_refs(op, hw, planted)
    pick = lambda per_clip: _with_guard(torch.stack([per_clip[b] if s else clip[b] for b, s in enumerate(sel)]))
    full = pick(want)
    name = f'{op} {hw} sel {sel}'
    return NS(name=name, hw=hw, buf=_with_guard(clip), B=3, sel=list(sel), want=full, emus={k: pick(v) for k, v in emus.items()},
              compare=_clip_compare(name, full))


# ---- RandAugment: pointwise ops
PW_SHAPES = [(840, 840), (209, 211)]
PW_RECS = [[1, 7], [2, 179], [0, 0]]


@functools.lru_cache(maxsize=None)
def pointwise_clip(hw):
    """planted_clip with the bytes behind the first trip of the 1024 workgroups (per clip: T H W 3 bytes) odd and >= 181:
    posterize to 7 bits and solarize at 179 both change every one of them."""
    clip = R.planted_clip(hw, seed=41 + hw[0])
    n = clip[0].numel()
    vec = n % 16 == 0
    first = 1024 * 256 * (16 if vec else 1)
    assert n > first and (n - first) % 256 and (vec or n % 256), (n, first)
    tail = torch.randint(181, 256, (3, n - first), generator=X.gen(600 + hw[0]), dtype=torch.uint8) | 1
    clip.view(3, n)[:, first:] = tail
    return clip, first


def pointwise_case(hw, shift):
    clip, first = pointwise_clip(hw)
    rec = PW_RECS[shift:] + PW_RECS[:shift]
    n = clip[0].numel()

    def ref(b):
        op, arg = rec[b]
        return clip[b] if op == 0 else R.posterize(clip[b], arg) if op == 1 else R.solarize(clip[b], 178.5)
    want = torch.stack([ref(b) for b in range(3)])
    emu = want.clone()
    emu.view(3, n)[:, first:] = clip.view(3, n)[:, first:]
    full = _with_guard(want)
    name = f'pointwise {hw} {rec}'
    return NS(name=name, hw=hw, buf=_with_guard(clip), B=3, rec=rec, want=full, emus={'first trip only': _with_guard(emu)},
              processed=[b for b in range(3) if rec[b][0]], compare=_clip_compare(name, full))


# ------------------------------------------------------------------------------------------------------------ HOG
MI355X_CUS = 256
HOG_KINDS = {'3ch': (32, 32), 'wide': (16, 272)}
SENT_F64 = 0x7FF8A5A5A5A5A5A5


def hog_grid(W, cus, items):
    """hog_launch: the persistent grid (workgroups per CU: LDS- and wave-limited)."""
    cp = 3 if W <= 256 else 1
    lds = 4096 * 4 + 30 * W + cp * 8 * W * 8 + cp * (W // 8) * 18 * 4 + (W // 8) * 27 * 8
    per_cu = max(160 * 1024 // lds, 1)
    per_cu = min(per_cu, 32 // (4 * cp))
    return min(per_cu * cus, items), per_cu


def _hog_frame(kind, hw, seed):
    H, W = hw
    if kind == 'rand':
        return torch.randint(0, 256, (H, W, 3), generator=X.gen(seed), dtype=torch.uint8)
    if kind == 'grad':
        y, x, c = torch.arange(H).view(H, 1, 1), torch.arange(W).view(1, W, 1), torch.arange(3).view(1, 1, 3)
        return ((x * (7 + seed % 5) + y * (3 + seed % 7) + 40 * c + seed) % 256).to(torch.uint8)
    return torch.full((H, W, 3), (seed * 37) % 256, dtype=torch.uint8)


def hog_case(path, cus=MI355X_CUS, select=False):
    """HOG over more strips than the persistent grid takes in two trips.  Frames cycle through D distinct ones -- random, a planted
    gradient, constant, ... -- so the oracle runs D times; D is chosen so that workgroups meet a constant frame right after a
    busy one (asserted): its strips must come out all zeros, whatever `hist` / `mag` / `msk` held from the strip before.
    select: an out-of-order subset (all frames but two) through vtx_hog_fwd_sel; the rows of the two others keep the sentinel.
    Emulations: 'first trip only' (strips behind the first trip left as sentinel) and 'stale hist' (a constant frame's strip
    behind the first trip repeats what its workgroup wrote one trip earlier)."""
    from oracle import hog_oracle
    hw = HOG_KINDS[path]
    H, W = hw
    strips = H // 8
    F = cus + 3 if path == '3ch' else 4 * cus + 3
    assert F * strips > (2 * (2 * cus) if path == '3ch' else 8 * cus)
    if select:
        order = torch.randperm(F, generator=X.gen(7))
        sel = order[(order != 5) & (order != F - 2)]
    else:
        sel = torch.arange(F)
    n = len(sel)
    items = n * strips
    grid, per_cu = hog_grid(W, cus, items)
    assert items > 2 * grid and items % grid, f'hog {path}: {items} strips against {grid} workgroups'
    item = torch.arange(items)
    f_of = sel[item // strips]
    for D in (7, 8, 10, 11, 13):
        kinds = [('rand', 'grad', 'const')[i % 3] for i in range(D)]
        const = torch.tensor([k == 'const' for k in kinds])[f_of % D]
        later = item >= grid
        stale = later & const & ~const[(item - grid).clamp(min=0)]
        if int(stale.sum()) >= 8 and int((later & ~const & const[(item - grid).clamp(min=0)]).sum()) >= 8:
            break
    else:
        raise AssertionError(f'hog {path}: no cycle puts a constant frame behind a busy one')
    distinct = torch.stack([_hog_frame(kinds[i], hw, 900 + i) for i in range(D)])
    feats = torch.from_numpy(np.stack([hog_oracle.extract_hog_features(distinct[i].numpy()) for i in range(D)]))
    for i in range(D):
        assert (kinds[i] == 'const') == bool((feats[i] == 0).all())
    frames = distinct[torch.arange(F) % D].contiguous()
    shape = (F + 2, H // 16, W // 16, 108)
    want = torch.from_numpy(np.full(shape, SENT_F64, dtype=np.int64)).view(torch.float64)
    want[sel] = feats[sel % D]

    def cut(which):
        emu = want.clone()
        fi, cr = f_of[which], (item % strips)[which]
        for f, c, i in zip(fi.tolist(), cr.tolist(), item[which].tolist()):
            dst = emu[f, c >> 1, :, (c & 1) * 54:(c & 1) * 54 + 54]
            if which is stale:
                j = i - grid
                pf, pc = int(f_of[j]), int(j % strips)
                dst.copy_(want[pf, pc >> 1, :, (pc & 1) * 54:(pc & 1) * 54 + 54])
            else:
                dst.fill_(float('nan'))
        return emu

    def compare(got):
        got = got.detach().cpu()
        bad = got.view(torch.int64) != want.view(torch.int64)
        assert not bool(bad[:F].any()), (f'hog {path}: {int(bad[:F].sum())} values differ from the oracle (or, on frames not selected, '
                                         f'from the sentinel), first at {bad.nonzero()[0].tolist()}')
        assert not bool(bad[F:].any()), f'hog {path}: the guard frames behind the last one were written'
        return True

    return NS(name=f'hog {path} select={select}', hw=hw, F=F, frames=frames, sel=sel, n=n, items=items, grid=grid, per_cu=per_cu, D=D,
              kinds=kinds, want=want, shape=shape, stale=int(stale.sum()), compare=compare,
              emus={'first trip only': lambda: cut(later), 'stale hist': lambda: cut(stale)})
