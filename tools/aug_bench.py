"""Clip augmentation on the device (csrc/aug.hip): time of the resampler and the colour jitter for one training batch --
96 clips of 8 frames, 256x340 -> 224x224, bicubic, every clip with its own crop, flip and three colour ops.  GPU box only.

    python tools/aug_bench.py [--clips 96] [--frames 8] [--step-ms MS] [--out profiles/clip_aug_bench.txt]

HIP events around `--iters` back-to-back launches per round, after a warm-up; `--rounds` rounds, median and minimum.  The
source clips rotate through `--sets` buffers (together larger than the 256 MiB Infinity Cache) so that reads come from HBM
as they do behind a data loader.  Bytes = what the algorithm has to move (source read + result written; the jitter: the
clip read once for the grey sums and read + written by the blend), held against the 8 TB/s DESIGN.md uses for the other
byte-bound kernels.  --step-ms: the `ms_per_step` of `bench.py --gpus 1` at the same number of clips, for the share of
the training step (not measured here).

    python tools/aug_bench.py --randaug [--step-ms MS] [--out profiles/clip_randaug_bench.txt]

times the RandAugment kernels (csrc/randaug.hip) at 96 clips x 8 frames x 224x224 with every clip selected, one launch of the
single-op jitter as the same-run yardstick, and the whole ClipAugment(auto_augment=True) call from 256x340 sources.  Beside
each time: the bytes the op has to move and the rate the jitter reached in profiles/clip_aug_bench.txt.

    python tools/aug_bench.py --views [--out profiles/clip_views_bench.txt]

times the test-time views (csrc/views.hip): 32 clips, 8 of 32 decoded frames each, 256x340 -> 3 x 224x224 (ClipTest: Resize(256) +
ThreeCrop, bilinear), `vtx.ops.clip_views_u8` against the composition the other kernels offer for the same bytes -- index_select
of the frames, three `clip_resample_u8` passes, one stacking copy -- in alternating rounds of the same run, after checking that
both give the same bytes.  256x340 sources make Resize(256) the identity, so a second block repeats it from 240x320 sources
(-> 256x341, a real resize).

    python tools/aug_bench.py --mix [--out profiles/clip_mix_bench.txt]

times Mixup / CutMix on uint8 clips (csrc/mix.hip) at 96 clips x 8 frames x 224x224, patch 16, bf16 rows: (a) the mixing gather
`vtx_patch_rows_mix_u8`, (b) the plain gather `vtx_patch_rows_u8` on the same clips (the floor), (c) the float route -- normalise
with torch, `ops.mixup_batch_`, `ops.patch_rows` -- after checking that (a) and (c) give the same rows; and `cutmix_batch_u8_`
for a half-area box against `ops.cutmix_batch_` on the float batch.  All paths in alternating rounds of one run.

    python tools/aug_bench.py --stem [--out profiles/stem_u8_bench.txt]

times MaskFeat's input path from uint8 clips (csrc/stem.hip) at 32 clips x 16 frames x 224x224, bf16 rows: (a) the stem gather
`vtx_im2col3d_u8` against `vtx_im2col3d` on a float clip that is already there (the bar: not slower, within that kernel's spread
over the rounds) and against the route it replaces, torch normalise + `vtx_im2col3d`; (b) `vtx.hog_targets` with three centre
frames per clip against index_select + `ops.hog_fwd` + scatter into a zeroed target.  Both pairs are checked for equal results
first; all paths in alternating rounds of one run.

    python tools/aug_bench.py --ragged [--out profiles/clip_ragged_bench.txt]

times a batch of clips that differ in source size (csrc/ragged.hip): 32 clips, 8 of 32 decoded frames each, sizes mixed over 256x340,
340x256, 240x320 and 360x480, ClipEval(224) (Resize(256) + centre crop, bicubic): (a) one call on the list, (b) what there was before
it -- 32 one-clip calls and a torch.cat --, (c) a uniform [B,Ts,331,320,3] batch of the same total bytes through `vtx_clip_views_u8`,
the kernel-rate yardstick, and (d) that uniform batch given as a list, i.e. through `vtx_clips_views_u8`: the same work as (c) plus
one descriptor read per workgroup.  (a) and (b) are checked for equal bytes first, (c) and (d) likewise; all paths in alternating
rounds of one run; per path the device time (HIP events around the calls of a round), the host clock around the same calls ending
in a synchronise, and the resampling kernel alone (a pair of HIP events around each launch, in rounds of its own).

    python tools/aug_bench.py --yuv [--parent-lib PATH/libvtx_ragged.so] [--out profiles/clip_yuv_bench.txt]

times the batch of --ragged given as decoded 4:2:0 planes (csrc/yuv.hip; NV12, the matrix of an untagged stream): (a) `vtx_clips_views_u8`
on RGB clips converted beforehand -- what a loader pays for today behind a CPU colour conversion --, (b) `vtx_yuv420_to_rgb_u8` on every
clip and then (a), (c) `vtx_clips_views_yuv420` on the planes.  --parent-lib: a libvtx_ragged.so built at the parent commit, timed as (p)
on the same RGB clips in the same alternating rounds: its device code is this commit's, so (p) and (a) must agree within (p)'s own
spread.  (a), (b) and (c) are checked for equal bytes first.  Per path the kernels alone (HIP events around each launch), the whole
call (host clock around `ClipEval` on the list, ending in a synchronise) and the bytes its kernels have to move.

    python tools/aug_bench.py --yuv10 [--out profiles/clip_yuv10_bench.txt]

times the same batch given as decoded 10-bit planes (csrc/yuv10.hip): `vtx_clips_views_yuv10` on (P) P010 clips, (L) yuv420p10le clips and
(M) a list that alternates P010 clips with NV12 ones, against (a) `vtx_clips_views_yuv420` on the same content as NV12 (the samples without
their two low bits), (b) `vtx_clips_views_u8` on RGB clips converted beforehand and (c) `vtx_yuv10_to_rgb_u8` on every decoded frame and
then (b).  (P), (L), (b) and (c) are checked for equal bytes first, the halves of (M) against (P) and (a).  Columns as for --yuv, and the
bytes a caller uploads per batch for each form.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'videotransformer-pytorch_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402
import vtx  # noqa: E402,F401
from vtx import aug, ops  # noqa: E402

HBM = 8.0e12


def timed(fn, iters, rounds, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for r in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(r * iters + i)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)          # us per call
    return out


#: why a kernel moves fewer bytes per second than the streaming jitter pass (from its code; none of these was profiled)
RANDAUG_WHY = {
    'vtx_clip_warp_nearest_u8': 'a gather: three single-byte loads per pixel at computed addresses, 13 float32 operations and two integer '
                                'divisions per pixel for the coordinate',
    'vtx_clip_sharpness_u8': 'a 3x3 stencil: 15 word loads (three rows, overlapping the neighbour threads\' words), 18 column sums and an '
                             'integer division by 13 per byte for four pixels',
    'vtx_clip_pointwise_u8': '',
    'vtx_clip_autocontrast_u8': 'two passes and two workspace memsets in one call; pass 1 ends in six single-lane integer atomics per wave',
    'vtx_clip_equalize_u8 (smooth)': 'as above, and neighbouring pixels of a smooth frame add to the same few LDS bins',
    'vtx_clip_equalize_u8': 'one LDS atomic per byte in pass 1 (neighbouring pixels hit the same bins), and every workgroup of pass 2 '
                            'rebuilds three 256-entry tables (16 barriers) before it touches a pixel; the table look-up is one LDS byte read per byte',
}


def jitter_yardstick(path):
    """TB/s of vtx_clip_jitter_u8 in profiles/clip_aug_bench.txt, or None."""
    import re
    try:
        for ln in open(path):
            m = re.match(r'vtx_clip_jitter_u8\s.*?([0-9.]+) TB/s', ln)
            if m:
                return float(m.group(1))
    except OSError:
        pass
    return None


def randaug_main(a):
    import time
    import numpy as np
    dev = 'cuda:0'
    B, T, S = a.clips, a.frames, a.size
    Hs, Ws = a.src
    g = torch.Generator().manual_seed(0)
    clips = [torch.randint(0, 256, (B, T, S, S, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(a.sets)]
    outs = [torch.empty_like(c) for c in clips]
    srcs = [torch.randint(0, 256, (B, T, Hs, Ws, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(a.sets)]
    mags = aug._randaug_magnitudes((S, S), 9, 31)
    f32 = lambda x: torch.tensor(np.asarray(x, dtype=np.float64)).float().to(dev)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    sel = i32([1] * B)
    geo = [(1 + b % 5, mags[1 + b % 5] * (1 if b % 2 else -1)) for b in range(B)]            # all five geometric ops, both signs
    theta = f32([aug.randaug_theta(op, m, S, S) for op, m in geo])
    sharp = f32([[1.0 + mags[9], 1.0 - (1.0 + mags[9])]] * B)
    pw = i32([[1, 7] if b % 2 else [2, 179] for b in range(B)])
    jo = i32([[1, 0, 0, 0]] * B)
    jf = f32([[1.0 + mags[6], 0, 0, 1.0 - (1.0 + mags[6]), 0, 0]] * B)
    n = clips[0].numel()
    k = a.sets
    # frames as a camera gives them, for the histogram's LDS atomics: a ramp with two bits of noise, so neighbours share bins
    ramp = ((torch.arange(S).view(S, 1) + torch.arange(S).view(1, S)) // 2 % 252).to(torch.uint8)
    smooth = [(ramp.view(1, 1, S, S, 1) + torch.randint(0, 4, (B, T, S, S, 3), generator=g, dtype=torch.uint8)).to(dev) for _ in range(k)]
    spare = [torch.empty_like(c) for c in smooth]

    def equalize_smooth(i):
        spare[i % k].copy_(smooth[i % k])                  # equalize is in place and would flatten the ramp: a fresh copy each time
        ops.clip_equalize_u8_(spare[i % k], sel)
    runs = [
        ('vtx_clip_warp_nearest_u8', lambda i: ops.clip_warp_nearest_u8(clips[i % k], theta, sel, out=outs[i % k]), 2 * n, 'read + write'),
        ('vtx_clip_sharpness_u8', lambda i: ops.clip_sharpness_u8(clips[i % k], sharp, sel, out=outs[i % k]), 2 * n, 'read + write'),
        ('vtx_clip_pointwise_u8', lambda i: ops.clip_pointwise_u8_(clips[i % k], pw), 2 * n, 'read + write'),
        ('vtx_clip_autocontrast_u8', lambda i: ops.clip_autocontrast_u8_(clips[i % k], sel), 3 * n, 'min/max pass: read; apply: read + write'),
        ('vtx_clip_equalize_u8', lambda i: ops.clip_equalize_u8_(clips[i % k], sel), 3 * n + 2 * B * T * 768 * 4,
         'histogram pass: read; apply: read + write; histograms written and read'),
        ('copy (torch)', lambda i: spare[i % k].copy_(smooth[i % k]), 2 * n, 'the copy inside the row below'),
        ('vtx_clip_equalize_u8 (smooth)', equalize_smooth, 5 * n + 2 * B * T * 768 * 4, 'a copy of ramp frames (read + write), then as above'),
        ('vtx_clip_jitter_u8 (1 op)', lambda i: ops.clip_jitter_u8_(clips[i % k], jo, jf), 2 * n, 'brightness alone: read + write (same-run yardstick)'),
    ]
    yard = jitter_yardstick(os.path.join(ROOT, 'profiles', 'clip_aug_bench.txt'))
    lines = [f'RandAugment kernels, {B} clips x {T} frames x {S}x{S}, every clip selected; {torch.cuda.get_device_name(0)}',
             f'{a.rounds} rounds of {a.iters} launches after {a.warmup} warm-up launches, HIP events; {a.sets} clip sets of '
             f'{n / 2**20:.0f} MiB in rotation (together larger than the 256 MiB Infinity Cache)',
             'yardstick: vtx_clip_jitter_u8 in profiles/clip_aug_bench.txt (three ops, sum pass + blend pass): '
             + (f'{yard:.2f} TB/s' if yard else 'not found'),
             'clips are uniform random bytes unless a row says otherwise (the least contended case for the histogram); rates above HBM speed: part of a '
             'set is still in the Infinity Cache',
             '']
    total = {}
    for name, fn, nbytes, what in runs:
        us = timed(fn, a.iters, a.rounds, a.warmup)
        med, lo = statistics.median(us), min(us)
        rate = nbytes / med / 1e6
        total[name] = med
        rel = f' = {rate / yard:4.2f} x the jitter\'s rate' if yard else ''
        lines.append(f'{name:<27} median {med:8.1f} us  min {lo:8.1f} us  floor {nbytes / 1e6:6.1f} MB ({what}) = {nbytes / HBM * 1e6:5.1f} us at 8 TB/s  '
                     f'{rate:5.2f} TB/s{rel}')
        why = RANDAUG_WHY.get(name, '')
        if yard and rate < 0.5 * yard and why:
            lines.append(f'{"":<27} below half the yardstick; expected cause (from the code, not profiled): {why}')
    whole = aug.ClipAugment(img_size=S, auto_augment=True)
    for i in range(2):
        whole(srcs[i % k], generator=g)
    torch.cuda.synchronize()
    host = []
    for i in range(a.rounds):
        t0 = time.perf_counter()
        whole(srcs[i % k], generator=g)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    lines.append('')
    lines.append(f'ClipAugment(auto_augment=True).__call__  median {statistics.median(host):8.2f} ms  min {min(host):8.2f} ms  host clock, synchronised, '
                 f'{Hs}x{Ws} -> {S}x{S} bicubic: {B} draws, {2 * B} tables, one upload, the resampler and the RandAugment launches of two slots')
    if a.step_ms:
        worst = max(v for n_, v in total.items() if n_ in RANDAUG_WHY and '(' not in n_)
        lines.append(f'training step (bench.py --gpus 1 --batch {B}, same run): {a.step_ms:.1f} ms -> the whole call is '
                     f'{statistics.median(host) / a.step_ms * 100:.2f} % of the step; the slowest RandAugment kernel on all {B} clips {worst / (a.step_ms * 1e3) * 100:.2f} %')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


def views_main(a):
    import numpy as np
    dev = 'cuda:0'
    B, Ts, T, S, k = a.clips, a.decoded, a.frames, a.size, a.sets
    t = aug.ClipTest(img_size=S, short_side=a.short_side)
    g = torch.Generator().manual_seed(0)
    lines = [f'test-time views, {B} clips, {T} of {Ts} decoded frames each, ClipTest({S}, short_side={a.short_side}), bilinear, antialias off; '
             f'{torch.cuda.get_device_name(0)}',
             f'{a.rounds} rounds of {a.iters} calls per path, the two paths in alternating rounds of one run, after {a.warmup} warm-up calls each, HIP events; '
             f'{k} source sets in rotation (together larger than the 256 MiB Infinity Cache)',
             'bytes = what each path has to move, whole source frames counted (the rows outside the crop window are never read by either); '
             'spread = (max - min) / median over the rounds',
             '']
    shapes = [tuple(a.src)] + ([(240, 320)] if tuple(a.src) == (256, 340) else [])
    for Hs, Ws in shapes:
        srcs = [torch.randint(0, 256, (B, Ts, Hs, Ws, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(k)]
        frames = np.stack([aug.sample_frames(Ts, T, Ts // T, generator=g) for _ in range(B)]).astype(np.int32)
        (Hr, Wr), (top, lefts) = t.resized_hw(Hs, Ws), t.offsets(Hs, Ws)
        up = lambda tab: tuple(torch.from_numpy(x).to(dev) for x in tab)
        ytab = up(aug._tables([(Hs, 0, Hs, Hr, False, top, S)] * B, 'bilinear', False))
        xall = up(aug._tables([(Ws, 0, Ws, Wr, False, 0, Wr)] * B, 'bilinear', False))
        xcut = [up(aug._tables([(Ws, 0, Ws, Wr, False, l, S)] * B, 'bilinear', False)) for l in lefts]
        fdev = torch.from_numpy(frames).to(dev)
        ldev = torch.tensor([lefts] * B, dtype=torch.int32, device=dev)
        flat = (torch.arange(B).view(B, 1) * Ts + torch.from_numpy(frames).long()).reshape(-1).to(dev)
        out = torch.empty(B, 3, T, S, S, 3, dtype=torch.uint8, device=dev)

        def one_launch(i):
            return ops.clip_views_u8(srcs[i % k], fdev, ldev, S, xall, ytab, out=out)

        def composition(i):
            sel = srcs[i % k].view(B * Ts, Hs, Ws, 3).index_select(0, flat).view(B, T, Hs, Ws, 3)
            return torch.stack([ops.clip_resample_u8(sel, (S, S), x, ytab) for x in xcut], dim=1)
        same = torch.equal(one_launch(0), composition(0))
        assert same, 'clip_views_u8 and the composition differ'
        for i in range(a.warmup):
            one_launch(i)
            composition(i)
        torch.cuda.synchronize()
        new, old = [], []
        for r in range(a.rounds):                              # alternating: what else runs on the machine hits both alike
            for fn, acc in ((one_launch, new), (composition, old)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.iters):
                    fn(r * a.iters + i)
                e1.record()
                e1.synchronize()
                acc.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        fr, src_b, view_b = B * T, Hs * Ws * 3, 3 * S * S * 3
        new_bytes = fr * (src_b + view_b)
        old_bytes = fr * (2 * src_b + 3 * src_b + view_b + 2 * view_b)
        lines.append(f'{Hs}x{Ws} -> {Hr}x{Wr} -> 3 x {S}x{S}, rows from {top}, columns from {lefts}: {len(set(c for l in lefts for c in range(l, l + S)))} of {Wr} '
                     f'columns in a view, {3 * S} stored; source set {srcs[0].numel() / 2**20:.0f} MiB; same bytes from both paths: {same}')

        def row(name, us, nbytes, what):
            med, lo, hi = statistics.median(us), min(us), max(us)
            lines.append(f'{name:<34} median {med:8.1f} us  min {lo:8.1f}  max {hi:8.1f}  spread {100 * (hi - lo) / med:4.1f} %  {nbytes / 1e6:7.1f} MB ({what})  {nbytes / med / 1e6:5.2f} TB/s '
                         f'= {nbytes / (med * 1e-6) / HBM:5.3f} of 8 TB/s')
            return med
        m_new = row('vtx_clip_views_u8', new, new_bytes, 'selected frames read, three views written')
        m_old = row('index_select + 3 resample + stack', old, old_bytes, 'gather: read + write; three passes: frame read, view written; stack: read + write')
        lines.append(f'one launch / composition: {m_new / m_old:.3f} of the time, {new_bytes / old_bytes:.3f} of the bytes'
                     + ('' if m_new <= m_old else '   <-- the one launch is SLOWER than the composition it replaces'))
        lines.append('')
        del srcs
    text = '\n'.join(lines)
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


def mix_main(a):
    dev = 'cuda:0'
    B, T, S, k, ps = a.clips, a.frames, a.size, a.sets, 16
    mean, std = [0.45, 0.456, 0.406], [0.225, 0.224, 0.229]
    lam = 0.3
    g = torch.Generator().manual_seed(0)
    clips = [torch.randint(0, 256, (B, T, S, S, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(k)]
    n = clips[0].numel()
    m_dev = torch.tensor(mean, device=dev).view(1, 1, 3, 1, 1)
    s_dev = torch.tensor(std, device=dev).view(1, 1, 3, 1, 1)
    c255 = torch.tensor(255.0, device=dev)                   # a device tensor: a true division, not a product with 1/255
    xf = torch.empty(B, T, 3, S, S, dtype=torch.float32, device=dev)

    def normalise(i, out=xf):
        out.copy_(clips[i % k].permute(0, 1, 4, 2, 3))        # uint8 channels-last -> float32 planes in one pass
        return out.div_(c255).sub_(m_dev).div_(s_dev)

    def fused(i):
        return ops.patch_rows(ops.MixedClip(clips[i % k], lam), torch.bfloat16, ps, 1, frame_major=False)

    def plain(i):
        return ops.patch_rows(clips[i % k], torch.bfloat16, ps, 1, frame_major=False)

    def today(i):
        x = normalise(i)
        ops.mixup_batch_(x.view(B, -1, S, S), lam)
        return ops.patch_rows(x, torch.bfloat16, ps, 1, frame_major=False)
    floats = [normalise(i, torch.empty_like(xf)) for i in range(k)]

    def today_mix_and_gather(i):                               # without the normalisation: 8 + 6 bytes per sample
        x = floats[i % k]
        ops.mixup_batch_(x.view(B, -1, S, S), lam)
        return ops.patch_rows(x, torch.bfloat16, ps, 1, frame_major=False)
    box = (33, 191, 35, 194)                                   # 158 x 159 of 224 x 224: half the area, no edge on a 4-byte boundary
    if S != 224:
        box = (S // 7, S // 7 + int(S * 0.7071), S // 6, S // 6 + int(S * 0.7071))
    box_samples = B * T * (box[1] - box[0]) * (box[3] - box[2]) * 3

    def cut_u8(i):
        return ops.cutmix_batch_u8_(clips[i % k], *box)

    def cut_f32(i):
        return ops.cutmix_batch_(floats[i % k].view(B, -1, S, S), *box)

    vtx.set_input_normalization(mean, std)
    # the same rows?  exactly, on four clips normalised on the CPU (the reference's ToTensor + Normalize), and on the whole batch
    # normalised by the torch expression that is timed
    small = clips[0][[0, 1, B - 2, B - 1]].contiguous()
    xs = small.cpu().permute(0, 1, 4, 2, 3).float().div(255)
    xs = xs.sub(torch.tensor(mean).view(1, 1, 3, 1, 1)).div(torch.tensor(std).view(1, 1, 3, 1, 1)).contiguous().to(dev)
    ops.mixup_batch_(xs.view(4, -1, S, S), lam)
    same = {}
    for dt_ in (torch.float32, torch.bfloat16):
        same[dt_] = torch.equal(ops.patch_rows(ops.MixedClip(small, lam), dt_, ps, 1, frame_major=False), ops.patch_rows(xs, dt_, ps, 1, frame_major=False))
        assert same[dt_], f'vtx_patch_rows_mix_u8 and normalise + mixup_batch_ + patch_rows differ ({dt_})'
    same_dev = torch.equal(fused(0), today(0))
    cut_a = clips[0].clone()
    ops.cutmix_batch_u8_(cut_a, *box)
    cut_b = normalise(0, torch.empty_like(xf))
    ops.cutmix_batch_(cut_b.view(B, -1, S, S), *box)
    same_cut = torch.equal(ops.patch_rows(cut_a, torch.float32, ps, 1, frame_major=False), ops.patch_rows(cut_b, torch.float32, ps, 1, frame_major=False))
    assert same_cut, 'cutmix_batch_u8_ and cutmix_batch_ on the normalised clip give different rows'
    del cut_a, cut_b

    paths = [(fused, []), (plain, []), (today, []), (today_mix_and_gather, []), (cut_u8, []), (cut_f32, [])]
    for i in range(a.warmup):
        for fn, _ in paths:
            fn(i)
    torch.cuda.synchronize()
    for r in range(a.rounds):                                  # alternating: what else runs on the machine hits all alike
        for fn, acc in paths:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.iters):
                fn(r * a.iters + i)
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1) * 1e3 / a.iters)
    vtx.set_input_normalization(None, None)
    lines = [f'Mixup / CutMix on uint8 clips, {B} clips x {T} frames x {S}x{S}, patch {ps}, bf16 rows, lam {lam}; {torch.cuda.get_device_name(0)}',
             f'{a.rounds} rounds of {a.iters} calls per path, the paths in alternating rounds of one run, after {a.warmup} warm-up calls each, HIP events; '
             f'{k} clip sets of {n / 2**20:.0f} MiB in rotation (together larger than the 256 MiB Infinity Cache)',
             f'same rows from (a) and (c): fp32 {same[torch.float32]}, bf16 {same[torch.bfloat16]} on four clips normalised on the host; '
             f'{same_dev} on the whole batch with the torch normalisation timed below; CutMix on bytes = CutMix on floats: {same_cut}',
             'bytes = what each path has to move per sample (one colour value of one pixel), every pass counted once',
             '']
    med = {}

    def row(name, key, us, per_sample, what, samples=n):
        m, lo = statistics.median(us), min(us)
        nbytes = per_sample * samples
        med[key] = m
        lines.append(f'{name:<46} median {m:8.1f} us  min {lo:8.1f} us  {nbytes / 1e6:7.1f} MB ({what})  {nbytes / m / 1e6:5.2f} TB/s')
    row('(a) vtx_patch_rows_mix_u8', 'a', paths[0][1], 3, '1 read + 2 written: one thread serves both clips of a pair')
    row('(b) vtx_patch_rows_u8 (no mixing: the floor)', 'b', paths[1][1], 3, '1 read + 2 written')
    row('(c) torch normalise + mixup_batch_ + patch_rows', 'c', paths[2][1], 5 + 3 * 8 + 8 + 6,
        'copy to float 1 + 4, three in-place passes 3 x 8, mix 4 + 4, gather 4 + 2; one fused normalising pass would make it 19')
    row('    mixup_batch_ + patch_rows alone', 'c2', paths[3][1], 8 + 6, 'mix 4 + 4, gather 4 + 2: (c) with a free normalisation')
    lines.append(f'(a) / (b) = {med["a"] / med["b"]:.3f}   (a) / (c) = {med["a"] / med["c"]:.3f}   (a) / (mix + gather alone) = {med["a"] / med["c2"]:.3f}'
                 + ('' if med['a'] < med['c'] else '   <-- the fused gather is SLOWER than the route it replaces'))
    if med['a'] > 2 * med['b']:
        lines.append('(a) takes more than twice (b).  From the code it has no second read stream (one thread serves both clips of a pair: 1 byte read per '
                     'sample, as (b)) and divides as often per sample as (b): neither of the two explains it')
    elif med['a'] < med['b']:
        lines.append('(a) is below its floor (b): the same bytes and the same two divisions per sample, but patch_rows_u8_kernel (csrc/elementwise.hip, not '
                     'changed here) writes its rows with one 2-byte store per element where (a) stores 16 bytes at a time')
    lines.append('')
    row(f'cutmix_batch_u8_, box {box}', 'ca', paths[4][1], 2, 'both partners read + written, 1 byte each', box_samples)
    row(f'cutmix_batch_ on the float batch, box {box}', 'cb', paths[5][1], 8, 'both partners read + written, 4 bytes each', box_samples)
    lines.append(f'bytes / floats = {med["ca"] / med["cb"]:.3f} of the time, 0.250 of the bytes')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    assert med['a'] < med['c'], 'the fused gather must beat normalise + mix + gather'


def stem_main(a):
    import ctypes as C
    from vtx import _lib
    dev = 'cuda:0'
    B, T, S, k = a.clips, a.frames, a.size, a.sets
    mean, std = [0.45, 0.456, 0.406], [0.225, 0.224, 0.229]
    k3, s3, p3 = (3, 7, 7), (2, 4, 4), (1, 3, 3)
    K = 3 * k3[0] * k3[1] * k3[2]
    Kp = (K + 63) // 64 * 64                                 # ConvStemFn's row width: 448
    To, Ho, Wo = ((n + 2 * p - kk) // s + 1 for n, p, kk, s in zip((T, S, S), p3, k3, s3))
    M = B * To * Ho * Wo
    g = torch.Generator().manual_seed(0)
    clips = [torch.randint(0, 256, (B, T, S, S, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(k)]
    n = clips[0].numel()
    m_dev = torch.tensor(mean, device=dev).view(1, 1, 3, 1, 1)
    s_dev = torch.tensor(std, device=dev).view(1, 1, 3, 1, 1)
    c255 = torch.tensor(255.0, device=dev)                   # a device tensor: a true division, not a product with 1/255
    xf = torch.empty(B, T, 3, S, S, dtype=torch.float32, device=dev)
    rows = torch.empty(M, Kp, dtype=torch.bfloat16, device=dev)
    i3 = lambda t: (C.c_int * 3)(*t)   # noqa: E731
    f3 = lambda t: (C.c_float * 3)(*t)   # noqa: E731
    bf16 = ops._DT[torch.bfloat16]

    def normalise(i, out=xf):
        out.copy_(clips[i % k].permute(0, 1, 4, 2, 3))        # uint8 channels-last -> float32 planes in one pass
        return out.div_(c255).sub_(m_dev).div_(s_dev)
    floats = [normalise(i, torch.empty_like(xf)) for i in range(k)]

    def gather_f32(x, out=rows):
        ops.call('vtx_im2col3d', bf16, B, T, 3, S, S, i3(k3), i3(s3), i3(p3), Kp, ops.ptr(x), ops.ptr(out), ops.stream())
        return out

    def u8(i, out=rows):                                       # (a) the new gather
        _lib.stem_call('vtx_im2col3d_u8', bf16, B, T, S, S, i3(k3), i3(s3), i3(p3), Kp, ops.ptr(clips[i % k]), f3(mean), f3(std), ops.ptr(out),
                       ops.stream())
        return out

    def parent(i):                                             # vtx_im2col3d alone, on a float clip that is already there
        return gather_f32(floats[i % k])

    def today(i):                                              # the route (a) replaces: normalise with torch, then gather
        return gather_f32(normalise(i))

    # the same rows?  on the whole batch, against the torch normalisation that is timed (the suite holds the CPU-normalised form)
    same = torch.equal(u8(0, torch.empty_like(rows)), today(0))
    assert same, 'vtx_im2col3d_u8 and normalise + vtx_im2col3d give different rows'

    # (b) HOG targets: three centre frames per clip
    markers = [[[0, 2], [2, 2], [5, 2]] for _ in range(B)]     # centres 2, 6, 12 at temporal stride 2
    flat = torch.tensor(ops.hog_center_frames(markers, T, 2), dtype=torch.int64, device=dev)
    g16 = S // 16

    def targets_new(i):
        return vtx.hog_targets(clips[i % k], markers)

    def targets_old(i):
        frames = clips[i % k].view(B * T, S, S, 3).index_select(0, flat)
        target = torch.zeros(B * T, g16, g16, 108, dtype=torch.float64, device=dev)
        target.index_copy_(0, flat, ops.hog_fwd(frames))
        return target.view(B, T, g16, g16, 108)
    same_hog = torch.equal(targets_new(0), targets_old(0))
    assert same_hog, 'hog_targets and index_select + hog_fwd + scatter differ'

    paths = [(u8, []), (parent, []), (today, []), (targets_new, []), (targets_old, [])]
    for i in range(a.warmup):
        for fn, _ in paths:
            fn(i)
    torch.cuda.synchronize()
    for r in range(a.rounds):                                  # alternating: what else runs on the machine hits all alike
        for fn, acc in paths:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.iters):
                fn(r * a.iters + i)
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1) * 1e3 / a.iters)
    row_bytes = M * Kp * 2
    lines = [f'MaskFeat from uint8 clips, {B} clips x {T} frames x {S}x{S}, stem kernel {k3} stride {s3} padding {p3}: {M} rows x {Kp} bf16 columns; '
             f'{torch.cuda.get_device_name(0)}',
             f'{a.rounds} rounds of {a.iters} calls per path, the paths in alternating rounds of one run, after {a.warmup} warm-up calls each, HIP events; '
             f'{k} clip sets of {n / 2**20:.0f} MiB (uint8) / {4 * n / 2**20:.0f} MiB (float) in rotation',
             f'same rows from vtx_im2col3d_u8 and torch normalise + vtx_im2col3d on the whole batch: {same}; same targets from both HOG routes: {same_hog}',
             'bytes = what each path has to move, every pass counted once; spread = (max - min) / median over the rounds',
             '']
    med, spread = {}, {}

    def row(name, key, us, nbytes, what):
        m, lo, hi = statistics.median(us), min(us), max(us)
        med[key], spread[key] = m, (hi - lo) / m
        lines.append(f'{name:<44} median {m:8.1f} us  min {lo:8.1f}  max {hi:8.1f}  spread {100 * (hi - lo) / m:4.1f} %  {nbytes / 1e6:7.1f} MB ({what})  '
                     f'{nbytes / m / 1e6:5.2f} TB/s')
    row('(a) vtx_im2col3d_u8', 'a', paths[0][1], n + row_bytes, 'clip bytes read, rows written')
    row('    vtx_im2col3d on a ready float clip', 'p', paths[1][1], 4 * n + row_bytes, 'float clip read, rows written')
    row('    torch normalise + vtx_im2col3d', 't', paths[2][1], (5 + 3 * 8) * n + 4 * n + row_bytes,
        'copy to float 1 + 4, three in-place passes 3 x 8 per sample; then as the row above')
    margin = spread['p'] * med['p']
    verdict = 'not slower' if med['a'] <= med['p'] + margin else 'SLOWER'
    lines.append(f'(a) / parent kernel alone = {med["a"] / med["p"]:.3f}   (a) / the route it replaces = {med["a"] / med["t"]:.3f}   '
                 f'bar: (a) <= parent + its spread = {med["p"]:.1f} + {margin:.1f} us: {verdict}')
    lines.append('')
    sel_bytes = 3 * B * (S * S * 3 + g16 * g16 * 108 * 8)
    tgt_bytes = B * T * g16 * g16 * 108 * 8
    row('(b) vtx.hog_targets, 3 centre frames per clip', 'hn', paths[3][1], tgt_bytes + sel_bytes,
        'target zeroed; selected frames read, their rows written; one index upload')
    row('    index_select + vtx_hog_fwd + scatter', 'ho', paths[4][1], tgt_bytes + sel_bytes + 3 * B * 2 * (S * S * 3 + g16 * g16 * 108 * 8),
        'target zeroed; frames gathered (read + write), HOG, rows scattered (read + write); index already on the device')
    lines.append(f'(b) new / old = {med["hn"] / med["ho"]:.3f}' + ('' if med['hn'] <= med['ho'] else '   <-- hog_targets is SLOWER than the route it replaces'))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


def ragged_main(a):
    import time
    import numpy as np
    dev = 'cuda:0'
    B, Ts, T, S, k = a.clips, a.decoded, a.frames, a.size, a.sets
    sizes = [(256, 340), (340, 256), (240, 320), (360, 480)]
    hw = [sizes[b % 4] for b in range(B)]
    area = sum(h * w for h, w in hw) // B                      # 105920 = 331 x 320 for the four sizes in equal shares
    uni = next(((area // w, w) for w in (320, 256, 384, 300) if area % w == 0), (int(round(area ** 0.5)),) * 2)
    ev = aug.ClipEval(img_size=S)
    g = torch.Generator().manual_seed(0)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)
    lists = [[rnd(Ts, h, w, 3) for h, w in hw] for _ in range(k)]
    unis = [rnd(B, Ts, uni[0], uni[1], 3) for _ in range(k)]
    ulists = [list(u) for u in unis]
    frames = np.stack([aug.sample_frames(Ts, T, Ts // T, generator=g) for _ in range(B)]).astype(np.int32)
    rows = [frames[b:b + 1] for b in range(B)]

    def one_call(i):
        return ev(lists[i % k], frames=frames)

    def per_clip(i):
        return torch.cat([ev(c[None], frames=rows[b]) for b, c in enumerate(lists[i % k])])

    def uniform(i):
        return ev(unis[i % k], frames=frames)

    def uniform_list(i):
        return ev(ulists[i % k], frames=frames)
    same_ab = torch.equal(one_call(0), per_clip(0))
    same_cd = torch.equal(uniform(0), uniform_list(0))
    assert same_ab and same_cd, 'the list call and the per-clip calls differ'
    paths = [('(a) one call on the list', one_call), ('(b) 32 one-clip calls + torch.cat', per_clip),
             ('(c) uniform 5-D batch, vtx_clip_views_u8', uniform), ('(d) the uniform batch as a list', uniform_list)]
    for i in range(a.warmup):
        for _, fn in paths:
            fn(i)
    torch.cuda.synchronize()
    dev_us, wall_us = {n: [] for n, _ in paths}, {n: [] for n, _ in paths}
    for r in range(a.rounds):                                  # alternating: what else runs on the machine hits all alike
        for n, fn in paths:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for i in range(a.iters):
                fn(r * a.iters + i)
            e1.record()
            e1.synchronize()
            wall_us[n].append((time.perf_counter() - t0) * 1e6 / a.iters)
            dev_us[n].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    # the resampling kernel alone: events around every launch (rounds of their own: the events slow the host)
    kern = {n: [] for n, _ in paths}
    for r in range(a.rounds):
        for n, fn in paths:
            ops.profile_start(('clips_views', 'clip_views'))
            for i in range(a.iters):
                fn(r * a.iters + i)
            torch.cuda.synchronize()
            tot = ops.profile_totals(ops.profile_stop())
            kern[n].append(sum(v[1] for v in tot.values()) * 1e3 / a.iters)          # us of kernel time per batch
    sel = B * T
    src_list = T * sum(h * w * 3 for h, w in hw)
    src_uni = sel * uni[0] * uni[1] * 3
    out_b = sel * S * S * 3
    lines = [f'clips of differing source size, {B} clips, {T} of {Ts} decoded frames each, sizes {sizes} in equal shares, ClipEval({S}) '
             f'(Resize({ev.scale_size}) + centre crop), bicubic, antialias off; {torch.cuda.get_device_name(0)}',
             f'{a.rounds} rounds of {a.iters} batches per path, the paths in alternating rounds of one run, after {a.warmup} warm-up batches each; '
             f'{k} source sets of {sum(c.numel() for c in lists[0]) / 2**20:.0f} MiB in rotation (together larger than the 256 MiB Infinity Cache)',
             f'uniform batch of (c), (d): [{B},{Ts},{uni[0]},{uni[1]},3], {unis[0].numel() / 2**20:.0f} MiB per set; same bytes from (a) and (b): {same_ab}; '
             f'from (c) and (d): {same_cd}',
             'device = HIP events around the calls of a round; wall = host clock around the same calls, ending in a synchronise; kernel = HIP events '
             'around each resampling launch, in rounds of their own; all per batch; spread = (max - min) / median over the rounds',
             f'bytes a batch has to move: selected frames read {src_list / 1e6:.1f} MB (list) / {src_uni / 1e6:.1f} MB (uniform), whole frames counted, '
             f'{out_b / 1e6:.1f} MB written',
             '']
    med, spread = {}, {}
    for (n, _), nbytes in zip(paths, (src_list + out_b, src_list + out_b, src_uni + out_b, src_uni + out_b)):
        d, w, kr = dev_us[n], wall_us[n], kern[n]
        md, mw, mk = statistics.median(d), statistics.median(w), statistics.median(kr)
        med[n[:3]], spread[n[:3]] = (md, mw, mk), ((max(d) - min(d)) / md, (max(w) - min(w)) / mw, (max(kr) - min(kr)) / mk)
        lines.append(f'{n:<42} device median {md:8.1f} us  min {min(d):8.1f}  max {max(d):8.1f}  spread {100 * spread[n[:3]][0]:5.1f} %   '
                     f'wall median {mw:8.1f} us  min {min(w):8.1f}  max {max(w):8.1f}  spread {100 * spread[n[:3]][1]:5.1f} %   '
                     f'kernel median {mk:7.1f} us  min {min(kr):7.1f}  max {max(kr):7.1f}  spread {100 * spread[n[:3]][2]:5.1f} %  '
                     f'{nbytes / mk / 1e6:5.2f} TB/s')
    A, Bp, Cc, D = med['(a)'], med['(b)'], med['(c)'], med['(d)']
    gap = Bp[1] - A[1]
    noise = max(spread['(a)'][1] * A[1], spread['(b)'][1] * Bp[1])
    lines.append('')
    lines.append(f'(a) / (b): wall {A[1] / Bp[1]:.3f}, device {A[0] / Bp[0]:.3f}; (b) - (a) = {gap:.1f} us of wall time per batch against a spread of '
                 f'{noise:.1f} us: ' + ('(a) beats (b) by more than the spread' if gap > noise else '(a) does NOT beat (b) by more than the spread'))
    bar = 2 * spread['(c)'][2] * Cc[2]
    lines.append(f'(d) - (c), kernel: {D[2] - Cc[2]:+.1f} us ({D[2] / Cc[2]:.3f}); twice the spread of (c): {bar:.1f} us: '
                 + ('within it' if D[2] - Cc[2] <= bar else 'the ragged kernel is SLOWER than the uniform one by more than that'))
    lines.append(f'(d) - (c), whole call: {D[1] - Cc[1]:+.1f} us of wall time ({D[1] / Cc[1]:.3f}): both calls are bound by the host (wall = device span > kernel), '
                 f'and the list costs per-clip host work the tensor does not -- type, shape, device and contiguity of {B} tensors, {B} data_ptr()')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


def yuv_main(a):
    import time
    import numpy as np
    from vtx import _lib
    dev = 'cuda:0'
    B, Ts, T, S, k = a.clips, a.decoded, a.frames, a.size, a.sets
    sizes = [(256, 340), (340, 256), (240, 320), (360, 480)]
    hw = [sizes[b % 4] for b in range(B)]
    ev = aug.ClipEval(img_size=S)
    g = torch.Generator().manual_seed(0)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)
    yuvs = [[vtx.YUVClip(rnd(Ts, h, w), rnd(Ts, (h + 1) // 2, (w + 1) // 2, 2)) for h, w in hw] for _ in range(k)]
    rgbs = [[ops.yuv420_to_rgb_u8(c) for c in clips] for clips in yuvs]
    frames = np.stack([aug.sample_frames(Ts, T, Ts // T, generator=g) for _ in range(B)]).astype(np.int32)
    this_lib = _lib.load_ragged()
    parent_lib = _lib._bind(a.parent_lib, 'the parent\'s libvtx_ragged.so', _lib.RAGGED_SIGNATURES) if a.parent_lib else None

    def with_lib(lib, fn):
        def run(i):
            _lib._side['ragged'] = lib                         # the binding calls whichever library is loaded under this key
            try:
                return fn(i)
            finally:
                _lib._side['ragged'] = this_lib
        return run

    def rgb_views(i):
        return ev(rgbs[i % k], frames=frames)

    def convert_then_views(i):
        return ev([ops.yuv420_to_rgb_u8(c) for c in yuvs[i % k]], frames=frames)

    def fused(i):
        return ev(yuvs[i % k], frames=frames)
    want = rgb_views(0)
    same = torch.equal(convert_then_views(0), want) and torch.equal(fused(0), want)
    assert same, 'the three routes differ'
    paths = [('(a) vtx_clips_views_u8 on RGB clips', with_lib(this_lib, rgb_views)),
             ('(b) vtx_yuv420_to_rgb_u8 + vtx_clips_views_u8', convert_then_views),
             ('(c) vtx_clips_views_yuv420', fused)]
    if parent_lib is not None:
        assert torch.equal(with_lib(parent_lib, rgb_views)(0), want), 'the parent library gives other bytes'
        paths.insert(0, ('(p) vtx_clips_views_u8 on RGB clips, parent commit', with_lib(parent_lib, rgb_views)))
    for i in range(a.warmup):
        for _, fn in paths:
            fn(i)
    torch.cuda.synchronize()
    wall = {n: [] for n, _ in paths}
    turn = lambda r: paths[r % len(paths):] + paths[:r % len(paths)]   # the order rotates: no path always runs behind the same neighbour
    for r in range(a.rounds):                                  # alternating: what else runs on the machine hits all alike
        for n, fn in turn(r):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.iters):
                fn(r * a.iters + i)
            torch.cuda.synchronize()
            wall[n].append((time.perf_counter() - t0) * 1e6 / a.iters)
    kern = {n: [] for n, _ in paths}                           # events around every launch, in rounds of their own: they slow the host
    for r in range(a.rounds):
        for n, fn in turn(r):
            ops.profile_start(('clips_views', 'clips_views_yuv', 'yuv420_to_rgb'))
            for i in range(a.iters):
                fn(r * a.iters + i)
            torch.cuda.synchronize()
            tot = ops.profile_totals(ops.profile_stop())
            kern[n].append(sum(v[1] for v in tot.values()) * 1e3 / a.iters)
    px_sel = T * sum(h * w for h, w in hw)
    px_all = Ts * sum(h * w for h, w in hw)
    out_b = B * T * S * S * 3
    nbytes = {'(p)': 3 * px_sel + out_b, '(a)': 3 * px_sel + out_b, '(b)': int(1.5 * px_all) + 3 * px_all + 3 * px_sel + out_b,
              '(c)': int(1.5 * px_sel) + out_b}
    what = {'(p)': 'selected RGB frames read, result written', '(a)': 'selected RGB frames read, result written',
            '(b)': f'all {Ts} decoded frames of every clip converted: planes read, RGB written; then as (a)',
            '(c)': 'selected frames of the planes read (1.5 bytes per pixel), result written'}
    lines = [f'decoded 4:2:0 clips (NV12), {B} clips, {T} of {Ts} decoded frames each, sizes {sizes} in equal shares, ClipEval({S}) '
             f'(Resize({ev.scale_size}) + centre crop), bicubic, antialias off; {torch.cuda.get_device_name(0)}',
             f'{a.rounds} rounds of {a.iters} batches per path, the paths in alternating rounds of one run whose order rotates from round to round, after {a.warmup} warm-up batches each; '
             f'{k} source sets in rotation: {sum(c.numel() for c in rgbs[0]) / 2**20:.0f} MiB of RGB and '
             f'{sum(p.numel() for c in yuvs[0] for p in c.planes) / 2**20:.0f} MiB of planes each',
             f'same bytes from (a), (b) and (c): {same}' + ('; (p): the same bytes from the parent library' if parent_lib is not None else ''),
             'kernel = HIP events around each launch of the path, summed per batch, in rounds of their own; wall = host clock around the whole '
             'call (tables, checks, one upload, the launches), ending in a synchronise; all per batch; spread = (max - min) / median over the rounds',
             'bytes = what the kernels of a path have to move, whole frames counted; the upload the caller makes before it is 3 bytes per decoded '
             f'pixel for (a) and 1.5 for (c): {3 * px_all / 1e6:.1f} MB against {1.5 * px_all / 1e6:.1f} MB per batch',
             '']
    med, spread = {}, {}
    for n, _ in paths:
        key, kr, w = n[:3], kern[n], wall[n]
        mk, mw = statistics.median(kr), statistics.median(w)
        med[key], spread[key] = (mk, mw), ((max(kr) - min(kr)) / mk, (max(w) - min(w)) / mw)
        lines.append(f'{n:<52} kernel median {mk:8.1f} us  min {min(kr):8.1f}  max {max(kr):8.1f}  spread {100 * spread[key][0]:5.1f} %   '
                     f'wall median {mw:8.1f} us  min {min(w):8.1f}  max {max(w):8.1f}  spread {100 * spread[key][1]:5.1f} %   '
                     f'{nbytes[key] / 1e6:7.1f} MB ({what[key]})  {nbytes[key] / mk / 1e6:5.2f} TB/s')
    lines.append('')
    if parent_lib is not None:
        d, bar = med['(a)'][0] - med['(p)'][0], spread['(p)'][0] * med['(p)'][0]
        lines.append(f'(a) - (p), kernel: {d:+.1f} us against the parent\'s own spread of {bar:.1f} us: '
                     + ('within it' if abs(d) <= bar else 'OUTSIDE it'))
    d, bar = med['(c)'][0] - med['(a)'][0], spread['(a)'][0] * med['(a)'][0]
    lines.append(f'(c) / (a), kernel: {med["(c)"][0] / med["(a)"][0]:.3f} of the time for {nbytes["(c)"] / nbytes["(a)"]:.3f} of the bytes; (c) - (a) = {d:+.1f} us against a '
                 f'spread of {bar:.1f} us: ' + ('the fused kernel is not slower than the RGB kernel on RGB clips' if d <= bar else
                                                'the fused kernel is SLOWER than the RGB kernel on RGB clips: it moves fewer bytes in more time, so the bytes do not set its time; '
                                                'what it adds per tap is arithmetic (5 integer multiply-adds, 3 shifts, 3 clamps) and a third load stream'))
    lines.append(f'(c) / (b), kernel: {med["(c)"][0] / med["(b)"][0]:.3f}; whole call: (c) / (a) = {med["(c)"][1] / med["(a)"][1]:.3f}, (c) / (b) = {med["(c)"][1] / med["(b)"][1]:.3f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


def yuv10_main(a):
    import time
    import numpy as np
    dev = 'cuda:0'
    B, Ts, T, S, k = a.clips, a.decoded, a.frames, a.size, a.sets
    sizes = [(256, 340), (340, 256), (240, 320), (360, 480)]
    hw = [sizes[b % 4] for b in range(B)]
    ev = aug.ClipEval(img_size=S)
    g = torch.Generator().manual_seed(0)
    rnd = lambda *shape: torch.randint(0, 1024, shape, dtype=torch.int16, device=dev)        # 10-bit samples
    p010s, p10les, nv12s, mixes = [], [], [], []
    for _ in range(k):
        planes = [(rnd(Ts, h, w), rnd(Ts, (h + 1) // 2, (w + 1) // 2, 2)) for h, w in hw]
        msb = lambda p: (p.to(torch.int32) << 6).to(torch.int16)                         # the sample in the upper 10 bits of its word
        p010s.append([vtx.YUVClip(msb(y), msb(uv), depth=10) for y, uv in planes])
        p10les.append([vtx.YUVClip(y, uv[..., 0].contiguous(), uv[..., 1].contiguous(), depth=10) for y, uv in planes])
        nv12s.append([vtx.YUVClip((y >> 2).to(torch.uint8), (uv >> 2).to(torch.uint8)) for y, uv in planes])
        mixes.append([p010s[-1][b] if b % 8 < 4 else nv12s[-1][b] for b in range(B)])    # every size in both depths
    rgbs = [[ops.yuv420_to_rgb_u8(c) for c in clips] for clips in p010s]
    frames = np.stack([aug.sample_frames(Ts, T, Ts // T, generator=g) for _ in range(B)]).astype(np.int32)
    on = lambda lists: (lambda i: ev(lists[i % k], frames=frames))
    paths = [('(P) vtx_clips_views_yuv10 on P010', on(p010s)), ('(L) vtx_clips_views_yuv10 on yuv420p10le', on(p10les)),
             ('(M) vtx_clips_views_yuv10 on P010 and NV12, half each', on(mixes)), ('(a) vtx_clips_views_yuv420 on NV12', on(nv12s)),
             ('(b) vtx_clips_views_u8 on RGB clips', on(rgbs)),
             ('(c) vtx_yuv10_to_rgb_u8 + vtx_clips_views_u8', lambda i: ev([ops.yuv420_to_rgb_u8(c) for c in p010s[i % k]], frames=frames))]
    out = {n[:3]: fn(0) for n, fn in paths}
    same = all(torch.equal(out[n], out['(b)']) for n in ('(P)', '(L)', '(c)'))
    ten = torch.tensor([b % 8 < 4 for b in range(B)], device=dev)
    same_mix = torch.equal(out['(M)'][ten], out['(P)'][ten]) and torch.equal(out['(M)'][~ten], out['(a)'][~ten])
    assert same and same_mix, 'the routes differ'
    del out
    for i in range(a.warmup):
        for _, fn in paths:
            fn(i)
    torch.cuda.synchronize()
    wall = {n: [] for n, _ in paths}
    turn = lambda r: paths[r % len(paths):] + paths[:r % len(paths)]   # the order rotates: no path always runs behind the same neighbour
    for r in range(a.rounds):                                  # alternating: what else runs on the machine hits all alike
        for n, fn in turn(r):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.iters):
                fn(r * a.iters + i)
            torch.cuda.synchronize()
            wall[n].append((time.perf_counter() - t0) * 1e6 / a.iters)
    kern = {n: [] for n, _ in paths}                           # events around every launch, in rounds of their own: they slow the host
    for r in range(a.rounds):
        for n, fn in turn(r):
            ops.profile_start(('clips_views', 'clips_views_yuv', 'clips_views_yuv10', 'yuv10_to_rgb'))
            for i in range(a.iters):
                fn(r * a.iters + i)
            torch.cuda.synchronize()
            tot = ops.profile_totals(ops.profile_stop())
            kern[n].append(sum(v[1] for v in tot.values()) * 1e3 / a.iters)
    px = [h * w for h, w in hw]
    px_sel, px_all = T * sum(px), Ts * sum(px)
    px_ten = T * sum(p for b, p in enumerate(px) if b % 8 < 4)
    out_b = B * T * S * S * 3
    nbytes = {'(P)': 3 * px_sel + out_b, '(L)': 3 * px_sel + out_b, '(M)': 3 * px_ten + int(1.5 * (px_sel - px_ten)) + out_b,
              '(a)': int(1.5 * px_sel) + out_b, '(b)': 3 * px_sel + out_b, '(c)': 3 * px_all + 3 * px_all + 3 * px_sel + out_b}
    what = {'(P)': 'selected frames of the planes read (1.5 samples of 2 bytes per pixel), result written', '(L)': 'as (P)',
            '(M)': 'as (P) for one half of the clips, 1.5 bytes per pixel for the other', '(a)': 'selected frames of the planes read (1.5 bytes per pixel), result written',
            '(b)': 'selected RGB frames read, result written',
            '(c)': f'all {Ts} decoded frames of every clip converted: planes read, RGB written; then as (b)'}
    up_ten = Ts * sum(p for b, p in enumerate(px) if b % 8 < 4)
    lines = [f'decoded 10-bit 4:2:0 clips, {B} clips, {T} of {Ts} decoded frames each, sizes {sizes} in equal shares, ClipEval({S}) '
             f'(Resize({ev.scale_size}) + centre crop), bicubic, antialias off; {torch.cuda.get_device_name(0)}',
             f'{a.rounds} rounds of {a.iters} batches per path, the paths in alternating rounds of one run whose order rotates from round to round, after {a.warmup} warm-up batches each; '
             f'{k} source sets in rotation: {sum(p.numel() * 2 for c in p010s[0] for p in c.planes) / 2**20:.0f} MiB of 10-bit planes, '
             f'{sum(p.numel() for c in nv12s[0] for p in c.planes) / 2**20:.0f} MiB of NV12 planes and {sum(c.numel() for c in rgbs[0]) / 2**20:.0f} MiB of RGB each',
             f'same bytes from (P), (L), (b) and (c): {same}; the 10-bit clips of (M) as in (P), its 8-bit clips as in (a): {same_mix}',
             'kernel = HIP events around each launch of the path, summed per batch, in rounds of their own; wall = host clock around the whole '
             'call (tables, checks, one upload, the launches), ending in a synchronise; all per batch; spread = (max - min) / median over the rounds',
             'bytes = what the kernels of a path have to move, whole frames counted',
             f'upload a caller makes per batch before the call (all {Ts} decoded frames): P010 or yuv420p10le {3 * px_all / 1e6:.1f} MB, the mix '
             f'{(3 * up_ten + 1.5 * (px_all - up_ten)) / 1e6:.1f} MB, NV12 {1.5 * px_all / 1e6:.1f} MB, RGB24 (after a CPU conversion) {3 * px_all / 1e6:.1f} MB',
             '']
    med, spread = {}, {}
    for n, _ in paths:
        key, kr, w = n[:3], kern[n], wall[n]
        mk, mw = statistics.median(kr), statistics.median(w)
        med[key], spread[key] = (mk, mw), ((max(kr) - min(kr)) / mk, (max(w) - min(w)) / mw)
        lines.append(f'{n:<54} kernel median {mk:8.1f} us  min {min(kr):8.1f}  max {max(kr):8.1f}  spread {100 * spread[key][0]:5.1f} %   '
                     f'wall median {mw:8.1f} us  min {min(w):8.1f}  max {max(w):8.1f}  spread {100 * spread[key][1]:5.1f} %   '
                     f'{nbytes[key] / 1e6:7.1f} MB ({what[key]})  {nbytes[key] / mk / 1e6:5.2f} TB/s')
    lines.append('')
    for key in ('(P)', '(L)', '(M)'):
        mk, mw = med[key]
        d, bar = mk - med['(b)'][0], spread['(b)'][0] * med['(b)'][0]
        lines.append(f'{key} kernel: {mk / med["(a)"][0]:.3f} x (a), {mk / med["(b)"][0]:.3f} x (b) ({d:+.1f} us against (b)\'s own spread of {bar:.1f} us: '
                     + ('not slower' if d <= bar else 'SLOWER') + f'), {mk / med["(c)"][0]:.3f} x (c);  whole call: {mw / med["(a)"][1]:.3f} x (a), '
                     f'{mw / med["(b)"][1]:.3f} x (b), {mw / med["(c)"][1]:.3f} x (c)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--yuv10', action='store_true', help='time a batch of decoded 10-bit 4:2:0 clips against the 8-bit and RGB routes (-> profiles/clip_yuv10_bench.txt)')
    ap.add_argument('--yuv', action='store_true', help='time a batch of decoded 4:2:0 clips against the RGB route (-> profiles/clip_yuv_bench.txt)')
    ap.add_argument('--parent-lib', default=None, help='--yuv: a libvtx_ragged.so built at the parent commit, timed beside this one')
    ap.add_argument('--ragged', action='store_true', help='time one call on a list of clips of differing size against one call per clip (-> profiles/clip_ragged_bench.txt)')
    ap.add_argument('--stem', action='store_true', help='time the uint8 stem gather and hog_targets against the float routes (-> profiles/stem_u8_bench.txt)')
    ap.add_argument('--mix', action='store_true', help='time Mixup / CutMix on uint8 clips against the float route (-> profiles/clip_mix_bench.txt)')
    ap.add_argument('--views', action='store_true', help='time clip_views_u8 against the composition it replaces (-> profiles/clip_views_bench.txt)')
    ap.add_argument('--decoded', type=int, default=32, help='--views, --ragged, --yuv, --yuv10: decoded frames per clip')
    ap.add_argument('--short-side', type=int, default=256, help='--views: the Resize of the test pipeline')
    ap.add_argument('--randaug', action='store_true', help='time the RandAugment kernels instead (-> profiles/clip_randaug_bench.txt)')
    ap.add_argument('--clips', type=int, default=None, help='default 96; 32 with --views, --stem, --ragged, --yuv and --yuv10')
    ap.add_argument('--frames', type=int, default=None, help='default 8; 16 with --stem')
    ap.add_argument('--src', type=int, nargs=2, default=(256, 340))
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--sets', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--step-ms', type=float, default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.clips is None:
        a.clips = 32 if a.views or a.stem or a.ragged or a.yuv or a.yuv10 else 96
    if a.frames is None:
        a.frames = 16 if a.stem else 8
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'clip_yuv10_bench.txt' if a.yuv10 else 'clip_yuv_bench.txt' if a.yuv else 'clip_ragged_bench.txt' if a.ragged else 'stem_u8_bench.txt' if a.stem else 'clip_mix_bench.txt' if a.mix else 'clip_views_bench.txt' if a.views else
                             'clip_randaug_bench.txt' if a.randaug else 'clip_aug_bench.txt')
    assert torch.cuda.is_available(), 'aug_bench needs a GPU'
    if a.yuv10:
        return yuv10_main(a)
    if a.yuv:
        return yuv_main(a)
    if a.ragged:
        return ragged_main(a)
    if a.stem:
        return stem_main(a)
    if a.mix:
        return mix_main(a)
    if a.views:
        return views_main(a)
    if a.randaug:
        return randaug_main(a)
    dev = 'cuda:0'
    B, T, (Hs, Ws), S = a.clips, a.frames, a.src, a.size
    g = torch.Generator().manual_seed(0)
    srcs = [torch.randint(0, 256, (B, T, Hs, Ws, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(a.sets)]
    draws = aug.sample_params(B, (Hs, Ws), generator=g)
    xt = aug._tables([(Ws, d.left, d.width, S, d.flip, 0, S) for d in draws], 'bicubic', False)
    yt = aug._tables([(Hs, d.top, d.height, S, False, 0, S) for d in draws], 'bicubic', False)
    up = lambda t: tuple(torch.from_numpy(x).to(dev) for x in t)
    xt, yt = up(xt), up(yt)
    jo = torch.tensor([[3] + list(d.ops) for d in draws], dtype=torch.int32, device=dev)
    jf = torch.tensor([list(d.factors) + [1.0 - f for f in d.factors] for d in draws], dtype=torch.float64).float().to(dev)
    outs = [ops.clip_resample_u8(s, (S, S), xt, yt) for s in srcs]
    whole = aug.ClipAugment(img_size=S)

    res = timed(lambda i: ops.clip_resample_u8(srcs[i % a.sets], (S, S), xt, yt), a.iters, a.rounds, a.warmup)
    jit = timed(lambda i: ops.clip_jitter_u8_(outs[i % a.sets], jo, jf), a.iters, a.rounds, a.warmup)
    # the public call: draws and tables on the host, one upload, both kernels; host clock around a synchronised call
    import time
    torch.cuda.synchronize()
    host = []
    for i in range(a.rounds):
        t0 = time.perf_counter()
        whole(srcs[i % a.sets], generator=g)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)

    frames = B * T
    crop = sum(d.height * d.width for d in draws) / B * 3 * frames            # bytes of the crop boxes actually read
    res_bytes = frames * (Hs * Ws * 3 + S * S * 3)
    jit_bytes = frames * S * S * 3 * 3
    lines = [f'clip augmentation, {B} clips x {T} frames, {Hs}x{Ws} -> {S}x{S}, bicubic, antialias off; {torch.cuda.get_device_name(0)}',
             f'{a.rounds} rounds of {a.iters} launches after {a.warmup} warm-up launches, HIP events; {a.sets} source sets of '
             f'{srcs[0].numel() / 2**20:.0f} MiB in rotation; spread = (max - min) / median over the rounds',
             '']

    def row(name, us, nbytes, note=''):
        med, lo, hi = statistics.median(us), min(us), max(us)
        lines.append(f'{name:<22} median {med:8.1f} us  min {lo:8.1f}  max {hi:8.1f}  spread {100 * (hi - lo) / med:4.1f} %  {nbytes / 1e6:7.1f} MB  {nbytes / med / 1e6:6.2f} TB/s '
                     f'= {nbytes / (med * 1e-6) / HBM:5.3f} of 8 TB/s{note}')
        return med
    m1 = row('vtx_clip_resample_u8', res, res_bytes, f'  (whole source frames; the crop boxes alone: {(crop + frames * S * S * 3) / 1e6:.1f} MB)')
    m2 = row('vtx_clip_jitter_u8', jit, jit_bytes, '  (three ops per clip, contrast among them: sum pass + blend pass)')
    lines.append(f'pair                   median {m1 + m2:8.1f} us')
    lines.append(f'ClipAugment.__call__   median {statistics.median(host):8.2f} ms  min {min(host):8.2f} ms  host clock, synchronised: '
                 f'{B} draws, {2 * B} tables, one upload, both kernels')
    if a.step_ms:
        lines.append(f'training step (bench.py --gpus 1 --batch {B}, same run): {a.step_ms:.1f} ms -> the kernel pair is '
                     f'{(m1 + m2) / (a.step_ms * 1e3) * 100:.2f} % of the step, the whole call {statistics.median(host) / a.step_ms * 100:.2f} %')
    lines.append("(the reference's CPU pipeline -- per frame bicubic RandomResizedCrop + ColorJitter in DataLoader workers -- was not measured)")
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
