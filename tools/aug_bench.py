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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--randaug', action='store_true', help='time the RandAugment kernels instead (-> profiles/clip_randaug_bench.txt)')
    ap.add_argument('--clips', type=int, default=96)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--src', type=int, nargs=2, default=(256, 340))
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--sets', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--step-ms', type=float, default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'clip_randaug_bench.txt' if a.randaug else 'clip_aug_bench.txt')
    assert torch.cuda.is_available(), 'aug_bench needs a GPU'
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
             f'{srcs[0].numel() / 2**20:.0f} MiB in rotation',
             '']

    def row(name, us, nbytes, note=''):
        med, lo = statistics.median(us), min(us)
        lines.append(f'{name:<22} median {med:8.1f} us  min {lo:8.1f} us  {nbytes / 1e6:7.1f} MB  {nbytes / med / 1e6:6.2f} TB/s '
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
