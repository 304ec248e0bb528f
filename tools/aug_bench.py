"""Clip augmentation on the device (csrc/aug.hip): time of the resampler and the colour jitter for one training batch --
96 clips of 8 frames, 256x340 -> 224x224, bicubic, every clip with its own crop, flip and three colour ops.  GPU box only.

    python tools/aug_bench.py [--clips 96] [--frames 8] [--step-ms MS] [--out profiles/clip_aug_bench.txt]

HIP events around `--iters` back-to-back launches per round, after a warm-up; `--rounds` rounds, median and minimum.  The
source clips rotate through `--sets` buffers (together larger than the 256 MiB Infinity Cache) so that reads come from HBM
as they do behind a data loader.  Bytes = what the algorithm has to move (source read + result written; the jitter: the
clip read once for the grey sums and read + written by the blend), held against the 8 TB/s DESIGN.md uses for the other
byte-bound kernels.  --step-ms: the `ms_per_step` of `bench.py --gpus 1` at the same number of clips, for the share of
the training step (not measured here).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=96)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--src', type=int, nargs=2, default=(256, 340))
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--sets', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--step-ms', type=float, default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_aug_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'aug_bench needs a GPU'
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
