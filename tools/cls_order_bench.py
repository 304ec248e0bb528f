"""Forward + backward of ONE BasicTransformerBlock in each divided-attention operator order, bf16:

    python tools/cls_order_bench.py [--orders default,new] [--clips 96] [--frames 8] [--patches 196] [--iters 20] [--rounds 5]

time-then-space (the models' order) against space-then-time (temporal attention over the cls token, spatial attention
without it).  Per order: median of `rounds` rounds of `iters` timed iterations (HIP events around the whole
round), and the spread of the rounds.  `--orders default` times the models' order alone -- one order per process, and the
form that also runs on a commit without the space-then-time order (copy this file there).  The tools next to this one time
single kernels (kernel_bench.py, attn_bench.py) or whole training steps (step_times.py); none times a block.  Run under `rocprofv3 --kernel-trace --stats -- python tools/cls_order_bench.py --iters 3
--rounds 1` for the kernel listing."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'videotransformer-pytorch_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--orders', default='default,new')
    ap.add_argument('--clips', type=int, default=96)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--patches', type=int, default=196)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    import vtx
    import transformer as T_
    vtx.set_precision('bf16')
    D, H = 768, 12
    x = torch.randn(a.clips, 1 + a.patches * a.frames, D, device='cuda:0').bfloat16().requires_grad_(True)
    g = torch.randn_like(x)
    known = {'default': ['time_attn', 'space_attn', 'ffn'], 'new': ['space_attn', 'time_attn', 'ffn']}
    for order in [known[k] for k in a.orders.split(',')]:
        torch.manual_seed(0)
        blk = T_.BasicTransformerBlock(D, H, a.frames, 4 * D, order).to('cuda:0').train()
        for p in blk.parameters():
            if p.abs().max() == 0:
                torch.nn.init.normal_(p, std=0.02)        # temporal_fc starts at zero
        times = []
        for r in range(a.rounds + 1):                      # round 0 warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                x.grad = None
                blk(x).backward(g)
            e1.record()
            torch.cuda.synchronize()
            if r:
                times.append(e0.elapsed_time(e1) / a.iters)
        times.sort()
        print(f"{'-'.join(o.split('_')[0] for o in order):>16}: median {times[len(times) // 2]:.3f} ms  min {times[0]:.3f}  max {times[-1]:.3f}  "
              f'({a.clips} clips, {a.frames} x {a.patches} tokens, {a.rounds} rounds of {a.iters})', flush=True)


if __name__ == '__main__':
    main()
