"""Self-attention by head dim at equal FLOPs (GPU box only): D = 768 as 24 x 32, 12 x 64, 8 x 96 and 6 x 128, bf16 or fp32.

    python tools/attn_hd_bench.py [spatial] [joint] [temporal] [temporal_cls] [hd=32,64,96,128] [rounds=5] [iters=5] [dtype=bf16|fp32]

  spatial       96 clips x 8 frames, VTX_ATTN_SPACE, L = 197 (the headline workload's spatial attention)
  joint         8 clips, VTX_ATTN_CONTIG, L = 1569
  temporal      S = 96 * 196, VTX_ATTN_CONTIG, L = 8 (the packed kernels of each head dim; attn_hd=valu: the packed VALU kernels)
  temporal_cls  B = 96, P = 196, T = 8, VTX_ATTN_TIME_CLS, L = 9 (the temporal attention of the space-then-time order)

Every (head dim, attn_hd value) pair is a configuration; a round times the forward and the backward of every configuration
once (`iters` launches behind two warm-up launches, device events), and the rounds are interleaved, so that drift of the
clock hits all configurations alike.  Printed: median over the rounds, min .. max, TFLOP/s of the median (forward
4 S H L^2 hd, backward 10 S H L^2 hd: the formulas of vtx/ops.py) and its share of the dense bf16 roof bench.py uses
(2500 TFLOP/s).  head_dim 64 ignores attn_hd and is listed once.  VTX_LIB names another build of the library (the
yardstick row of a parent build: hd=64).
dtype=fp32: fp32 buffers, the configuration axis is the value of attn_f32 (every head dim answers to it, 64 included: its mfma
row is the equal-FLOP yardstick), and the share is of the fp32 matrix peak, 157.3 TFLOP/s.
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'videotransformer-pytorch_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402
import vtx  # noqa: E402
from vtx import ops  # noqa: E402
from vtx._lib import ATTN_CONTIG, ATTN_SPACE, ATTN_TIME_CLS  # noqa: E402

DEV = 'cuda:0'
ROOF = {'bf16': 2500.0, 'fp32': 157.3}
D = 768


def timed(fn, iters):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def shape_of(name):
    """(mode, S, L, B, T, P, rows of qkv, rows of out)"""
    if name == 'spatial':
        B, T, P = 96, 8, 196
        return ATTN_SPACE, B * T, P + 1, B, T, P, B * (P * T + 1), B * P * T + B * T
    if name == 'temporal_cls':
        B, T, P = 96, 8, 196
        return ATTN_TIME_CLS, B * P, T + 1, B, T, P, B * (P * T + 1), B * P * T + B * P
    S, L = (8, 1569) if name == 'joint' else (96 * 196, 8)
    return ATTN_CONTIG, S, L, 0, 0, 0, S * L, S * L


def bench(name, hds, rounds, iters, has_option, dtype='bf16'):
    mode, S, L, B, T, P, rin, rout = shape_of(name)
    bf = torch.float32 if dtype == 'fp32' else torch.bfloat16
    option, roof = ('attn_f32' if dtype == 'fp32' else 'attn_hd'), ROOF[dtype]
    r = lambda *s: (torch.randn(*s, device=DEV) * 0.5).to(bf)   # noqa: E731
    qkv, do = r(rin, 3 * D), r(rout, D)
    o = torch.empty(rout, D, device=DEV, dtype=bf)
    dqkv = torch.empty(rin, 3 * D, device=DEV, dtype=bf)
    dcls = torch.empty(max(S, 1), 3 * D, device=DEV, dtype=bf) if mode in (ATTN_SPACE, ATTN_TIME_CLS) else None
    configs = [(hd, v) for hd in hds for v in (('mfma', 'valu') if (hd != 64 or dtype == 'fp32') and has_option else ('-',))]
    times = {c: ([], []) for c in configs}
    for _ in range(rounds):
        for hd, v in configs:
            H = D // hd
            if v != '-':
                vtx.set_option(option, v)
            lse = torch.empty(S * H * L, device=DEV)
            times[(hd, v)][0].append(timed(lambda: ops.attn_fwd(qkv, o, lse, mode, S, L, H, hd, hd ** -0.5, B, T, P), iters))
            times[(hd, v)][1].append(timed(lambda: ops.attn_bwd(qkv, o, lse, do, dqkv, mode, S, L, H, hd, hd ** -0.5, B, T, P, dqkv_cls=dcls), iters))
            if v != '-':
                vtx.set_option(option, 'mfma')
    print(f'{name} {dtype}: S={S} L={L} D={D}, {rounds} interleaved rounds x {iters} launches; library {os.path.basename(vtx.load()._name)}')
    for (hd, v), both in times.items():
        H = D // hd
        for what, ts, per in (('fwd', both[0], 4.0), ('bwd', both[1], 10.0)):
            med, fl = statistics.median(ts), per * S * H * L * L * hd
            print(f'  hd={hd:3d} H={H:2d} {option}={v:4s} {what}  {med * 1e3:9.3f} ms  ({min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f})  '
                  f'{fl / med / 1e12:7.1f} TFLOP/s  {fl / med / 1e12 / roof * 100:5.2f} % of {roof:g}', flush=True)


def main():
    kv = dict(a.split('=') for a in sys.argv[1:] if '=' in a)
    names = [a for a in sys.argv[1:] if '=' not in a] or ['spatial', 'joint', 'temporal', 'temporal_cls']
    hds = [int(h) for h in kv.get('hd', '32,64,96,128').split(',')]
    dtype = kv.get('dtype', 'bf16')
    assert dtype in ROOF, 'dtype=bf16|fp32'
    try:
        vtx.set_option('attn_f32' if dtype == 'fp32' else 'attn_hd', 'mfma')
        has_option = True
    except vtx.VtxError:                                 # a build from before the option
        has_option = False
    for name in names:
        bench(name, hds, int(kv.get('rounds', 5)), int(kv.get('iters', 5)), has_option, dtype)


if __name__ == '__main__':
    main()
