"""Three measurements for the dropout path (csrc/dropout.hip), written to profiles/dropout_bench.txt:

    python tools/dropout_bench.py [--parent DIR] [--out profiles/dropout_bench.txt] [--skip kernel,bench,step]

  kernel  vtx_dropout_rows in place on the two shapes it meets at the benchmark batch (150 624 x 3072: the FFN's hidden
          activation, 150 624 x 768: a sub-block's output; bf16) against vtx_row_scale_copy in place on the same shapes, which
          moves the same bytes without the generator.  Both in one process, alternating, HIP events around `iters` launches,
          median of `rounds` rounds after a warm-up round; GB/s counts one read and one write of the tensor.
  bench   `python bench.py` (the p == 0 path) in DIR, a checkout of the parent commit with its libraries built, and in this
          tree: three runs each, alternating, one process per run.  The difference of the means has to lie within the spread of
          the parent's own three runs.  Without --parent this part is skipped.
  step    forward + backward of TimeSformer-B, 96 clips x 8 frames, bf16, with dropout_p = 0.1 on the embeddings, the FFNs and
          proj_drop of both attention operators against p = 0 (two models with the same weights, alternating).  The temporal
          operator runs its two projection GEMMs unmerged with proj_drop on, so this costs more than the masks alone.

VTX_DROPOUT_LIB=<path> loads another build of libvtx_dropout.so for the kernel part (a scratch build with fewer Philox rounds
shows what the generator costs; the product always runs ten).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'videotransformer-pytorch_amd'))


def _timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_rate(say, iters, rounds):
    import torch
    from vtx import ops
    say('kernel rate, bf16, in place: median ms per launch over %d rounds of %d launches (min .. max), GB/s = 2 x tensor bytes / median' % (rounds, iters))
    for rows, D in ((150624, 3072), (150624, 768)):
        x = torch.randn(rows, D, device='cuda:0').bfloat16()
        nbytes = 2.0 * rows * D * 2
        sides = {'vtx_dropout_rows p=0.1': lambda: ops.dropout_rows(x, x, rows, D, 0.1, 1234567, 0),
                 'vtx_row_scale_copy    ': lambda: ops.row_scale_copy(x, x, rows, D)}
        times = {k: [] for k in sides}
        for r in range(rounds + 1):                        # round 0 warms up
            for k, fn in sides.items():
                t = _timed(fn, iters)
                if r:
                    times[k].append(t)
        for k, ts in times.items():
            med = statistics.median(ts)
            say(f'  {rows} x {D}  {k}  {med:.4f} ms ({min(ts):.4f} .. {max(ts):.4f})  {nbytes / med / 1e6:.0f} GB/s')
        del x


def bench_ab(say, parent, runs):
    say(f'bench.py, p == 0 path: {runs} runs each, alternating, clips/s per GPU')
    vals = {'parent': [], 'this': []}
    for r in range(runs):
        for name, tree in (('parent', parent), ('this', ROOT)):
            out = subprocess.run([sys.executable, 'bench.py', '--gpus', '1'], cwd=tree, capture_output=True, text=True, timeout=600)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
            if out.returncode != 0 or not line:
                say(f'  {name} run {r}: failed (exit {out.returncode}): {out.stderr[-300:]}')
                return
            v = json.loads(line[-1])
            cps = v.get('clips_per_sec_per_gpu', v.get('value'))
            vals[name].append(float(cps))
            say(f'  {name} run {r}: {cps}')
    mp, mt = statistics.mean(vals['parent']), statistics.mean(vals['this'])
    spread = max(vals['parent']) - min(vals['parent'])
    say(f'  parent mean {mp:.3f} (spread {spread:.3f}), this commit mean {mt:.3f}, difference {mt - mp:+.3f}: '
        f'{"within" if abs(mt - mp) <= spread else "OUTSIDE"} the spread of the parent\'s own runs')


def step_cost(say, clips, iters, rounds):
    import torch
    import vtx
    import transformer as T
    import video_transformer as V
    vtx.set_precision('bf16')
    dev = torch.device('cuda:0')

    def build(p):
        torch.manual_seed(0)
        m = V.TimeSformer(num_frames=8, dropout_p=p)
        with torch.no_grad():
            for blk in m.transformer_layers.layers:
                blk.attentions[0].temporal_fc.weight.normal_(0, 0.02)
        for mod in m.modules():                            # the constructor hands its dropout_p to the embeddings only
            if isinstance(mod, T.FFNWithPreNorm):
                mod.dropout_p = p
            elif hasattr(mod, 'proj_drop') and hasattr(mod, 'layer_drop'):
                mod.proj_drop.p = p
        return m.to(dev).train()
    models = {'p = 0  ': build(0.0), 'p = 0.1': build(0.1)}
    x = torch.randn(clips, 8, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(dev)

    def run(m):
        def f():
            for prm in m.parameters():
                prm.grad = None
            m(x).sum().backward()
        return f
    times = {k: [] for k in models}
    for r in range(rounds + 1):
        for k, m in models.items():
            t = _timed(run(m), iters)
            if r:
                times[k].append(t)
    say(f'TimeSformer-B forward + backward, {clips} clips x 8 frames, bf16: median ms per step over {rounds} rounds of {iters} (min .. max)')
    for k, ts in times.items():
        say(f'  {k}  {statistics.median(ts):.2f} ms ({min(ts):.2f} .. {max(ts):.2f})')
    a, b = statistics.median(times['p = 0  ']), statistics.median(times['p = 0.1'])
    say(f'  dropout on embeddings, FFN and proj_drop: {b - a:+.2f} ms ({(b / a - 1) * 100:+.1f} %)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit (for the bench.py comparison)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dropout_bench.txt'))
    ap.add_argument('--skip', default='')
    ap.add_argument('--clips', type=int, default=96)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    skip = set(a.skip.split(','))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, 'w')

    def say(s):
        print(s, flush=True)
        f.write(s + '\n')
        f.flush()
    say('tools/dropout_bench.py: ' + ' '.join(sys.argv[1:]))
    if 'bench' not in skip and a.parent:                   # first: this process has not opened the GPU yet
        bench_ab(say, a.parent, 3)
    if 'kernel' not in skip:
        kernel_rate(say, a.iters, a.rounds)
    if 'step' not in skip:
        step_cost(say, a.clips, 3, a.rounds)
    f.close()


if __name__ == '__main__':
    main()
