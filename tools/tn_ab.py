"""A/B of the weight-gradient GEMM routes between two builds (GPU box only): launch + slab reduction per call, as vtx_gemm_tn
runs them.  A process loads one library, so the builds alternate as child processes, one at a time.

    python tools/tn_ab.py                      the rows of ROWS for the library VTX_LIB names (default: this tree's), one line each
    python tools/tn_ab.py --ab PARENT_LIB      parent, this tree, this tree, parent; per row the medians, the parent's A/A
                                               spread (its two runs are not adjacent) and whether this tree is within it
    ... --only ring,w4                         either form with the rows of these names alone (to repeat one kernel family)

Rows: pp256, ring and w4 at M = 150528 on the four training shapes with and without the column sums; auto at M = 12544;
dma2 at M = 768 on 768x768 and 768x400; nodma and fp32 at M = 5000 on 216x768.  A sample is `reps` launches between two
events (200 for the launches of a few microseconds, so that a sample is no shorter than a millisecond), a row's figure the
median of 9 samples after 3 warm-up launches.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = ((768, 3072), (3072, 768), (2304, 768), (768, 768))
# (name, options, dtype, M, N1, N2, column sums, launches per sample)
ROWS = ([(v, dict(gemm_tn=v), 'bfloat16', 150528, n1, n2, cs, 10) for v in ('pp256', 'ring', 'w4') for n1, n2 in TRAIN for cs in (1, 0)] +
        [('auto', dict(gemm_tn='auto'), 'bfloat16', 12544, n1, n2, 1, 50) for n1, n2 in TRAIN] +
        [('dma2', dict(gemm_tn='dma2'), 'bfloat16', 768, 768, n2, cs, 200) for n2 in (768, 400) for cs in (1, 0)] +
        [('nodma', dict(gemm_nodma='1'), 'bfloat16', 5000, 216, 768, 1, 200), ('f32', {}, 'float32', 5000, 216, 768, 1, 50)])
DEFAULTS = dict(gemm_tn='auto', gemm_nodma='0')


def key(r):
    return f'{r[0]:6s} {r[3]}x{r[4]}x{r[5]} colsum={r[6]}'


def measure(only):
    for p in (ROOT, os.path.join(ROOT, 'videotransformer-pytorch_amd')):
        sys.path.insert(0, p)
    import torch
    import vtx
    from vtx import ops
    res, held = {}, {}
    for r in [r for r in ROWS if not only or r[0] in only]:
        name, opts, dtype, M, N1, N2, cs, reps = r
        for k, v in dict(DEFAULTS, **opts).items():
            vtx.set_option(k, v)
        if (dtype, M, N1, N2) not in held:
            held.clear()
            g = torch.Generator(device='cuda:0').manual_seed(M + N1 + N2)
            held[(dtype, M, N1, N2)] = tuple(torch.randn(M, n, device='cuda:0', generator=g).to(getattr(torch, dtype)) for n in (N1, N2))
        x, y = held[(dtype, M, N1, N2)]
        C, s = torch.empty(N1, N2, device='cuda:0'), torch.empty(N1, device='cuda:0')
        call = (lambda: ops.gemm_tn(x, y, M, N1, N2, out=C, colsum_out=s)) if cs else (lambda: ops.gemm_tn(x, y, M, N1, N2, out=C))
        for _ in range(3):
            call()
        t = []
        for _ in range(9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3 / reps)
        res[key(r)] = sorted(t)[4]
        print(f'{key(r)}: median {res[key(r)]:9.2f} us  min {min(t):9.2f} us', flush=True)
    for k, v in DEFAULTS.items():
        vtx.set_option(k, v)
    print('TN_AB ' + json.dumps(res), flush=True)


def ab(parent, only):
    runs = []
    for lib in (parent, None, None, parent):         # symmetric in time: a drift of the box cancels in the two means
        env = dict(os.environ)
        env.pop('VTX_LIB', None)
        if lib:
            env['VTX_LIB'] = os.path.abspath(lib)
        out = subprocess.run([sys.executable, os.path.abspath(__file__)] + (['--only', ','.join(only)] if only else []), env=env, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:                     # stop here: nothing more is started on the GPU after a failed run
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
            return out.returncode
        runs.append(json.loads(next(l for l in out.stdout.splitlines() if l.startswith('TN_AB '))[6:]))
    p1, n1, n2, p2 = runs
    print(f'{"row":34s} {"parent":>9s} {"parent":>9s} {"A/A":>7s} {"new":>9s} {"new":>9s}  new / parent (medians of the two)')
    miss = 0
    for k in p1:
        p, n = (p1[k] + p2[k]) / 2, (n1[k] + n2[k]) / 2
        aa = abs(p1[k] - p2[k]) / p
        ok = n <= p * (1 + aa)
        miss += not ok
        print(f'{k:34s} {p1[k]:9.2f} {p2[k]:9.2f} {aa * 100:6.2f}% {n1[k]:9.2f} {n2[k]:9.2f}  {n / p:6.4f}  {"within the A/A spread" if ok else "MISS"}')
    print(f'{len(p1)} rows, {miss} outside the parent\'s A/A spread')
    return 0


if __name__ == '__main__':
    only = sys.argv[sys.argv.index('--only') + 1].split(',') if '--only' in sys.argv else []
    sys.exit(ab(sys.argv[2], only) if sys.argv[1:2] == ['--ab'] else measure(only))
