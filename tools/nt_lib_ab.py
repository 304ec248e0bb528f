"""A/B of the persistent NT GEMM between two builds (GPU box only).  A process loads one library, so the builds alternate as
child processes, one at a time -- the two-process form of tools/nt_ab.py, for changes that are not behind a run-time option.

    python tools/nt_lib_ab.py                     the rows of ROWS for the library VTX_LIB names (default: this tree's)
    python tools/nt_lib_ab.py --ab PARENT_LIB     parent, this, this, parent, parent, this, this, parent; per row all samples of
                                                  an arm (mean, min, max) and whether the difference of the means exceeds the
                                                  min-max spread of either arm

Rows: the six NT shapes of a 96-clip TimeSformer-B step with their epilogues (gemm_nt=pp256, random operands).  A sample is 20
back-to-back launches between two HIP events; a child takes one warm-up sample and four samples per row.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [(150528, 2304, 768, 'plain'), (150528, 768, 2304, 'plain'), (150528, 768, 768, 'residual'),
        (150624, 3072, 768, 'gelu2'), (150624, 3072, 768, 'mul'), (150624, 768, 3072, 'residual')]
L = 20


def measure():
    for p in (ROOT, os.path.join(ROOT, 'videotransformer-pytorch_amd')):
        sys.path.insert(0, p)
    import torch
    import vtx
    from vtx import ops
    dev = 'cuda:0'
    vtx.set_option('gemm_nt', 'pp256')
    res = {}
    for M, N, K, kind in ROWS:
        A = torch.randn(M, K, device=dev).bfloat16()
        W = torch.randn(N, K, device=dev).bfloat16()
        C = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        kw = dict(bias=torch.randn(N, device=dev))
        if kind == 'residual':
            kw.update(R=torch.randn(M, N, device=dev).bfloat16(), row_scale=torch.ones(M, device=dev))
        elif kind == 'mul':
            kw = dict(dgelu_in=torch.randn(M, N, device=dev).bfloat16(), dgelu_kind=1)
        elif kind == 'gelu2':
            kw.update(act=2, C2=torch.empty(M, N, device=dev, dtype=torch.bfloat16))
        t = []
        for r in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(L):
                ops.gemm_nt(A, W, C, M, N, K, **kw)
            e1.record()
            torch.cuda.synchronize()
            if r >= 1:
                t.append(e0.elapsed_time(e1) / L * 1e3)
        res[f'{M}x{N}x{K} {kind}'] = t
        print(f'{M}x{N}x{K} {kind:8s}: median {sorted(t)[len(t) // 2]:8.1f} us  min {min(t):8.1f}  max {max(t):8.1f}', flush=True)
        del A, W, C, kw
    vtx.set_option('gemm_nt', 'auto')
    print('NT_AB ' + json.dumps(res), flush=True)


def ab(parent):
    runs = {'P': [], 'N': []}
    for c in 'PNNPPNNP':                            # symmetric in time: a drift of the box cancels in the two means
        env = dict(os.environ)
        env.pop('VTX_LIB', None)
        if c == 'P':
            env['VTX_LIB'] = os.path.abspath(parent)
        out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        if out.returncode != 0:                     # stop here: nothing more is started on the GPU after a failed run
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-2000:])
            return out.returncode
        runs[c].append(json.loads(next(l for l in out.stdout.splitlines() if l.startswith('NT_AB '))[6:]))
    print(f'{"row":34s} {"parent mean":>11s} {"min":>8s} {"max":>8s} | {"new mean":>9s} {"min":>8s} {"max":>8s} | new / parent')
    for k in runs['P'][0]:
        p = [x for r in runs['P'] for x in r[k]]
        n = [x for r in runs['N'] for x in r[k]]
        pm, nm = sum(p) / len(p), sum(n) / len(n)
        spread = max(max(p) - min(p), max(n) - min(n))
        verdict = 'within the spread' if abs(pm - nm) <= spread else ('new faster' if nm < pm else 'NEW SLOWER')
        print(f'{k:34s} {pm:11.1f} {min(p):8.1f} {max(p):8.1f} | {nm:9.1f} {min(n):8.1f} {max(n):8.1f} | {nm / pm:.4f}  {verdict}')
    return 0


if __name__ == '__main__':
    sys.exit(ab(sys.argv[2]) if sys.argv[1:2] == ['--ab'] else measure())
