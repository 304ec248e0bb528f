"""Do two builds of libvtx.so launch the same GEMM kernels and compute the same bits?

    rocprofv3 --kernel-trace -f csv -d DIR_A -- python tools/gemm_launches.py run OUT_A.json          (VTX_LIB names build A)
    rocprofv3 --kernel-trace -f csv -d DIR_B -- python tools/gemm_launches.py run OUT_B.json          (build B)
    python tools/gemm_launches.py compare DIR_A OUT_A.json DIR_B OUT_B.json

`run` drives vtx_gemm_nt / vtx_gemm_tn over NT_SHAPES / NT_NODMA_SHAPES of tests/exact.py, TN_SHAPES of
tests/test_gpu_exact_arith.py and the layer shapes of tools/gemm_shapes.py (ViT-B at 8 clips of 8 frames: M = 12544, and the
headline M = 150528 for the weight gradients), under auto and every forced variant, gemm_nodma, tn_safe, pp_cont = 0, pp_epi in
{1, 6}, tn_cus = 240, with and without bias-gradient sums, residual, row scale and activation, and writes a sha256 per output
buffer.  vtx.ops hands vtx_gemm_tn exactly vtx_gemm_tn_workspace() bytes, so every weight-gradient call also shows that the plan
it chose fits the advertised workspace.  `compare` checks that the two traces hold the same sequence of (kernel, grid,
workgroup, LDS bytes) and the two runs the same hashes; exit status 1 otherwise.
"""
import csv
import glob
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'videotransformer-pytorch_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

LAYER_M, HEAD_M = 12544, 150528
LAYER_NT = ((2304, 768), (768, 768), (3072, 768), (768, 3072))          # (N, K): qkv, proj, fc1, fc2
NT_FAMILIES = ('auto', 'pp256', 'dma2', 'ring128x3', 'ring128x4k32', 'ring256x3', 'ring256x3k32', 'ring256x4k32')
TN_VARIANTS = ('auto', 'pp256', 'ring', 'dma2', 'w4')


def run(out_path):
    import torch
    import vtx
    from vtx import ops
    import exact as X
    from test_gpu_exact_arith import TN_SHAPES
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(7)
    hashes = []

    def rnd(*shape, dtype=torch.bfloat16):
        return (torch.randint(-3, 4, shape, generator=g).float()).to(dtype).to(dev)

    def note(tag, *tensors):
        torch.cuda.synchronize()
        for t in tensors:
            hashes.append((tag, hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()))

    def with_opts(opts, fn):
        for k, v in opts.items():
            vtx.set_option(k, v)
        try:
            fn()
        finally:
            for k in opts:
                vtx.set_option(k, dict(gemm_nt='auto', gemm_tn='auto', gemm_nodma='0', tn_safe='0', tn_cus='256', pp_cont='1', pp_epi='0')[k])

    def nt_cases(M, N, K, dtype=torch.bfloat16, rich=True):
        A, W, b = rnd(M, K, dtype=dtype), rnd(N, K, dtype=dtype), rnd(N, dtype=torch.float32)
        epis = [('plain', {}), ('bias', dict(bias=b))]
        if rich:
            R, sc = rnd(M, N, dtype=dtype), rnd(M, dtype=torch.float32)
            epis += [('bias+res', dict(bias=b, R=R)), ('bias+scale', dict(bias=b, row_scale=sc, rs=(M, 0, 1, 0))),
                     ('bias+res+scale', dict(bias=b, R=R, row_scale=sc, rs=(M, 0, 1, 0))), ('bias+gelu', dict(bias=b, act=1)),
                     ('bias+gelu+grad', dict(bias=b, act=2, C2=torch.zeros(M, N, dtype=dtype, device=dev))),
                     ('mul', dict(dgelu_in=rnd(M, N, dtype=dtype), dgelu_kind=1)), ('dgelu', dict(dgelu_in=rnd(M, N, dtype=dtype), dgelu_kind=0))]
        for name, kw in epis:
            C = torch.zeros(M, N, dtype=dtype, device=dev)
            ops.gemm_nt(A, W, C, M, N, K, **kw)
            note(f'nt {M}x{N}x{K} {name}', C, *([kw['C2']] if 'C2' in kw else []))

    def tn_cases(M, N1, N2, dtype=torch.bfloat16):
        A, B = rnd(M, N1, dtype=dtype), rnd(M, N2, dtype=dtype)
        note(f'tn {M}x{N1}x{N2}', ops.gemm_tn(A, B, M, N1, N2))
        C, s = ops.gemm_tn(A, B, M, N1, N2, want_colsum=True)
        note(f'tn {M}x{N1}x{N2} colsum', C, s)

    nt_shapes = [(m, n, k) for m, n, k, _ in X.NT_SHAPES + X.NT_NODMA_SHAPES] + [(LAYER_M, n, k) for n, k in LAYER_NT]
    nt_opts = [dict(gemm_nt=f) for f in NT_FAMILIES] + [dict(gemm_nodma='1'), dict(pp_cont='0'), dict(pp_epi='1'), dict(pp_epi='6'),
                                                       dict(gemm_nt='pp256', pp_cont='0'), dict(gemm_nt='pp256', pp_epi='6')]
    for opts in nt_opts:
        for m, n, k in nt_shapes:
            with_opts(opts, lambda: nt_cases(m, n, k, rich=m != LAYER_M or opts in ({'gemm_nt': 'auto'}, {'pp_cont': '0'}, {'pp_epi': '1'})))
    nt_cases(*nt_shapes[0], dtype=torch.float32, rich=False)
    tn_shapes = list(TN_SHAPES) + [(LAYER_M, k, n) for n, k in LAYER_NT] + [(HEAD_M, 768, 768), (HEAD_M, 768, 2304)]
    tn_opts = [dict(gemm_tn=v) for v in TN_VARIANTS] + [dict(gemm_nodma='1'), dict(tn_safe='1'), dict(tn_cus='240'),
                                                       dict(gemm_tn='w4', tn_cus='240'), dict(gemm_tn='ring', tn_cus='240')]
    for opts in tn_opts:
        for m, n1, n2 in tn_shapes:
            if m == HEAD_M and opts.get('gemm_tn') not in (None, 'auto', 'w4', 'ring'):
                continue
            with_opts(opts, lambda: tn_cases(m, n1, n2))
    tn_cases(*TN_SHAPES[0], dtype=torch.float32)
    with open(out_path, 'w') as f:
        json.dump(hashes, f)
    print(f'{len(hashes)} output buffers hashed -> {out_path}')


def trace(d):
    files = sorted(glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True))
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    keep = ('Kernel_Name', 'Grid_Size_X', 'Grid_Size_Y', 'Grid_Size_Z', 'Workgroup_Size_X', 'Workgroup_Size_Y', 'Workgroup_Size_Z', 'LDS_Block_Size')
    return [tuple(r[k] for k in keep) for r in rows if 'gemm' in r['Kernel_Name'] or 'reduce_partials' in r['Kernel_Name']]


def compare(dir_a, out_a, dir_b, out_b):
    ta, tb = trace(dir_a), trace(dir_b)
    ha, hb = json.load(open(out_a)), json.load(open(out_b))
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(ta, tb)) if a != b]
    names = sorted({t[0].split('(')[0] for t in ta})
    print(f'launches: {len(ta)} / {len(tb)}, {len(bad)} differ; {len(names)} distinct kernels')
    for n in names:
        print('  ', n[:150])
    for x in bad[:10]:
        print('  DIFF', x)
    hbad = [(a, b) for a, b in zip(ha, hb) if a != b]
    print(f'output buffers: {len(ha)} / {len(hb)}, {len(hbad)} differ')
    for x in hbad[:10]:
        print('  DIFF', x)
    return 1 if (bad or hbad or len(ta) != len(tb) or len(ha) != len(hb) or not ta or not ha) else 0


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        run(sys.argv[2])
    else:
        sys.exit(compare(*sys.argv[2:6]))
