"""Interleaved same-process A/B of the LayerNorm kernels (GPU box only): option ln_rows = 1 .. 4, forward and backward; the
float32-stream forward (vtx_layernorm_acc_fwd) and the float32-gradient backward (vtx_layernorm_bwd_g32) at the same size; and
the partial-sum reduction alone (launch_reduce_partials) at the sizes of a TimeSformer-B step.  VTX_LIB selects another build.

    python tools/ln_ab.py [clips] [D]
    python tools/ln_ab.py reduce
"""
import ctypes
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'videotransformer-pytorch_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402
import vtx  # noqa: E402
from vtx import ops  # noqa: E402

DEV = 'cuda:0'


def timeit(fn, iters=20):
    """us per call."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 96
    D = int(sys.argv[2]) if len(sys.argv) > 2 else 768
    rows = B * 1569
    x = (torch.randn(rows, D, device=DEV) * 0.5).bfloat16()
    y, dx = torch.empty_like(x), torch.empty_like(x)
    g, b_ = torch.rand(D, device=DEV) + 0.5, torch.randn(D, device=DEV) * 0.1
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    fw = lambda: ops.layernorm_fwd(x, rows, D, D, ops.IDENT, g, b_, 1e-5, y, D, mean=mean, rstd=rstd)          # noqa: E731
    bw = lambda: ops.layernorm_bwd(y, D, ops.IDENT, x, D, ops.IDENT, rows, D, mean, rstd, g, x, dx, D, dg, db)  # noqa: E731
    # the exact stream: xo = xs + d (float32), y = LayerNorm(xo); its backward with the float32 gradient stream
    xs, xo = torch.randn(rows, D, device=DEV), torch.empty(rows, D, device=DEV)
    dres32, dx32 = torch.randn(rows, D, device=DEV), torch.empty(rows, D, device=DEV)
    acc = lambda: ops.layernorm_acc_fwd(xs, x, rows, D, D, ops.IDENT, xo, D, ops.IDENT, g, b_, 1e-5, y, D, mean=mean, rstd=rstd)   # noqa: E731
    g32 = lambda: ops.layernorm_bwd(y, D, ops.IDENT, xs, D, ops.IDENT, rows, D, mean, rstd, g, None, dx, D, dg, db,               # noqa: E731
                                    dres32=dres32, dx32=dx32)
    res = {}
    for r in range(10):
        for v in ('1', '2', '3', '4'):
            vtx.set_option('ln_rows', v)
            for name, fn in (('fwd', fw), ('bwd', bw)):
                t = timeit(fn)
                if r >= 2:
                    res.setdefault((name, v), []).append(t)
        if D <= 1024:
            for name, fn in (('acc_fwd', acc), ('bwd_g32', g32)):
                t = timeit(fn)
                if r >= 2:
                    res.setdefault((name, '-'), []).append(t)
    for name, nbytes in (('acc_fwd', 12), ('bwd_g32', 16)):        # bytes per element: 4 + 2 in, 4 + 2 out; 2 + 4 + 4 in, 4 + 2 out
        if (name, '-') in res:
            t = sorted(res[(name, '-')])
            med = t[len(t) // 2]
            print(f'ln_{name} rows {rows} D {D}: median {med:7.1f} us  min {t[0]:7.1f} us  {nbytes * rows * D / med / 1e6:6.2f} TB/s')
    es = 2
    for name, nb in (('fwd', 2), ('bwd', 4)):
        for v in ('1', '2', '3', '4'):
            t = sorted(res[(name, v)])
            med = t[len(t) // 2]
            print(f'ln_{name} rows {rows} D {D} ln_rows={v}: median {med:7.1f} us  min {t[0]:7.1f} us  {nb * rows * D * es / med / 1e6:6.2f} TB/s')
    # the two forward kernels against each other and against float64
    outs = []
    for v in ('1', '2', '3', '4'):
        vtx.set_option('ln_rows', v)
        fw()
        outs.append((y.float().cpu(), mean.cpu().clone(), rstd.cpu().clone()))
    xd = x.double().cpu()
    ref = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-5) * g.double().cpu() + b_.double().cpu()
    for v, (o, m, r) in zip(('1', '2', '3', '4'), outs):
        print(f'ln_rows={v}: max |y - ref| / max|ref| = {(o.double() - ref).abs().max().item() / ref.abs().max().item():.3e}')
    print('outputs equal:', [torch.equal(outs[0][0], o[0]) for o in outs[1:]])


def reduce_routes():
    """launch_reduce_partials alone (the library's internal C++ entry, by its mangled name) on the partial layouts of one
    TimeSformer-B step: the 768 x 3072 weight gradient with its bias-gradient copies (7 slabs, 12 folded copies: the 16-byte
    kernel and its scalar tail), the LayerNorm backward's [1024][2][768] (the wide kernel), the column sum of 150 528 rows
    (256 slabs: the wide kernel) and of 12 552 rows, 8 clips (50 slabs: the 4-lane kernel).  The small ones run a few
    microseconds, about what the host needs to issue a launch: 200 launches per sample, so that a sample is no shorter than a
    millisecond and one late launch does not move it (at 20 per sample two samples of one build differed by 20 %)."""
    # the Itanium name of vtx::launch_reduce_partials (csrc/common.h); after a change of its signature read the new one from
    # `nm -D libvtx.so | grep launch_reduce_partials` and keep argtypes below in step
    fn = getattr(vtx.load(), '_ZN3vtx22launch_reduce_partialsEPKfillPfifP12ihipStream_tS2_liil')
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_long]
    w = 768 * 3072
    cases = (('weight partials 768x3072 + 12 x 768', 7, w + 12 * 768, w + 768, w, 12, 768),
             ('LayerNorm partials 1024 x [2][768]', 1024, 1536, 1536, 768, 1, 0),
             ('column sum 256 x 768', 256, 768, 768, 0, 1, 0),
             ('column sum 50 x 768', 50, 768, 768, 0, 1, 0))
    runs = []
    for name, nslabs, stride, N, split, fold, fold_stride in cases:
        part = torch.randn(nslabs * stride, device=DEV)
        out, out2 = torch.zeros(N, device=DEV), torch.zeros(768, device=DEV)
        args = (part.data_ptr(), nslabs, stride, N, out.data_ptr(), 1, 1.0, ops.stream(), out2.data_ptr() if split else None, split, 1,
                fold, fold_stride)
        call = functools.partial(fn, *args)
        assert call() == 0
        runs.append((name, call, nslabs * (N + (fold - 1) * 768 * bool(split)) * 4, (part, out, out2)))
    res = {}
    for r in range(10):
        for name, call, _, _ in runs:
            t = timeit(call, iters=200)
            if r >= 2:
                res.setdefault(name, []).append(t)
    for name, _, nbytes, _ in runs:
        t = sorted(res[name])
        med = t[len(t) // 2]
        print(f'reduce {name}: median {med:7.1f} us  min {t[0]:7.1f} us  {nbytes / med / 1e6:6.2f} TB/s')


if __name__ == '__main__':
    reduce_routes() if sys.argv[1:2] == ['reduce'] else main()
