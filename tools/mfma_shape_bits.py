"""Do v_mfma_f32_32x32x16_bf16 and v_mfma_f32_16x16x32_bf16 give the same bits?  (GPU box only; one launch.)

    python tools/mfma_shape_bits.py [steps=64] [seed=0]

One wave multiplies random bf16 A[32][K] by B[32][K]^T, K = 32 * steps, into an fp32 accumulator in K order: once as two
32x32x16 instructions per 32-deep step, once as one 16x16x32 instruction per step (tools/micro/mfma_shape_bits.hip, built
next to its source when stale).  Prints how many of the 1024 outputs differ in bits, the largest difference in units of the
float64 result's fp32 ulp, and each shape's own error against float64.  Bit-equal shapes would mean that a kernel can change
shape without any result moving; a difference means the fp32 adds inside a 32-deep step are grouped differently.
"""
import ctypes
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'micro', 'mfma_shape_bits.hip')
LIB = os.path.join(HERE, 'micro', 'mfma_shape_bits.so')


def build():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
        subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-o', LIB, SRC], check=True)
    return LIB


def run(steps=64, seed=0):
    import torch
    lib = ctypes.CDLL(build())
    lib.mfma_shape_bits.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    g = torch.Generator().manual_seed(seed)
    K = 32 * steps
    A = torch.randn(32, K, generator=g).bfloat16()
    B = torch.randn(32, K, generator=g).bfloat16()
    ref = A.double() @ B.double().t()
    dA, dB = A.cuda(), B.cuda()
    o32 = torch.full((32, 32), float('nan'), device='cuda')
    o16 = torch.full((32, 32), float('nan'), device='cuda')
    rc = lib.mfma_shape_bits(dA.data_ptr(), dB.data_ptr(), steps, o32.data_ptr(), o16.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    o32, o16 = o32.cpu(), o16.cpu()
    ndiff = int((o32.view(torch.int32) != o16.view(torch.int32)).sum())
    ulp = torch.maximum(ref.abs(), torch.tensor(2.0 ** -126, dtype=torch.float64)).log2().floor().exp2() * 2.0 ** -23
    return dict(steps=steps, K=K, differ=ndiff, of=1024,
                max_diff_ulp=float(((o32.double() - o16.double()).abs() / ulp).max()),
                err32_ulp=float(((o32.double() - ref).abs() / ulp).max()),
                err16_ulp=float(((o16.double() - ref).abs() / ulp).max()),
                bound_ok=bool(((o32.double() - ref).abs().max() < 1e-2) and ((o16.double() - ref).abs().max() < 1e-2)))


if __name__ == '__main__':
    r = run(*(int(x) for x in sys.argv[1:3]))
    print(f"K = {r['K']} ({r['steps']} steps of 32): {r['differ']} of {r['of']} outputs differ in bits; largest difference "
          f"{r['max_diff_ulp']:.2f} ulp; against float64: 32x32x16 {r['err32_ulp']:.2f} ulp, 16x16x32 {r['err16_ulp']:.2f} ulp"
          f"{'' if r['bound_ok'] else '  -- A RESULT IS WRONG (operand or result map)'}")
    print('the shapes are bit-identical' if r['differ'] == 0 else 'the shapes are NOT bit-identical')
