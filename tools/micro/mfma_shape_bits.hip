// mfma_shape_bits.hip -- do the two bf16 MFMA shapes of gfx950 give the same bits?  (tools/mfma_shape_bits.py)
//
// One wave.  C[32][32] = A[32][K] * B[32][K]^T over K = 32 * steps, both operands K-contiguous bf16, accumulated in fp32 in
// K order, once as two v_mfma_f32_32x32x16_bf16 per 32-deep step and once as one v_mfma_f32_16x16x32_bf16 per step and
// 16 x 16 block.  Operand and result maps: gemm_nt.hip's header.
#include <hip/hip_runtime.h>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

__global__ __launch_bounds__(64) void mfma_shape_bits_kernel(const unsigned short* __restrict__ A, const unsigned short* __restrict__ B,
                                                             int steps, float* __restrict__ out32, float* __restrict__ out16) {
  const int l = threadIdx.x, K = 32 * steps;
  {
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int row = l & 31, h = l >> 5;
    for (int t = 0; t < steps; ++t)
      for (int s = 0; s < 2; ++s) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(A + (long)row * K + 32 * t + 16 * s + 8 * h);
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(B + (long)row * K + 32 * t + 16 * s + 8 * h);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
      }
    for (int r = 0; r < 16; ++r) out32[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + row] = acc[r];
  }
  {
    f32x4 acc[2][2];
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j)
        for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
    const int row = l & 15, g = l >> 4;
    for (int t = 0; t < steps; ++t) {
      bf16x8 a[2], b[2];
      for (int i = 0; i < 2; ++i) {
        a[i] = *reinterpret_cast<const bf16x8*>(A + (long)(16 * i + row) * K + 32 * t + 8 * g);
        b[i] = *reinterpret_cast<const bf16x8*>(B + (long)(16 * i + row) * K + 32 * t + 8 * g);
      }
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j)
        for (int r = 0; r < 4; ++r) out16[(16 * i + 4 * g + r) * 32 + 16 * j + row] = acc[i][j][r];
  }
}

extern "C" int mfma_shape_bits(const void* A, const void* B, int steps, float* out32, float* out16, void* stream) {
  hipLaunchKernelGGL(mfma_shape_bits_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const unsigned short*)A,
                     (const unsigned short*)B, steps, out32, out16);
  return (int)hipGetLastError();
}
