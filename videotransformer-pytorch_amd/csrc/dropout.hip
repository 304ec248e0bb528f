// dropout.hip -- element-wise dropout whose mask is a pure function of (seed, site, element index, p): it is never stored,
// the backward launch regenerates it (reference transformer.py:176,265,498-507 nn.Dropout; video_transformer.py:212,238,474,
// 500,523 drop_after_pos / drop_after_time).  The contract is written down at vtx_dropout_rows in include/vtx_dropout.h.
// One thread per 8 consecutive columns = two Philox4x32-10 evaluations, one 16-byte (bf16) or two 16-byte (fp32) accesses per
// operand; the kernel streams every byte once.
//
// A library of its own, libvtx_dropout.so (include/vtx_dropout.h): the other seven keep their export lists and versions.
// Error plumbing, version and last-error exports: VTX_SIDE_LIB(dropout) (side_lib.h).
#include "side_lib.h"
#include "philox.h"
#include "../../include/vtx_dropout.h"

VTX_SIDE_LIB(dropout)

namespace vtx {

// Grid-stride with a capped grid: at most DROPOUT_GRID_CAP workgroups of 256 threads, i.e. launches of more than
// DROPOUT_GRID_CAP * 256 * 8 = 8 388 608 elements take a second trip (vtx/ops.py mirrors the two numbers for the tests).
constexpr int DROPOUT_GRID_CAP = 4096;
constexpr int DROPOUT_BLOCK = 256;

template <typename T>
__global__ __launch_bounds__(DROPOUT_BLOCK) void dropout_rows_kernel(
    int rows, int D, const T* x, long ldx, vtx_rowmap xmap, T* y, long ldy, vtx_rowmap ymap, const T* post, long ldp,
    vtx_rowmap pmap, const float* __restrict__ pre, int pre_period, const float* __restrict__ s, int d1, int m1, int d2, int m2,
    unsigned long long thr, float scale, uint32_t k0, uint32_t k1, uint32_t site, unsigned long long e0) {
#pragma clang fp contract(off)
  const long per = D / 8;
  const long total = (long)rows * per;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long m = idx / per;
    const int c = (int)(idx - m * per) * 8;
    float v[8];
    load8(x + map_row(xmap, m) * ldx + c, v);
    if (pre) {
      float a[8];
      load8(pre + (m % pre_period) * (long)D + c, a);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] + a[j];
    }
    // element e = e0 + m D + c is a multiple of 4: counters e / 4 and e / 4 + 1, word j & 3 of each
    const unsigned long long q = (e0 + (unsigned long long)m * (unsigned long long)D + (unsigned long long)c) >> 2;
    uint32_t w[8];
    {
      uint32_t o[4];
      philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), site, 0u, k0, k1, o);
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = o[j];
      const unsigned long long q1 = q + 1;
      philox4x32_10((uint32_t)q1, (uint32_t)(q1 >> 32), site, 0u, k0, k1, o);
#pragma unroll
      for (int j = 0; j < 4; ++j) w[4 + j] = o[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = ((unsigned long long)w[j] < thr) ? 0.0f : v[j] * scale;
    if (s) {
      const float sc = s[(m / d1) * m1 + (m % d2) * m2];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] * sc;
    }
    if (post) {
      float r[8];
      load8(post + map_row(pmap, m) * ldp + c, r);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] + r[j];
    }
    store8(y + map_row(ymap, m) * ldy + c, v);
  }
}

}  // namespace vtx

using namespace vtx;

extern "C" int vtx_dropout_rows(int dtype, int rows, int D, const void* x, long ldx, vtx_rowmap xmap, void* y, long ldy,
                                vtx_rowmap ymap, const void* post, long ldp, vtx_rowmap pmap, const float* pre, int pre_period,
                                const float* s, int rs_d1, int rs_m1, int rs_d2, int rs_m2, unsigned long long thr, float scale,
                                unsigned long long seed, unsigned int site, unsigned long long e0, void* stream) {
  VTX_REQUIRE(x && y, VTX_EINVAL, "dropout_rows: null pointer");
  VTX_REQUIRE(rows > 0 && D > 0, VTX_EINVAL, "dropout_rows: rows and D must be positive");
  VTX_REQUIRE(D % 8 == 0, VTX_EINVAL, "dropout_rows: D must be a multiple of 8 (got %d)", D);
  VTX_REQUIRE(e0 % 4 == 0, VTX_EINVAL, "dropout_rows: e0 must be a multiple of 4");
  VTX_REQUIRE(thr <= (1ull << 32), VTX_EINVAL, "dropout_rows: thr must lie in [0, 2^32]");
  VTX_REQUIRE(dtype == VTX_F32 || dtype == VTX_BF16, VTX_EINVAL, "dropout_rows: bad dtype %d", dtype);
  VTX_REQUIRE(!pre || pre_period > 0, VTX_EINVAL, "dropout_rows: pre needs pre_period > 0");
  VTX_REQUIRE(!s || (rs_d1 > 0 && rs_d2 > 0), VTX_EINVAL, "dropout_rows: divisors must be > 0");
  VTX_REQUIRE(ldx >= D && ldy >= D && (!post || ldp >= D), VTX_EINVAL, "dropout_rows: leading dimension smaller than D");
  VTX_REQUIRE(aligned16(x) && aligned16(y) && aligned16(post) && aligned16(pre) && ldx % 8 == 0 && ldy % 8 == 0 &&
              (!post || ldp % 8 == 0), VTX_EALIGN, "dropout_rows: 16-byte aligned pointers and leading dimensions that are multiples of 8 required");
  const long work = (long)rows * (D / 8);
  long g = (work + DROPOUT_BLOCK - 1) / DROPOUT_BLOCK;
  if (g > DROPOUT_GRID_CAP) g = DROPOUT_GRID_CAP;
  dim3 grid((unsigned)g), block(DROPOUT_BLOCK);
  hipStream_t st = as_stream(stream);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  if (dtype == VTX_F32)
    hipLaunchKernelGGL(dropout_rows_kernel<float>, grid, block, 0, st, rows, D, (const float*)x, ldx, xmap, (float*)y, ldy, ymap,
                       (const float*)post, ldp, pmap, pre, pre_period, s, rs_d1, rs_m1, rs_d2, rs_m2, thr, scale, k0, k1,
                       (uint32_t)site, e0);
  else
    hipLaunchKernelGGL(dropout_rows_kernel<bf16raw>, grid, block, 0, st, rows, D, (const bf16raw*)x, ldx, xmap, (bf16raw*)y, ldy,
                       ymap, (const bf16raw*)post, ldp, pmap, pre, pre_period, s, rs_d1, rs_m1, rs_d2, rs_m2, thr, scale, k0, k1,
                       (uint32_t)site, e0);
  return check_launch("dropout_rows");
}
