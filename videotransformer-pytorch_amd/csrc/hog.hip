// hog.hip -- MaskFeat HOG target extractor and the MaskFeat head's small kernels.
//
// HOG: reference dataset.py:39-45 -> skimage.feature.hog(orientations=9,
// pixels_per_cell=(8,8), cells_per_block=(1,1), block_norm='L2') per channel.
// Bit-exact contract (see oracle/hog_oracle.py for the derivation):
//   * gradients are integer central differences (0 on the image border);
//   * the orientation bin is decided without atan2 and without floating point: skimage's interval test equals the eight
//     sign tests  g_row cos(20k) - g_col sin(20k) >= 0  (proven for all 261 121 integer gradient pairs, oracle tests), and
//     those equal  |g_col| <= floor(g_row cot(20j))  for j = 1..4 with the sign of g_col choosing the half -- four
//     fixed-point products (g cot is never within 2.6e-4 of an integer for g <= 255: 16 fraction bits decide it);
//     vtx_selftest checks the integer rule against the double rule for every pair ON THE DEVICE;
//   * magnitude = libm hypot(g_col, g_row) of the HOST (what numpy calls): for the 65 536 integer pairs it differs from
//     the correctly rounded sqrt(g_row^2 + g_col^2) in 300 entries by one ulp (glibc 2.35), so the kernel computes the
//     correctly rounded square root (device sqrt) and adds a 2-bit correction looked up in a 16-KB table that
//     vtx_hog_build_table derives from the host's hypot (round 4 gathered the 512-KB double table per pixel: the
//     vector L1 fills, not the arithmetic, bounded it); vtx_selftest compares all 65 536 magnitudes with the host table;
//   * per (cell, bin): the magnitudes of that bin's pixels are accumulated in row-major order into a float32
//     accumulator with double adds, divided by 64 in float32 (pixels with magnitude 0 leave the accumulator unchanged);
//   * per cell: L2 norm in float64 with numpy's pairwise order for 9 terms.
// HBM-bound by bytes: 150 528 B read + 169 344 B written per 224x224 frame.
//
// Round 5 kernel.  One persistent workgroup per (frame, cell row) item for ALL THREE channels: the ten pixel rows of a
// strip are one contiguous 30 W-byte block of the interleaved RGB frame, fetched with 16-byte loads (every byte once per
// strip; round 4: one workgroup per channel, stride-3 byte loads, each row three times).  Per channel: (A) a thread per
// pixel column walks the eight rows -- gradient, integer bin, magnitude -> LDS, and ONE LDS atomic OR that sets the
// pixel's bit in the 64-bit mask of its (cell, bin); (B) a thread per (cell, bin) walks only the SET bits of its mask in
// ascending (= row-major) order -- on average 7 double adds instead of 64 compare-and-maybe-add steps; then (C) the
// norms, and the 27 features of a cell leave as 16-byte stores (two horizontally adjacent cells = 432 contiguous bytes).
// The kernel, its device functions and its launch live in hog_kernel.h: libvtx_stem.so (stem.hip) runs the same code for the
// selected frames of a clip batch.
#include <math.h>
#include <string.h>
#include <vector>
#include "hog_kernel.h"

namespace vtx {

__constant__ double HOG_BC[8] = {0.93969262078590838, 0.76604444311897804, 0.5, 0.17364817766693035,
                                 -0.17364817766693035, -0.5, -0.76604444311897804, -0.93969262078590838};
__constant__ double HOG_BS[8] = {0.34202014332566873, 0.64278760968653933, 0.8660254037844386, 0.98480775301220806,
                                 0.98480775301220806, 0.8660254037844386, 0.64278760968653933, 0.34202014332566873};

// the eight sign tests in float64 (round 1 - 4 kernel; kept as the device-side cross-check of the integer rule)
__device__ inline int hog_bin_f64(int gr, int gc) {
  if (gr == 0 && gc == 0) return 0;
  if (gr < 0 || (gr == 0 && gc < 0)) { gr = -gr; gc = -gc; }
  int b = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) b += (HOG_BC[k] * (double)gr - HOG_BS[k] * (double)gc >= 0.0) ? 1 : 0;
  return b;
}

// vtx_selftest: every gradient pair through the device functions above -- magnitudes [256*256] and both bin rules [511*511]
__global__ void hog_probe_kernel(const uint32_t* __restrict__ exc, double* __restrict__ mags, int* __restrict__ bin_int,
                                 int* __restrict__ bin_f64) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 65536) mags[i] = hog_mag(i >> 8, i & 255, exc[i >> 4]);
  if (i < 511 * 511) {
    const int gr = i / 511 - 255, gc = i % 511 - 255;
    bin_int[i] = hog_bin(gr, gc);
    bin_f64[i] = hog_bin_f64(gr, gc);
  }
}

// ---- MaskFeat mask-token blend (video_transformer.py:914-919) ------------------------
template <typename T>
__global__ void mf_blend_fwd_kernel(long rows, int Tq, int Hq, int Wq, int C, int g, const T* __restrict__ x,
                                    const uint8_t* __restrict__ mask, const float* __restrict__ tok, T* __restrict__ out) {
  const long per = C / 8;
  const int r = Hq / g;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < rows * per; idx += (long)gridDim.x * blockDim.x) {
    const long row = idx / per;
    const int c = (int)(idx - row * per) * 8;
    long q = row;
    const int w = (int)(q % Wq); q /= Wq;
    const int h = (int)(q % Hq); q /= Hq;
    const int t = (int)(q % Tq); q /= Tq;
    const uint8_t mk = mask[((q * Tq + t) * g + h / r) * g + w / r];
    float v[8];
    if (mk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = tok[c + j];
    } else {
      load8(x + row * C + c, v);
    }
    store8(out + row * C + c, v);
  }
}

template <typename T>
__global__ void mf_blend_bwd_kernel(long rows, int Tq, int Hq, int Wq, int C, int g, const T* __restrict__ dy,
                                    const uint8_t* __restrict__ mask, T* __restrict__ dx, float* __restrict__ dtok) {
  // grid.x covers column chunks of 8, grid.y strides rows; per-block partial of dtoken via atomics (C is tiny: 96)
  const int c = blockIdx.x * 8;
  const int r = Hq / g;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long row = (long)blockIdx.y * blockDim.x + threadIdx.x; row < rows; row += (long)gridDim.y * blockDim.x) {
    long q = row;
    const int w = (int)(q % Wq); q /= Wq;
    const int h = (int)(q % Hq); q /= Hq;
    const int t = (int)(q % Tq); q /= Tq;
    const uint8_t mk = mask[((q * Tq + t) * g + h / r) * g + w / r];
    float v[8];
    load8(dy + row * C + c, v);
    if (mk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { acc[j] += v[j]; v[j] = 0.f; }
    }
    store8(dx + row * C + c, v);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float s = wave_sum(acc[j]);
    if ((threadIdx.x & 63) == 0 && s != 0.f) atomicAdd(dtok + c + j, s);
  }
}

// ---- masked MSE (video_transformer.py:882-901) ----------------------------------------
// pred row (b, tq, h, w) holds ts*Cf features: frame tq*ts+dt uses features [dt*Cf, (dt+1)*Cf).
// One wave per (b, frame, h, w) cell of the target grid; skips cells with cmask == 0.
template <typename T>
__global__ __launch_bounds__(256) void mf_loss_fwd_kernel(long cells, int Tq, int ts, int g, int Cf, const T* __restrict__ pred,
                                                          long ldp, const double* __restrict__ target,
                                                          const uint8_t* __restrict__ cmask, double* __restrict__ acc2) {
  const int lane = threadIdx.x & 63;
  const long wave0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  double lsum = 0.0, msum = 0.0;
  for (long cell = wave0; cell < cells; cell += nwaves) {
    if (!cmask[cell]) continue;
    long q = cell;
    const int w = (int)(q % g); q /= g;
    const int h = (int)(q % g); q /= g;
    const int fr = (int)(q % (Tq * ts)); q /= (Tq * ts);
    const int tq = fr / ts, dt = fr - tq * ts;
    const T* pr = pred + (((q * Tq + tq) * g + h) * g + w) * ldp + dt * Cf;
    const double* tg = target + cell * Cf;
    double e = 0.0;
    for (int k = lane; k < Cf; k += 64) {
      const double d = (double)ET<T>::ld(pr + k) - tg[k];
      e += d * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
    lsum += e / (double)Cf;
    msum += 1.0;
  }
  if (lane == 0 && msum != 0.0) {
    atomicAdd(acc2, lsum);
    atomicAdd(acc2 + 1, msum);
  }
}
// The reference computes `mask.sum() + 1e-5` on an int32 mask: the integer sum is promoted to
// float32 (video_transformer.py:901), so the denominator is float32(sum + 1e-5).
__device__ inline double mf_denominator(double msum) { return (double)((float)msum + 1e-5f); }
__global__ void mf_loss_finish_kernel(double* acc2) { acc2[0] = acc2[0] / mf_denominator(acc2[1]); }

template <typename T>
__global__ __launch_bounds__(256) void mf_loss_bwd_kernel(long rows, int Tq, int ts, int g, int Cf, const T* __restrict__ pred,
                                                          long ldp, const double* __restrict__ target,
                                                          const uint8_t* __restrict__ cmask, const double* __restrict__ acc2,
                                                          float gloss, T* __restrict__ dpred, long lddp) {
  // one thread per element of pred [rows, ts*Cf]
  const long total = rows * ts * Cf;
  const double coef = (double)gloss * 2.0 / ((double)Cf * mf_denominator(acc2[1]));
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long row = idx / (ts * Cf);
    const int col = (int)(idx - row * (ts * Cf));
    const int dt = col / Cf, k = col - dt * Cf;
    long q = row;
    const int w = (int)(q % g); q /= g;
    const int h = (int)(q % g); q /= g;
    const int tq = (int)(q % Tq); q /= Tq;
    const long cell = ((q * (Tq * ts) + tq * ts + dt) * g + h) * g + w;
    float gv = 0.f;
    if (cmask[cell]) gv = (float)(coef * ((double)ET<T>::ld(pred + row * ldp + col) - target[cell * Cf + k]));
    ET<T>::st(dpred + row * lddp + col, gv);
  }
}

}  // namespace vtx

using namespace vtx;

extern "C" size_t vtx_hog_table_bytes(void) { return (size_t)256 * 256 * sizeof(double) + (size_t)HOG_EXC_WORDS * sizeof(uint32_t); }

// [65 536 doubles: the host's hypot(c, r)] [4096 words: per pair, 2 bits = hypot minus the correctly rounded sqrt(r^2 + c^2) in ulps]
extern "C" int vtx_hog_build_table(double* host_table) {
  VTX_REQUIRE(host_table != nullptr, VTX_EINVAL, "hog_build_table: null pointer");
  uint32_t* exc = reinterpret_cast<uint32_t*>(host_table + 256 * 256);
  for (int w = 0; w < HOG_EXC_WORDS; ++w) exc[w] = 0u;
  for (int r = 0; r < 256; ++r)
    for (int c = 0; c < 256; ++c) {
      const double h = hypot((double)c, (double)r);
      const double q = sqrt((double)(r * r + c * c));          // the integer is exact, the host square root correctly rounded
      host_table[r * 256 + c] = h;
      long long hb, qb;
      memcpy(&hb, &h, 8);
      memcpy(&qb, &q, 8);
      const long long d = hb - qb;
      VTX_REQUIRE(d >= -1 && d <= 1, VTX_EINVAL, "hog_build_table: hypot(%d, %d) is %lld ulps from the rounded square root", c, r, d);
      const int idx = r * 256 + c;
      exc[idx >> 4] |= (uint32_t)(d & 3) << (2 * (idx & 15));
    }
  return VTX_OK;
}

namespace vtx {
// part of vtx_selftest (api.hip): 0 = the device reproduces the host's hypot for all 65 536 gradient pairs and the integer
// bin rule equals the float64 sign tests for all 511 x 511 pairs
int hog_selftest(int* bad_mag, int* bad_bin) {
  // (defined counts on every path -- 0 mismatches can only come from a completed comparison --, every device buffer
  // freed on every path, every runtime call checked)
  *bad_mag = 65536; *bad_bin = 511 * 511;
  std::vector<double> tab(vtx_hog_table_bytes() / 8);
  if (vtx_hog_build_table(tab.data()) != VTX_OK) return -1;
  uint32_t* d_exc = nullptr; double* d_mag = nullptr; int *d_bi = nullptr, *d_bf = nullptr;
  const int NB = 511 * 511;
  std::vector<double> mags(65536);
  std::vector<int> bi(NB), bf(NB);
  bool ok = hipMalloc(&d_exc, HOG_EXC_WORDS * 4) == hipSuccess && hipMalloc(&d_mag, 65536 * 8) == hipSuccess &&
            hipMalloc(&d_bi, NB * 4) == hipSuccess && hipMalloc(&d_bf, NB * 4) == hipSuccess;
  ok = ok && hipMemcpy(d_exc, tab.data() + 65536, HOG_EXC_WORDS * 4, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(hog_probe_kernel, dim3((NB + 255) / 256), dim3(256), 0, 0, d_exc, d_mag, d_bi, d_bf);
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  }
  ok = ok && hipMemcpy(mags.data(), d_mag, 65536 * 8, hipMemcpyDeviceToHost) == hipSuccess &&
       hipMemcpy(bi.data(), d_bi, NB * 4, hipMemcpyDeviceToHost) == hipSuccess &&
       hipMemcpy(bf.data(), d_bf, NB * 4, hipMemcpyDeviceToHost) == hipSuccess;
  if (d_exc) (void)hipFree(d_exc);
  if (d_mag) (void)hipFree(d_mag);
  if (d_bi) (void)hipFree(d_bi);
  if (d_bf) (void)hipFree(d_bf);
  if (!ok) return -1;
  *bad_mag = 0; *bad_bin = 0;
  for (int i = 0; i < 65536; ++i) *bad_mag += memcmp(&mags[i], &tab[i], 8) != 0;
  for (int i = 0; i < NB; ++i) *bad_bin += bi[i] != bf[i];
  return 0;
}
}  // namespace vtx

extern "C" int vtx_hog_fwd(const uint8_t* frames, int F, int H, int W, const double* table, size_t table_bytes, double* out,
                           int32_t* bins, void* stream) {
  VTX_REQUIRE(F >= 0 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0 && W <= 1024, VTX_EINVAL,
              "hog_fwd: H=%d, W=%d must be multiples of 16 (W <= 1024)", H, W);
  if (F == 0) return VTX_OK;                       // empty batch: nothing to do (pointers may be null)
  VTX_REQUIRE(frames && table && out, VTX_EINVAL, "hog_fwd: null pointer");
  // the blob is 512 KB of magnitudes + the 16 KB of correction words the kernel reads: a caller that still uploads the
  // magnitude table of library version 200 and earlier (512 KB) would have the kernel read 16 KB beyond it
  VTX_REQUIRE(table_bytes >= vtx_hog_table_bytes(), VTX_EINVAL, "hog_fwd: the table blob holds %zu bytes, vtx_hog_table_bytes() = %zu "
              "(magnitudes + correction words: build it with vtx_hog_build_table)", table_bytes, vtx_hog_table_bytes());
  VTX_REQUIRE(aligned16(frames) && aligned16(out), VTX_EALIGN, "hog_fwd: frames and out must be 16-byte aligned");
  return hog_launch("hog_fwd", frames, F, H, W, table, out, bins, nullptr, F, stream);     // (hog_kernel.h)
}

extern "C" int vtx_maskfeat_blend_fwd(int dtype, int B, int Tq, int Hq, int Wq, int C, int g, const void* x,
                                      const uint8_t* mask, const float* mask_token, void* out, void* stream) {
  VTX_REQUIRE(B > 0 && C % 8 == 0 && g > 0 && Hq % g == 0 && Wq % g == 0 && Hq / g == Wq / g && x && mask && mask_token && out,
              VTX_EINVAL, "maskfeat_blend_fwd: bad arguments");
  const long rows = (long)B * Tq * Hq * Wq;
  long gsz = (rows * (C / 8) + 255) / 256; if (gsz > 8192) gsz = 8192;
  dim3 grid((unsigned)gsz), block(256);
  hipStream_t st = as_stream(stream);
  if (dtype == VTX_F32)
    hipLaunchKernelGGL(mf_blend_fwd_kernel<float>, grid, block, 0, st, rows, Tq, Hq, Wq, C, g, (const float*)x, mask, mask_token, (float*)out);
  else if (dtype == VTX_BF16)
    hipLaunchKernelGGL(mf_blend_fwd_kernel<bf16raw>, grid, block, 0, st, rows, Tq, Hq, Wq, C, g, (const bf16raw*)x, mask, mask_token, (bf16raw*)out);
  else
    VTX_REQUIRE(false, VTX_EINVAL, "maskfeat_blend_fwd: bad dtype");
  return check_launch("maskfeat_blend_fwd");
}

extern "C" int vtx_maskfeat_blend_bwd(int dtype, int B, int Tq, int Hq, int Wq, int C, int g, const void* dy,
                                      const uint8_t* mask, void* dx, float* dtoken, void* stream) {
  VTX_REQUIRE(B > 0 && C % 8 == 0 && g > 0 && Hq % g == 0 && Wq % g == 0 && dy && mask && dx && dtoken, VTX_EINVAL,
              "maskfeat_blend_bwd: bad arguments");
  const long rows = (long)B * Tq * Hq * Wq;
  long gy = (rows + 255) / 256; if (gy > 1024) gy = 1024;
  dim3 grid(C / 8, (unsigned)gy), block(256);
  hipStream_t st = as_stream(stream);
  hipMemsetAsync(dtoken, 0, (size_t)C * sizeof(float), st);
  if (dtype == VTX_F32)
    hipLaunchKernelGGL(mf_blend_bwd_kernel<float>, grid, block, 0, st, rows, Tq, Hq, Wq, C, g, (const float*)dy, mask, (float*)dx, dtoken);
  else if (dtype == VTX_BF16)
    hipLaunchKernelGGL(mf_blend_bwd_kernel<bf16raw>, grid, block, 0, st, rows, Tq, Hq, Wq, C, g, (const bf16raw*)dy, mask, (bf16raw*)dx, dtoken);
  else
    VTX_REQUIRE(false, VTX_EINVAL, "maskfeat_blend_bwd: bad dtype");
  return check_launch("maskfeat_blend_bwd");
}

extern "C" int vtx_maskfeat_loss_fwd(int dtype, int B, int Tq, int ts, int g, int Cf, const void* pred, long ldp,
                                     const double* target, const uint8_t* cmask, double* loss_out, void* stream) {
  VTX_REQUIRE(B > 0 && Tq > 0 && ts > 0 && g > 0 && Cf > 0 && pred && target && cmask && loss_out, VTX_EINVAL,
              "maskfeat_loss_fwd: bad arguments");
  const long cells = (long)B * Tq * ts * g * g;
  hipStream_t st = as_stream(stream);
  hipMemsetAsync(loss_out, 0, 2 * sizeof(double), st);
  long gsz = (cells * 64 + 255) / 256; if (gsz > 2048) gsz = 2048;
  dim3 grid((unsigned)gsz), block(256);
  if (dtype == VTX_F32)
    hipLaunchKernelGGL(mf_loss_fwd_kernel<float>, grid, block, 0, st, cells, Tq, ts, g, Cf, (const float*)pred, ldp, target, cmask, loss_out);
  else if (dtype == VTX_BF16)
    hipLaunchKernelGGL(mf_loss_fwd_kernel<bf16raw>, grid, block, 0, st, cells, Tq, ts, g, Cf, (const bf16raw*)pred, ldp, target, cmask, loss_out);
  else
    VTX_REQUIRE(false, VTX_EINVAL, "maskfeat_loss_fwd: bad dtype");
  hipLaunchKernelGGL(mf_loss_finish_kernel, dim3(1), dim3(1), 0, st, loss_out);
  return check_launch("maskfeat_loss_fwd");
}

extern "C" int vtx_maskfeat_loss_bwd(int dtype, int B, int Tq, int ts, int g, int Cf, const void* pred, long ldp,
                                     const double* target, const uint8_t* cmask, const double* loss_out, float gloss,
                                     void* dpred, long lddp, void* stream) {
  VTX_REQUIRE(B > 0 && pred && target && cmask && loss_out && dpred, VTX_EINVAL, "maskfeat_loss_bwd: bad arguments");
  const long rows = (long)B * Tq * g * g;
  long gsz = (rows * ts * Cf + 255) / 256; if (gsz > 8192) gsz = 8192;
  dim3 grid((unsigned)gsz), block(256);
  hipStream_t st = as_stream(stream);
  if (dtype == VTX_F32)
    hipLaunchKernelGGL(mf_loss_bwd_kernel<float>, grid, block, 0, st, rows, Tq, ts, g, Cf, (const float*)pred, ldp, target, cmask, loss_out, gloss, (float*)dpred, lddp);
  else if (dtype == VTX_BF16)
    hipLaunchKernelGGL(mf_loss_bwd_kernel<bf16raw>, grid, block, 0, st, rows, Tq, ts, g, Cf, (const bf16raw*)pred, ldp, target, cmask, loss_out, gloss, (bf16raw*)dpred, lddp);
  else
    VTX_REQUIRE(false, VTX_EINVAL, "maskfeat_loss_bwd: bad dtype");
  return check_launch("maskfeat_loss_bwd");
}
