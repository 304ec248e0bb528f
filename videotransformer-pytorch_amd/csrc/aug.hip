// aug.hip -- clip augmentation on decoded uint8 frames: random-resized crop + horizontal flip (one separable resampling
// kernel) and colour jitter, the steps of the reference's transforms_train (data_transform.py:495-531) that precede
// ToTensor + Normalize (those two live in patch_rows_u8_kernel, elementwise.hip).
//
// Arithmetic contract (what torchvision's tensor path computes, restated in tests/aug_ref.py):
//   * resampling = torch.nn.functional.interpolate(align_corners=False) of the cropped frame: a separable weighted sum,
//     x pass first, then y pass, both in float32 without fma contraction; the result is clamped to [0, 255] and rounded
//     half-to-even (torchvision's _cast_squeeze_out).  The weights come from vtx_resample_build_table (host, float64,
//     rounded once), so crop, border clamping, antialiasing and the flip are all in the tables and the kernel is one
//     weighted sum per axis whatever the mode;
//   * colour jitter = up to three blends  trunc(clamp(r * img + (1 - r) * other, 0, 255))  in a per-clip order: two float32
//     products and one add; `other` is 0 (brightness), the frame's mean grey (contrast) or the pixel's grey (saturation),
//     grey = trunc(0.2989 r + 0.587 g + 0.114 b).
//
// HBM-bound by bytes: a 256x340 -> 224x224 clip frame is 261 120 B read + 150 528 B written by the resampler, and the
// jitter moves 150 528 B two or three times (grey sum pass only for clips that draw contrast; read + write of the blend).
//
// Built into a library of its own, libvtx_aug.so (include/vtx_aug.h): it runs in front of the model and shares nothing with
// the training path, so libvtx.so keeps its export list and version.  The error plumbing and the version / last-error exports
// are VTX_SIDE_LIB(aug) (side_lib.h); the resampling band is resample_band.h, shared with views.hip and ragged.hip.
#include <math.h>
#include <string.h>
#include "side_lib.h"
#include "resample_band.h"
#include "../../include/vtx_aug.h"

VTX_SIDE_LIB(aug)

namespace vtx {

// ---- separable resampling: the band of resample_band.h, one destination ------------------------------------------------
__global__ __launch_bounds__(256) void clip_resample_u8_kernel(int T, int Hs, int Ws, int H, int W,
                                                               const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                               const int* __restrict__ xf, const int* __restrict__ xc,
                                                               const float* __restrict__ xw, int xt,
                                                               const int* __restrict__ yf, const int* __restrict__ yc,
                                                               const float* __restrict__ yw, int yt) {
  const int frame = blockIdx.z, b = frame / T;
  const int x = blockIdx.x * 256 + threadIdx.x;
  // idle lanes of the last column tile leave here (no barrier follows, and the y windows do not depend on the lane); a
  // store callable that tests `x < W` per row measured 2.7 % slower than the parent, this 1 % (inside its spread)
  if (x >= W) return;
  const long col = (long)b * W + x;
  const int r0 = blockIdx.y * BAND_ROWS;
  resample_band(src + (long)frame * Hs * Ws * 3, Hs, Ws, H, r0, xf[col], xc[col], xw + col * xt, xt,
                yf + (long)b * H, yc + (long)b * H, yw + (long)b * H * yt, yt, [=](int r, uint8_t q0, uint8_t q1, uint8_t q2) {
                  uint8_t* o = dst + (((long)frame * H + r0 + r) * W + x) * 3;
                  o[0] = q0; o[1] = q1; o[2] = q2;
                });
}

// ---- colour jitter ----------------------------------------------------------------------------------------------
enum { JIT_BRIGHTNESS = 0, JIT_CONTRAST = 1, JIT_SATURATION = 2 };

struct JitRec {
  int n, op[3];
  float r[3], q[3];                // blend weights: r and 1 - r, each rounded to float32 by the caller (torchvision forms 1.0 - r in float64)
};

__device__ inline JitRec jit_load(const int* __restrict__ ops, const float* __restrict__ fac, int b) {
  JitRec j;
  j.n = ops[b * 4];
  j.n = j.n < 0 ? 0 : (j.n > 3 ? 3 : j.n);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    j.op[i] = ops[b * 4 + 1 + i];
    j.r[i] = fac[b * 6 + i];
    j.q[i] = fac[b * 6 + 3 + i];
  }
  return j;
}

__device__ inline float jit_grey(float r, float g, float b) {
#pragma clang fp contract(off)
  return truncf(0.2989f * r + 0.587f * g + 0.114f * b);       // rgb_to_grayscale(...).to(uint8): values are >= 0
}
__device__ inline float jit_blend(float a, float other, float r, float q) {
#pragma clang fp contract(off)
  return truncf(fminf(fmaxf(r * a + q * other, 0.0f), 255.0f));
}

// ops [0, upto) of the record on one pixel; `mean` is read only by a contrast op (never below `upto` of the sum pass)
__device__ inline void jit_apply(const JitRec& j, int upto, float mean, float& r, float& g, float& b) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (i >= upto) break;
    const int op = j.op[i];
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
    if (op == JIT_CONTRAST) {
      o0 = o1 = o2 = mean;
    } else if (op == JIT_SATURATION) {
      o0 = o1 = o2 = jit_grey(r, g, b);
    }
    r = jit_blend(r, o0, j.r[i], j.q[i]);
    g = jit_blend(g, o1, j.r[i], j.q[i]);
    b = jit_blend(b, o2, j.r[i], j.q[i]);
  }
}

// position of the contrast op in the record, or -1
__device__ inline int jit_contrast_at(const JitRec& j) {
  int at = -1;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (i < j.n && j.op[i] == JIT_CONTRAST && at < 0) at = i;
  return at;
}

// VEC: four pixels = three aligned 32-bit words per thread (npix % 4 == 0 and a 4-byte aligned clip); else one pixel per thread
template <bool VEC>
__device__ inline void jit_load_px(const uint8_t* p, float (&v)[VEC ? 12 : 3]) {
  if constexpr (VEC) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const uint32_t u = w[i];
      v[4 * i] = (float)(u & 255u); v[4 * i + 1] = (float)((u >> 8) & 255u);
      v[4 * i + 2] = (float)((u >> 16) & 255u); v[4 * i + 3] = (float)(u >> 24);
    }
  } else {
    v[0] = (float)p[0]; v[1] = (float)p[1]; v[2] = (float)p[2];
  }
}

// pass 1 (clips that draw contrast): sums[frame] = sum of the greys of the frame as it stands in front of the contrast op.
// The ops before it are per-pixel, so they are recomputed here and nothing is written back.  Integer sum: exact and
// independent of the order of the atomics.
template <bool VEC>
__global__ __launch_bounds__(256) void clip_jitter_sum_kernel(int T, int npix, const uint8_t* __restrict__ clip,
                                                              const int* __restrict__ ops, const float* __restrict__ fac,
                                                              unsigned int* __restrict__ sums) {
  constexpr int PP = VEC ? 4 : 1;
  const int frame = blockIdx.y, b = frame / T;
  const JitRec j = jit_load(ops, fac, b);
  const int at = jit_contrast_at(j);
  if (at < 0) return;                                    // uniform per workgroup
  const uint8_t* img = clip + (long)frame * npix * 3;
  unsigned int tot = 0;
  for (int i = (blockIdx.x * 256 + threadIdx.x) * PP; i < npix; i += gridDim.x * 256 * PP) {
    float v[PP * 3];
    jit_load_px<VEC>(img + (long)i * 3, v);
#pragma unroll
    for (int p = 0; p < PP; ++p) {
      float r = v[3 * p], g = v[3 * p + 1], bl = v[3 * p + 2];
      jit_apply(j, at, 0.0f, r, g, bl);
      tot += (unsigned int)jit_grey(r, g, bl);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(sums + frame, tot);
}

// pass 2: every op of the record, in place
template <bool VEC>
__global__ __launch_bounds__(256) void clip_jitter_apply_kernel(int T, int npix, uint8_t* __restrict__ clip,
                                                                const int* __restrict__ ops, const float* __restrict__ fac,
                                                                const unsigned int* __restrict__ sums) {
  constexpr int PP = VEC ? 4 : 1;
  const int frame = blockIdx.y, b = frame / T;
  const JitRec j = jit_load(ops, fac, b);
  if (j.n == 0) return;
  // torch.mean of the float32 greys: their sum (an exact integer below 2^24 up to 65 793 pixels) divided once
  const float mean = jit_contrast_at(j) >= 0 ? (float)sums[frame] / (float)npix : 0.0f;
  uint8_t* img = clip + (long)frame * npix * 3;
  for (int i = (blockIdx.x * 256 + threadIdx.x) * PP; i < npix; i += gridDim.x * 256 * PP) {
    float v[PP * 3];
    jit_load_px<VEC>(img + (long)i * 3, v);
#pragma unroll
    for (int p = 0; p < PP; ++p) jit_apply(j, j.n, mean, v[3 * p], v[3 * p + 1], v[3 * p + 2]);
    if constexpr (VEC) {
      uint32_t* w = reinterpret_cast<uint32_t*>(img + (long)i * 3);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        w[k] = (uint32_t)v[4 * k] | ((uint32_t)v[4 * k + 1] << 8) | ((uint32_t)v[4 * k + 2] << 16) | ((uint32_t)v[4 * k + 3] << 24);
    } else {
      img[(long)i * 3] = (uint8_t)v[0]; img[(long)i * 3 + 1] = (uint8_t)v[1]; img[(long)i * 3 + 2] = (uint8_t)v[2];
    }
  }
}

// ---- host: the weight tables --------------------------------------------------------------------------------------
static double rs_cubic(double x, double a) {
  x = fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a;
  return 0.0;
}
static double rs_linear(double x) {
  x = fabs(x);
  return x < 1.0 ? 1.0 - x : 0.0;
}
static int rs_taps(int crop_len, int out_len, int mode, int antialias) {
  const int base = mode == VTX_RESAMPLE_BICUBIC ? 4 : 2;
  if (!antialias) return base;
  const double scale = (double)crop_len / (double)out_len;
  const double support = 0.5 * base * (scale >= 1.0 ? scale : 1.0);
  return (int)ceil(support) * 2 + 1;
}

}  // namespace vtx

using namespace vtx;

extern "C" int vtx_resample_max_taps(int crop_len, int out_len, int mode, int antialias) {
  VTX_REQUIRE(crop_len > 0 && out_len > 0 && (mode == VTX_RESAMPLE_BILINEAR || mode == VTX_RESAMPLE_BICUBIC), VTX_EINVAL,
              "resample_max_taps: crop_len=%d, out_len=%d must be positive, mode=%d bilinear (0) or bicubic (1)", crop_len, out_len, mode);
  return rs_taps(crop_len, out_len, mode, antialias);
}

extern "C" int vtx_resample_build_table(int src_len, int crop_start, int crop_len, int out_len, int mode, int antialias, int flip,
                                        int max_taps, int32_t* first, int32_t* count, float* weights) {
  VTX_REQUIRE(first && count && weights, VTX_EINVAL, "resample_build_table: null pointer");
  VTX_REQUIRE(mode == VTX_RESAMPLE_BILINEAR || mode == VTX_RESAMPLE_BICUBIC, VTX_EINVAL, "resample_build_table: mode=%d is neither bilinear (0) nor bicubic (1)", mode);
  VTX_REQUIRE(src_len > 0 && out_len > 0 && crop_len > 0 && crop_start >= 0 && crop_len <= src_len && crop_start <= src_len - crop_len, VTX_EINVAL,
              "resample_build_table: crop [%d, %d + %d) does not lie inside the source of length %d (out_len=%d)", crop_start, crop_start, crop_len, src_len, out_len);
  const int need = rs_taps(crop_len, out_len, mode, antialias);
  VTX_REQUIRE(max_taps >= need, VTX_EINVAL, "resample_build_table: max_taps=%d, vtx_resample_max_taps() = %d", max_taps, need);
  VTX_REQUIRE(need <= 4096, VTX_EINVAL, "resample_build_table: %d taps per output (a %d -> %d reduction) are not supported", need, crop_len, out_len);
  const bool cubic = mode == VTX_RESAMPLE_BICUBIC;
  const double scale = (double)crop_len / (double)out_len;
  double w[4097];
  for (int i = 0; i < out_len; ++i) {
    int lo = 0, n = 0;                                   // taps lo .. lo + n - 1 of the crop, weights w[0 .. n-1]
    if (!antialias) {
      double c = scale * ((double)i + 0.5) - 0.5;
      if (!cubic && c < 0.0) c = 0.0;
      const double fl = floor(c);
      const double t = c - fl;
      const int i0 = (int)fl;
      double coef[4];
      int idx0, nt;
      if (cubic) {
        const double a = -0.75;
        coef[0] = rs_cubic(t + 1.0, a); coef[1] = rs_cubic(t, a); coef[2] = rs_cubic(1.0 - t, a); coef[3] = rs_cubic(2.0 - t, a);
        idx0 = i0 - 1; nt = 4;
      } else {
        coef[0] = 1.0 - t; coef[1] = t;
        idx0 = i0; nt = 2;
      }
      // taps beyond the crop fold onto its border sample
      auto clampi = [&](int v) { return v < 0 ? 0 : (v > crop_len - 1 ? crop_len - 1 : v); };
      lo = clampi(idx0);
      n = clampi(idx0 + nt - 1) - lo + 1;
      for (int k = 0; k < n; ++k) w[k] = 0.0;
      for (int k = 0; k < nt; ++k) w[clampi(idx0 + k) - lo] += coef[k];
    } else {
      const double sc = scale >= 1.0 ? scale : 1.0;
      const double support = (cubic ? 2.0 : 1.0) * sc;
      const double c = scale * ((double)i + 0.5);
      long xmin = (long)(c - support + 0.5);
      if (xmin < 0) xmin = 0;
      long xmax = (long)(c + support + 0.5);
      if (xmax > crop_len) xmax = crop_len;
      lo = (int)xmin;
      n = (int)(xmax - xmin);
      VTX_REQUIRE(n > 0 && n <= need, VTX_EINVAL, "resample_build_table: output %d has %d taps (at most %d expected)", i, n, need);
      double tot = 0.0;
      for (int k = 0; k < n; ++k) {
        const double u = ((double)(k + lo) - c + 0.5) / sc;
        w[k] = cubic ? rs_cubic(u, -0.5) : rs_linear(u);
        tot += w[k];
      }
      for (int k = 0; k < n; ++k) w[k] /= tot;
    }
    // taps of weight zero at either end are dropped: an identity crop is ONE tap of weight 1.0
    int k0 = 0, k1 = n;
    while (k1 - k0 > 1 && w[k1 - 1] == 0.0) --k1;
    while (k1 - k0 > 1 && w[k0] == 0.0) ++k0;
    const int o = flip ? out_len - 1 - i : i;
    first[o] = crop_start + lo + k0;
    count[o] = k1 - k0;
    for (int k = k0; k < k1; ++k) weights[(long)o * max_taps + (k - k0)] = (float)w[k];
  }
  return VTX_OK;
}

extern "C" int vtx_clip_resample_u8(int B, int T, int Hs, int Ws, int H, int W, const unsigned char* src, unsigned char* dst,
                                    const int32_t* x_first, const int32_t* x_count, const float* x_weights, int x_taps,
                                    const int32_t* y_first, const int32_t* y_count, const float* y_weights, int y_taps, void* stream) {
  VTX_REQUIRE(B > 0 && T > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && x_taps > 0 && y_taps > 0, VTX_EINVAL,
              "clip_resample_u8: B=%d T=%d source %dx%d output %dx%d taps %d/%d must all be positive", B, T, Hs, Ws, H, W, x_taps, y_taps);
  VTX_REQUIRE(src && dst && x_first && x_count && x_weights && y_first && y_count && y_weights, VTX_EINVAL, "clip_resample_u8: null pointer");
  VTX_REQUIRE(src != dst, VTX_EINVAL, "clip_resample_u8: in place is not supported");
  const long bands = (H + BAND_ROWS - 1) / BAND_ROWS;
  VTX_REQUIRE((long)B * T <= 65535 && bands <= 65535, VTX_EINVAL, "clip_resample_u8: %ld frames / %ld row bands exceed the grid (65535 each)", (long)B * T, bands);
  dim3 grid((unsigned)((W + 255) / 256), (unsigned)bands, (unsigned)(B * T));
  hipLaunchKernelGGL(clip_resample_u8_kernel, grid, dim3(256), 0, as_stream(stream), T, Hs, Ws, H, W, src, dst,
                     x_first, x_count, x_weights, x_taps, y_first, y_count, y_weights, y_taps);
  return check_launch("clip_resample_u8");
}

extern "C" size_t vtx_clip_jitter_workspace(int B, int T) { return B > 0 && T > 0 ? (size_t)B * T * sizeof(unsigned int) : 0; }

extern "C" int vtx_clip_jitter_u8(int B, int T, int H, int W, unsigned char* clip, const int32_t* ops, const float* factors,
                                  void* workspace, size_t ws_bytes, void* stream) {
  VTX_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0, VTX_EINVAL, "clip_jitter_u8: B=%d T=%d H=%d W=%d must all be positive", B, T, H, W);
  VTX_REQUIRE(clip && ops && factors && workspace, VTX_EINVAL, "clip_jitter_u8: null pointer");
  VTX_REQUIRE((long)H * W <= 16000000L, VTX_EINVAL, "clip_jitter_u8: %dx%d frames overflow the 32-bit grey sum", H, W);
  VTX_REQUIRE((long)B * T <= 65535, VTX_EINVAL, "clip_jitter_u8: %ld frames exceed the grid (65535)", (long)B * T);
  VTX_REQUIRE(ws_bytes >= vtx_clip_jitter_workspace(B, T), VTX_EWS, "clip_jitter_u8: workspace of %zu bytes, vtx_clip_jitter_workspace() = %zu",
              ws_bytes, vtx_clip_jitter_workspace(B, T));
  VTX_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, VTX_EALIGN, "clip_jitter_u8: workspace must be 4-byte aligned");
  const int npix = H * W;
  const bool vec = npix % 4 == 0 && (reinterpret_cast<uintptr_t>(clip) & 3u) == 0;
  hipStream_t st = as_stream(stream);
  unsigned int* sums = reinterpret_cast<unsigned int*>(workspace);
  if (hipMemsetAsync(sums, 0, (size_t)B * T * sizeof(unsigned int), st) != hipSuccess) {
    set_error("clip_jitter_u8: hipMemsetAsync failed");
    return VTX_ELAUNCH;
  }
  const int per = vec ? 1024 : 256;                      // pixels per workgroup and trip
  long gx = (npix + per - 1) / per; if (gx > 64) gx = 64;
  dim3 grid((unsigned)gx, (unsigned)(B * T));
  if (vec) {
    hipLaunchKernelGGL(clip_jitter_sum_kernel<true>, grid, dim3(256), 0, st, T, npix, clip, ops, factors, sums);
    hipLaunchKernelGGL(clip_jitter_apply_kernel<true>, grid, dim3(256), 0, st, T, npix, clip, ops, factors, sums);
  } else {
    hipLaunchKernelGGL(clip_jitter_sum_kernel<false>, grid, dim3(256), 0, st, T, npix, clip, ops, factors, sums);
    hipLaunchKernelGGL(clip_jitter_apply_kernel<false>, grid, dim3(256), 0, st, T, npix, clip, ops, factors, sums);
  }
  return check_launch("clip_jitter_u8");
}
