// randaug.hip -- RandAugment on decoded uint8 clips [B,T,H,W,3]: the `auto_augment` branch of the reference's transforms_train
// (data_transform.py:520-521: transforms.autoaugment.RandAugment() in place of ColorJitter).  The kernels are the op
// families of torchvision's RandAugment._apply_op on its tensor path that csrc/aug.hip does not have already:
//   * vtx_clip_warp_nearest_u8   ShearX / ShearY / TranslateX / TranslateY / Rotate: F.affine / F.rotate, nearest, fill 0;
//   * vtx_clip_sharpness_u8      adjust_sharpness: 3x3 stencil ([1 1 1; 1 5 1; 1 1 1] / 13) blended with the frame;
//   * vtx_clip_pointwise_u8      posterize and solarize;
//   * vtx_clip_autocontrast_u8   per (frame, channel) min / max, then the stretch;
//   * vtx_clip_equalize_u8       per (frame, channel) histogram, then a look-up table from its prefix sum.
// Brightness, Color and Contrast are the three blends of vtx_clip_jitter_u8 (libvtx_aug.so) and are not repeated here.
//
// Arithmetic contract (restated in tests/randaug_ref.py): everything is integer arithmetic or a float32 expression of
// single-rounded steps without fma contraction, so every result but the warp's is torchvision's byte for byte; the warp
// evaluates its source coordinate in float32 in another order than affine_grid + grid_sample do and may pick the other
// neighbour where the coordinate lies within ~1e-5 of a rounding tie.
//
// Every clip carries its own draw: `sel` [B] int32 (or the per-clip record) says which clips of the batch an op applies to;
// the others are left as they are (in-place kernels return, out-of-place kernels copy).
//
// Each kernel comes in two forms picked at launch: four pixels = three aligned 32-bit words per thread where the frame has
// a multiple of four pixels and the clip is 4-byte aligned (the stencil: rows of a multiple of four pixels; posterize and
// solarize: 16 bytes per thread), else one pixel per thread with byte accesses.
//
// A library of its own, libvtx_randaug.so (include/vtx_randaug.h): libvtx_aug.so keeps its seven symbols and its version.
// Error plumbing, version and last-error exports: VTX_SIDE_LIB(randaug) (side_lib.h).
#include <math.h>
#include <string.h>
#include "side_lib.h"
#include "../../include/vtx_randaug.h"

VTX_SIDE_LIB(randaug)

namespace vtx {

// ---- pixel groups ---------------------------------------------------------------------------------------------------
// A thread owns PP consecutive pixels of a frame (linear index i .. i + PP - 1): 12 bytes as three words, or 3 bytes.
template <bool VEC>
__device__ inline void px_load(const uint8_t* p, uint32_t (&v)[VEC ? 12 : 3]) {
  if constexpr (VEC) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const uint32_t u = w[i];
      v[4 * i] = u & 255u; v[4 * i + 1] = (u >> 8) & 255u; v[4 * i + 2] = (u >> 16) & 255u; v[4 * i + 3] = u >> 24;
    }
  } else {
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
  }
}
template <bool VEC>
__device__ inline void px_store(uint8_t* p, const uint32_t (&v)[VEC ? 12 : 3]) {
  if constexpr (VEC) {
    uint32_t* w = reinterpret_cast<uint32_t*>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
  } else {
    p[0] = (uint8_t)v[0]; p[1] = (uint8_t)v[1]; p[2] = (uint8_t)v[2];
  }
}

// ---- nearest-neighbour affine warp --------------------------------------------------------------------------------
// dst(xo, yo) = src(rint sx, rint sy), 0 outside the frame, with
//   sx = M0 (xo - W/2 + .5) + M1 (yo - H/2 + .5) + M2 + W/2 - .5,   sy likewise with M3 .. M5 and H:
// torchvision's _gen_affine_grid + grid_sample(mode='nearest', padding_mode='zeros', align_corners=False) with the
// normalisation by W/2 and its inverse cancelled.  The bounds test is made on the rounded float, so a coordinate of any
// size (or a NaN in theta) reads nothing.
template <bool VEC>
__global__ __launch_bounds__(256) void clip_warp_nearest_kernel(int T, int H, int W, const uint8_t* __restrict__ src,
                                                                uint8_t* __restrict__ dst, const float* __restrict__ theta,
                                                                const int* __restrict__ sel) {
#pragma clang fp contract(off)
  constexpr int PP = VEC ? 4 : 1;
  const int frame = blockIdx.y, b = frame / T, npix = H * W;
  const bool on = sel[b] != 0;
  const float m0 = theta[b * 6], m1 = theta[b * 6 + 1], m2 = theta[b * 6 + 2];
  const float m3 = theta[b * 6 + 3], m4 = theta[b * 6 + 4], m5 = theta[b * 6 + 5];
  const float cx = (float)W * 0.5f - 0.5f, cy = (float)H * 0.5f - 0.5f;
  const float xmax = (float)(W - 1), ymax = (float)(H - 1);
  const uint8_t* in = src + (long)frame * npix * 3;
  uint8_t* out = dst + (long)frame * npix * 3;
  for (int i = (blockIdx.x * 256 + threadIdx.x) * PP; i < npix; i += gridDim.x * 256 * PP) {
    uint32_t v[PP * 3];
    if (!on) {
      px_load<VEC>(in + (long)i * 3, v);
    } else {
#pragma unroll
      for (int p = 0; p < PP; ++p) {
        const int yo = (i + p) / W, xo = (i + p) - yo * W;
        const float fx = (float)xo - cx, fy = (float)yo - cy;
        const float rx = __builtin_rintf(m0 * fx + m1 * fy + m2 + cx);        // half to even, as nearbyint
        const float ry = __builtin_rintf(m3 * fx + m4 * fy + m5 + cy);
        uint32_t c0 = 0, c1 = 0, c2 = 0;
        if (rx >= 0.0f && rx <= xmax && ry >= 0.0f && ry <= ymax) {
          const uint8_t* q = in + ((long)(int)ry * W + (int)rx) * 3;
          c0 = q[0]; c1 = q[1]; c2 = q[2];
        }
        v[3 * p] = c0; v[3 * p + 1] = c1; v[3 * p + 2] = c2;
      }
    }
    px_store<VEC>(out + (long)i * 3, v);
  }
}

// ---- sharpness ------------------------------------------------------------------------------------------------------
// degenerate = round((8 neighbours + 5 centre) / 13) inside, the frame itself on its one-pixel border; 13 is odd, so the
// quotient is never within 1/26 of a tie and (s + 6) / 13 in integers is torchvision's float32 convolution, rounded.
// result = trunc(clamp(r * img + (1 - r) * degenerate, 0, 255)), border included (r v + (1 - r) v need not give v back).
// `blend` = 0 for frames of H <= 2 or W <= 2, which adjust_sharpness returns as they are.
// Byte path: one pixel per thread, 27 single-byte neighbour loads.  Word path (W % 4 == 0, so the four pixels of a thread
// share a row): the columns x0 - 1 .. x0 + 4 of the rows y - 1, y, y + 1 are five aligned words per row, fetched once;
// the 18 column sums are formed once and each byte's stencil is three of them.  A word that lies outside the row (left
// of column 0, right of column W - 1, rows -1 and H) is not loaded, and only border pixels would have read it.
template <bool VEC>
__global__ __launch_bounds__(256) void clip_sharpness_kernel(int T, int H, int W, int blend, const uint8_t* __restrict__ src,
                                                             uint8_t* __restrict__ dst, const float* __restrict__ fac,
                                                             const int* __restrict__ sel) {
#pragma clang fp contract(off)
  constexpr int PP = VEC ? 4 : 1;
  const int frame = blockIdx.y, b = frame / T, npix = H * W;
  const bool on = blend && sel[b] != 0;
  const float r = fac[b * 2], q = fac[b * 2 + 1];
  const uint8_t* in = src + (long)frame * npix * 3;
  uint8_t* out = dst + (long)frame * npix * 3;
  for (int i = (blockIdx.x * 256 + threadIdx.x) * PP; i < npix; i += gridDim.x * 256 * PP) {
    uint32_t v[PP * 3];
    if constexpr (VEC) {
      if (on) {
        const int y = i / W, x0 = i - y * W;
        uint32_t w[3][5];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          const int yy = y + dy - 1;
          const bool row = yy >= 0 && yy < H;
          const long at = (((long)yy * W + x0) * 3) / 4;           // word of the row's byte 3 * x0: the thread's own three start here
          const uint32_t* rp = reinterpret_cast<const uint32_t*>(in);
#pragma unroll
          for (int j = 0; j < 5; ++j) {
            const bool ok = row && (j == 0 ? x0 > 0 : (j == 4 ? x0 + 4 < W : true));
            w[dy][j] = ok ? rp[at + j - 1] : 0u;
          }
        }
        // byte o of the 20 fetched per row; column q (x0 - 1 + q), channel c sits at o = 1 + 3 q + c
        auto byte = [&](int dy, int o) { return (w[dy][o >> 2] >> ((o & 3) * 8)) & 255u; };
        uint32_t col[18];
#pragma unroll
        for (int k = 0; k < 18; ++k) col[k] = byte(0, 1 + k) + byte(1, 1 + k) + byte(2, 1 + k);
        const bool yin = y > 0 && y < H - 1;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const bool inner = yin && x0 + p > 0 && x0 + p < W - 1;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int k = 3 * p + c;
            const uint32_t ctr = byte(1, 4 + k);
            const uint32_t deg = inner ? (col[k] + col[k + 3] + col[k + 6] + 4 * ctr + 6) / 13 : ctr;
            v[k] = (uint32_t)truncf(fminf(fmaxf(r * (float)ctr + q * (float)deg, 0.0f), 255.0f));
          }
        }
        px_store<VEC>(out + (long)i * 3, v);
        continue;
      }
    }
    px_load<VEC>(in + (long)i * 3, v);
    if (on) {
#pragma unroll
      for (int p = 0; p < PP; ++p) {
        const int y = (i + p) / W, x = (i + p) - y * W;
        const bool inner = y > 0 && y < H - 1 && x > 0 && x < W - 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint32_t ctr = v[3 * p + c];
          uint32_t deg = ctr;
          if (inner) {
            const uint8_t* n = in + ((long)(y - 1) * W + (x - 1)) * 3 + c;
            uint32_t s = 4 * ctr;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
              for (int dx = 0; dx < 3; ++dx) s += n[((long)dy * W + dx) * 3];
            deg = (s + 6) / 13;
          }
          const float o = truncf(fminf(fmaxf(r * (float)ctr + q * (float)deg, 0.0f), 255.0f));
          v[3 * p + c] = (uint32_t)o;
        }
      }
    }
    px_store<VEC>(out + (long)i * 3, v);
  }
}

// ---- posterize / solarize ---------------------------------------------------------------------------------------------
enum { PW_NONE = 0, PW_POSTERIZE = 1, PW_SOLARIZE = 2 };

__device__ inline uint32_t pw_word(uint32_t w, int op, uint32_t mask, uint32_t thr) {
  if (op == PW_POSTERIZE) return w & mask;
  uint32_t o = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t v = (w >> (8 * k)) & 255u;
    o |= (v >= thr ? 255u - v : v) << (8 * k);
  }
  return o;
}

// in place over the n = T*H*W*3 bytes of each clip; VEC: 16 bytes per thread (n % 16 == 0, 16-byte aligned clip)
template <bool VEC>
__global__ __launch_bounds__(256) void clip_pointwise_kernel(long n, uint8_t* __restrict__ clip, const int* __restrict__ ops) {
  const int b = blockIdx.y;
  const int op = ops[b * 2], arg = ops[b * 2 + 1];
  if (op != PW_POSTERIZE && op != PW_SOLARIZE) return;      // uniform per workgroup
  const int bits = arg < 0 ? 0 : (arg > 8 ? 8 : arg);
  const uint32_t m8 = (~((1u << (8 - bits)) - 1u)) & 255u;   // posterize: the top `bits` bits stay
  const uint32_t mask = m8 * 0x01010101u;
  const uint32_t thr = arg < 0 ? 0u : (uint32_t)arg;         // solarize: v >= thr is inverted (thr > 255: nothing is)
  uint8_t* p = clip + (long)b * n;
  if constexpr (VEC) {
    u32x4* w = reinterpret_cast<u32x4*>(p);
    const long nw = n / 16;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nw; i += (long)gridDim.x * 256) {
      u32x4 u = w[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) u[k] = pw_word(u[k], op, mask, thr);
      w[i] = u;
    }
  } else {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
      p[i] = (uint8_t)pw_word(p[i], op, mask, thr);
  }
}

// ---- autocontrast ---------------------------------------------------------------------------------------------------
// pass 1: lo[frame * 3 + c] = min, hi[frame * 3 + c] = max of channel c of the frame: per thread, then across the wave, then
// one integer atomic per wave, channel and bound.  The caller initialises lo = 0xffffffff, hi = 0.
template <bool VEC>
__global__ __launch_bounds__(256) void clip_minmax_kernel(int T, int npix, const uint8_t* __restrict__ clip,
                                                          const int* __restrict__ sel, unsigned int* __restrict__ glo,
                                                          unsigned int* __restrict__ ghi) {
  constexpr int PP = VEC ? 4 : 1;
  const int frame = blockIdx.y, b = frame / T;
  if (sel[b] == 0) return;                                  // uniform per workgroup
  const uint8_t* img = clip + (long)frame * npix * 3;
  uint32_t lo[3] = {255u, 255u, 255u}, hi[3] = {0u, 0u, 0u};
  for (int i = (blockIdx.x * 256 + threadIdx.x) * PP; i < npix; i += gridDim.x * 256 * PP) {
    uint32_t v[PP * 3];
    px_load<VEC>(img + (long)i * 3, v);
#pragma unroll
    for (int k = 0; k < PP * 3; ++k) {
      lo[k % 3] = v[k] < lo[k % 3] ? v[k] : lo[k % 3];
      hi[k % 3] = v[k] > hi[k % 3] ? v[k] : hi[k % 3];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t l = __shfl_xor(lo[c], o, 64), h = __shfl_xor(hi[c], o, 64);
      lo[c] = l < lo[c] ? l : lo[c];
      hi[c] = h > hi[c] ? h : hi[c];
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      atomicMin(glo + frame * 3 + c, lo[c]);
      atomicMax(ghi + frame * 3 + c, hi[c]);
    }
  }
}

// pass 2: v -> trunc(clamp((v - lo) * (255.0f / (hi - lo)), 0, 255)): one correctly rounded float32 division per
// channel, one product per byte; a constant channel (hi == lo, torchvision's non-finite scale) stays as it is.
template <bool VEC>
__global__ __launch_bounds__(256) void clip_autocontrast_kernel(int T, int npix, uint8_t* __restrict__ clip,
                                                                const int* __restrict__ sel,
                                                                const unsigned int* __restrict__ glo,
                                                                const unsigned int* __restrict__ ghi) {
#pragma clang fp contract(off)
  constexpr int PP = VEC ? 4 : 1;
  const int frame = blockIdx.y, b = frame / T;
  if (sel[b] == 0) return;
  float lo[3], sc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const unsigned int l = glo[frame * 3 + c], h = ghi[frame * 3 + c];
    const bool flat = h <= l;
    lo[c] = flat ? 0.0f : (float)l;
    sc[c] = flat ? 1.0f : 255.0f / ((float)h - (float)l);
  }
  uint8_t* img = clip + (long)frame * npix * 3;
  for (int i = (blockIdx.x * 256 + threadIdx.x) * PP; i < npix; i += gridDim.x * 256 * PP) {
    uint32_t v[PP * 3];
    px_load<VEC>(img + (long)i * 3, v);
#pragma unroll
    for (int k = 0; k < PP * 3; ++k)
      v[k] = (uint32_t)truncf(fminf(fmaxf(((float)v[k] - lo[k % 3]) * sc[k % 3], 0.0f), 255.0f));
    px_store<VEC>(img + (long)i * 3, v);
  }
}

// ---- equalize -------------------------------------------------------------------------------------------------------
// pass 1: hist[(frame * 3 + c) * 256 + v] += count.  3 x 256 bins per workgroup in LDS, filled with LDS atomics and
// flushed with one global atomic per non-zero bin.  In LDS the bins are interleaved (v * 3 + c): the three channels of
// a pixel, usually of similar value, then fall into neighbouring banks instead of the same one.
template <bool VEC>
__global__ __launch_bounds__(256) void clip_hist_kernel(int T, int npix, const uint8_t* __restrict__ clip,
                                                        const int* __restrict__ sel, unsigned int* __restrict__ hist) {
  constexpr int PP = VEC ? 4 : 1;
  __shared__ unsigned int h[768];
  const int frame = blockIdx.y, b = frame / T;
  if (sel[b] == 0) return;                                  // uniform per workgroup
  for (int t = threadIdx.x; t < 768; t += 256) h[t] = 0;
  __syncthreads();
  const uint8_t* img = clip + (long)frame * npix * 3;
  for (int i = (blockIdx.x * 256 + threadIdx.x) * PP; i < npix; i += gridDim.x * 256 * PP) {
    uint32_t v[PP * 3];
    px_load<VEC>(img + (long)i * 3, v);
#pragma unroll
    for (int k = 0; k < PP * 3; ++k) atomicAdd(&h[v[k] * 3 + k % 3], 1u);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 768; t += 256) {
    const unsigned int n = h[t];
    if (n) atomicAdd(hist + (long)frame * 768 + (t % 3) * 256 + t / 3, n);
  }
}

// pass 2: every workgroup rebuilds the three look-up tables of its frame in LDS (thread t owns bin t), then applies them.
//   cum = inclusive prefix sum of the histogram (cum[255] = npix);
//   step = (npix - count of the last non-zero bin) / 255;  step == 0: the channel stays as it is;
//   lut[0] = 0, lut[t] = min((cum[t - 1] + step / 2) / step, 255).
template <bool VEC>
__global__ __launch_bounds__(256) void clip_equalize_kernel(int T, int npix, uint8_t* __restrict__ clip,
                                                            const int* __restrict__ sel, const unsigned int* __restrict__ hist) {
  constexpr int PP = VEC ? 4 : 1;
  __shared__ unsigned int cum[3][256];
  __shared__ unsigned int last[3];
  __shared__ uint8_t lut[3][256];
  const int frame = blockIdx.y, b = frame / T, t = threadIdx.x;
  if (sel[b] == 0) return;                                  // uniform per workgroup
  unsigned int mine[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    mine[c] = hist[(long)frame * 768 + c * 256 + t];
    cum[c][t] = mine[c];
  }
  if (t < 3) last[t] = 0;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    unsigned int add[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) add[c] = t >= off ? cum[c][t - off] : 0u;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) cum[c][t] += add[c];
    __syncthreads();
  }
  // the last non-zero bin is the first whose prefix sum reaches the pixel count: exactly one thread per channel
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (cum[c][t] == (unsigned int)npix && (t == 0 || cum[c][t - 1] < (unsigned int)npix)) last[c] = mine[c];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const unsigned int step = ((unsigned int)npix - last[c]) / 255u;
    unsigned int o = (unsigned int)t;
    if (step != 0) {
      o = t == 0 ? 0u : (cum[c][t - 1] + step / 2u) / step;
      o = o > 255u ? 255u : o;
    }
    lut[c][t] = (uint8_t)o;
  }
  __syncthreads();
  uint8_t* img = clip + (long)frame * npix * 3;
  for (int i = (blockIdx.x * 256 + t) * PP; i < npix; i += gridDim.x * 256 * PP) {
    uint32_t v[PP * 3];
    px_load<VEC>(img + (long)i * 3, v);
#pragma unroll
    for (int k = 0; k < PP * 3; ++k) v[k] = lut[k % 3][v[k]];
    px_store<VEC>(img + (long)i * 3, v);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
static bool word_path(const void* a, const void* b, long npix) {
  return npix % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3u) == 0;
}
// workgroups per frame: every pixel group once, at most `cap` (the kernels stride)
static unsigned groups(long npix, bool vec, long cap) {
  const long per = vec ? 1024 : 256;
  long g = (npix + per - 1) / per;
  return (unsigned)(g > cap ? cap : g);
}

}  // namespace vtx

using namespace vtx;

#define RA_SHAPE(name)                                                                                                        \
  VTX_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0, VTX_EINVAL, name ": B=%d T=%d H=%d W=%d must all be positive", B, T, H, W);   \
  VTX_REQUIRE((long)H * W <= (1L << 28), VTX_EINVAL, name ": %dx%d frames exceed 2^28 pixels", H, W);                         \
  VTX_REQUIRE((long)B * T <= 65535, VTX_EINVAL, name ": %ld frames exceed the grid (65535)", (long)B * T)

extern "C" int vtx_clip_warp_nearest_u8(int B, int T, int H, int W, const unsigned char* src, unsigned char* dst, const float* theta,
                                        const int32_t* sel, void* stream) {
  RA_SHAPE("clip_warp_nearest_u8");
  VTX_REQUIRE(src && dst && theta && sel, VTX_EINVAL, "clip_warp_nearest_u8: null pointer");
  VTX_REQUIRE(src != dst, VTX_EINVAL, "clip_warp_nearest_u8: in place is not supported");
  const long npix = (long)H * W;
  const bool vec = word_path(src, dst, npix);
  dim3 grid(groups(npix, vec, 1L << 20), (unsigned)(B * T));
  if (vec)
    hipLaunchKernelGGL(clip_warp_nearest_kernel<true>, grid, dim3(256), 0, as_stream(stream), T, H, W, src, dst, theta, sel);
  else
    hipLaunchKernelGGL(clip_warp_nearest_kernel<false>, grid, dim3(256), 0, as_stream(stream), T, H, W, src, dst, theta, sel);
  return check_launch("clip_warp_nearest_u8");
}

extern "C" int vtx_clip_sharpness_u8(int B, int T, int H, int W, const unsigned char* src, unsigned char* dst, const float* factors,
                                     const int32_t* sel, void* stream) {
  RA_SHAPE("clip_sharpness_u8");
  VTX_REQUIRE(src && dst && factors && sel, VTX_EINVAL, "clip_sharpness_u8: null pointer");
  VTX_REQUIRE(src != dst, VTX_EINVAL, "clip_sharpness_u8: in place is not supported");
  const long npix = (long)H * W;
  const bool vec = W % 4 == 0 && word_path(src, dst, npix);
  const int blend = H > 2 && W > 2;
  dim3 grid(groups(npix, vec, 1L << 20), (unsigned)(B * T));
  if (vec)
    hipLaunchKernelGGL(clip_sharpness_kernel<true>, grid, dim3(256), 0, as_stream(stream), T, H, W, blend, src, dst, factors, sel);
  else
    hipLaunchKernelGGL(clip_sharpness_kernel<false>, grid, dim3(256), 0, as_stream(stream), T, H, W, blend, src, dst, factors, sel);
  return check_launch("clip_sharpness_u8");
}

extern "C" int vtx_clip_pointwise_u8(int B, int T, int H, int W, unsigned char* clip, const int32_t* ops, void* stream) {
  RA_SHAPE("clip_pointwise_u8");
  VTX_REQUIRE(clip && ops, VTX_EINVAL, "clip_pointwise_u8: null pointer");
  const long n = (long)T * H * W * 3;
  const bool vec = n % 16 == 0 && aligned16(clip);
  long g = ((vec ? n / 16 : n) + 255) / 256;
  if (g > 1024) g = 1024;
  dim3 grid((unsigned)g, (unsigned)B);
  if (vec)
    hipLaunchKernelGGL(clip_pointwise_kernel<true>, grid, dim3(256), 0, as_stream(stream), n, clip, ops);
  else
    hipLaunchKernelGGL(clip_pointwise_kernel<false>, grid, dim3(256), 0, as_stream(stream), n, clip, ops);
  return check_launch("clip_pointwise_u8");
}

extern "C" size_t vtx_clip_autocontrast_workspace(int B, int T) { return B > 0 && T > 0 ? (size_t)B * T * 6 * sizeof(unsigned int) : 0; }

extern "C" int vtx_clip_autocontrast_u8(int B, int T, int H, int W, unsigned char* clip, const int32_t* sel, void* workspace,
                                        size_t ws_bytes, void* stream) {
  RA_SHAPE("clip_autocontrast_u8");
  VTX_REQUIRE(clip && sel && workspace, VTX_EINVAL, "clip_autocontrast_u8: null pointer");
  VTX_REQUIRE(ws_bytes >= vtx_clip_autocontrast_workspace(B, T), VTX_EINVAL, "clip_autocontrast_u8: workspace of %zu bytes, vtx_clip_autocontrast_workspace() = %zu",
              ws_bytes, vtx_clip_autocontrast_workspace(B, T));
  VTX_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, VTX_EALIGN, "clip_autocontrast_u8: workspace must be 4-byte aligned");
  const int npix = H * W;
  const bool vec = word_path(clip, clip, npix);
  hipStream_t st = as_stream(stream);
  // minima [B*T*3] start at 0xffffffff, the maxima behind them at 0
  const size_t half = (size_t)B * T * 3 * sizeof(unsigned int);
  unsigned int* lo = reinterpret_cast<unsigned int*>(workspace);
  unsigned int* hi = lo + (size_t)B * T * 3;
  if (hipMemsetAsync(lo, 0xff, half, st) != hipSuccess || hipMemsetAsync(hi, 0, half, st) != hipSuccess) {
    set_error("clip_autocontrast_u8: workspace initialisation failed");
    return VTX_ELAUNCH;
  }
  // pass 1 with few workgroups per frame: its cost is the atomics (six per wave on six words per frame), not the bytes
  dim3 grid1(groups(npix, vec, 8), (unsigned)(B * T)), grid(groups(npix, vec, 64), (unsigned)(B * T));
  if (vec) {
    hipLaunchKernelGGL(clip_minmax_kernel<true>, grid1, dim3(256), 0, st, T, npix, clip, sel, lo, hi);
    hipLaunchKernelGGL(clip_autocontrast_kernel<true>, grid, dim3(256), 0, st, T, npix, clip, sel, lo, hi);
  } else {
    hipLaunchKernelGGL(clip_minmax_kernel<false>, grid1, dim3(256), 0, st, T, npix, clip, sel, lo, hi);
    hipLaunchKernelGGL(clip_autocontrast_kernel<false>, grid, dim3(256), 0, st, T, npix, clip, sel, lo, hi);
  }
  return check_launch("clip_autocontrast_u8");
}

extern "C" size_t vtx_clip_equalize_workspace(int B, int T) { return B > 0 && T > 0 ? (size_t)B * T * 768 * sizeof(unsigned int) : 0; }

extern "C" int vtx_clip_equalize_u8(int B, int T, int H, int W, unsigned char* clip, const int32_t* sel, void* workspace,
                                    size_t ws_bytes, void* stream) {
  RA_SHAPE("clip_equalize_u8");
  VTX_REQUIRE(clip && sel && workspace, VTX_EINVAL, "clip_equalize_u8: null pointer");
  VTX_REQUIRE(ws_bytes >= vtx_clip_equalize_workspace(B, T), VTX_EINVAL, "clip_equalize_u8: workspace of %zu bytes, vtx_clip_equalize_workspace() = %zu",
              ws_bytes, vtx_clip_equalize_workspace(B, T));
  VTX_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, VTX_EALIGN, "clip_equalize_u8: workspace must be 4-byte aligned");
  const int npix = H * W;
  const bool vec = word_path(clip, clip, npix);
  hipStream_t st = as_stream(stream);
  unsigned int* hist = reinterpret_cast<unsigned int*>(workspace);
  if (hipMemsetAsync(hist, 0, (size_t)B * T * 768 * sizeof(unsigned int), st) != hipSuccess) {
    set_error("clip_equalize_u8: hipMemsetAsync failed");
    return VTX_ELAUNCH;
  }
  // few workgroups per frame: each flushes up to 768 bins (pass 1) and rebuilds the tables (pass 2)
  dim3 grid(groups(npix, vec, 8), (unsigned)(B * T));
  if (vec) {
    hipLaunchKernelGGL(clip_hist_kernel<true>, grid, dim3(256), 0, st, T, npix, clip, sel, hist);
    hipLaunchKernelGGL(clip_equalize_kernel<true>, grid, dim3(256), 0, st, T, npix, clip, sel, hist);
  } else {
    hipLaunchKernelGGL(clip_hist_kernel<false>, grid, dim3(256), 0, st, T, npix, clip, sel, hist);
    hipLaunchKernelGGL(clip_equalize_kernel<false>, grid, dim3(256), 0, st, T, npix, clip, sel, hist);
  }
  return check_launch("clip_equalize_u8");
}
