// hog_kernel.h -- the device code of the HOG extractor (contract and kernel design: the head of hog.hip) and its launch,
// written once for the two libraries that run it: libvtx.so (hog.hip: vtx_hog_fwd, a dense stack of frames) and
// libvtx_stem.so (stem.hip: vtx_hog_fwd_sel, selected frames of a clip batch).  Both translation units are compiled with
// -ffp-contract=off (csrc/build.py).
#pragma once
#include "common.h"

namespace vtx {

constexpr int HOG_EXC_WORDS = 4096;          // 65 536 gradient pairs x 2 bits: 0 = hypot is the rounded sqrt, 1 = one ulp above, 3 = one below

// integer rule: with (g, c) = (g_row, g_col) flipped into the upper half plane, the orientation is at least 20 j degrees
// iff |c| <= floor(g cot(20 j)) on the c >= 0 side (bins 0..4), and the mirror image on the c < 0 side (bins 4..8).
// floor(g cot) = (g * round(cot * 2^16)) >> 16 for every g in 0..255 (checked offline and by vtx_selftest).
__device__ inline int hog_bin(int gr, int gc) {
  const bool flip = gr < 0 || (gr == 0 && gc < 0);
  const int g = flip ? -gr : gr, c = flip ? -gc : gc;
  const int a = c < 0 ? -c : c;
  // (g <= 255 and the constants are below 2^18: the 24-bit multiply is exact and full rate, v_mul_lo_u32 is quarter rate)
  const int cnt = (a <= (__mul24(g, 180059) >> 16) ? 1 : 0) + (a <= (__mul24(g, 78103) >> 16) ? 1 : 0) +
                  (a <= (__mul24(g, 37837) >> 16) ? 1 : 0) + (a <= (__mul24(g, 11556) >> 16) ? 1 : 0);
  const int b = c >= 0 ? cnt : 8 - cnt;
  return (gr | gc) == 0 ? 0 : b;
}

// host hypot(ac, ar) for 0 <= ar, ac <= 255: correctly rounded sqrt of the exact integer n = ar^2 + ac^2 <= 130 050, moved by
// the table's correction (`word` = exc[(ar * 256 + ac) >> 4]).  The square root: n is exact in float32, s = v_sqrt_f32(n) is
// good to ~2^-23, h = 0.5 / s from v_rcp_f32; two Newton corrections in float64 -- r = fma(-m, m, n) is the exact residual of
// the 24-bit s in the first, m += r * h -- leave an error of ~2^-69 m, far below the half-ulp of the result (the generic
// float64 lowering costs twice the float64 instructions: range scaling, v_rsq_f64, three iterations).  "Far below" is not a
// proof of correct rounding: vtx_selftest compares ALL 65 536 magnitudes with the host table on the device at hand.
__device__ inline double hog_mag(int ar, int ac, unsigned word) {
  const int idx = ar * 256 + ac;
  const int n = __mul24(ar, ar) + __mul24(ac, ac);
#if defined(HOG_ABLATE) && HOG_ABLATE == 1           // diagnostic builds (csrc/build.py --variant): no square root
  double m = (double)n;
#elif defined(HOG_ABLATE) && HOG_ABLATE == 6         // the compiler's float64 square root
  double m = sqrt((double)n);
#else
  const float nf = (float)n;
  const float s = __builtin_amdgcn_sqrtf(nf);
  const double x = (double)nf;
  double m = (double)s;
  const double h = (double)(0.5f * __builtin_amdgcn_rcpf(s));
  m = fma(fma(-m, m, x), h, m);
  m = fma(fma(-m, m, x), h, m);
  m = n == 0 ? 0.0 : m;                              // rcp(0) = inf
#endif
#if defined(HOG_ABLATE) && HOG_ABLATE == 2           // no correction
  return m + (double)(word & 0u);
#else
  const int delta = ((int)(word << (30 - 2 * (idx & 15)))) >> 30;          // 2-bit field, sign-extended: 0, +1, -1
  // one ulp up or down = the low word +- 1: no square root of these integers has a low word of all zeros or all ones next to a
  // correction (vtx_selftest would show it), so the carry into the high word is never needed
  const long long b = __double_as_longlong(m);
  return __longlong_as_double((b & ~0xffffffffLL) | (unsigned)((int)b + delta));
#endif
}

// frames [F,H,W,3] u8; grid = persistent workgroups over the F * (H/8) strips; block = 256 * CP threads.
// CP = channels in parallel: 3 (W <= 256: threads 256 c .. 256 c + 255 work on channel c, every phase once per strip, 12 waves per
// workgroup and two workgroups per CU) or 1 (wider frames: the three channels one after the other through one magnitude tile).
// sel (vtx_hog_fwd_sel; nullptr: every frame, vtx_hog_fwd): work frame fi of the F is frame sel[fi] of the `frames_all` the
// buffers hold -- read there and written to THAT row of out; an index outside 0 .. frames_all-1 is skipped by the whole workgroup.
template <int CP>
__global__ __launch_bounds__(256 * CP, CP == 3 ? 6 : 1) void hog_kernel(const uint8_t* __restrict__ frames, int F, int H, int W,
                                                       const uint32_t* __restrict__ exc, double* __restrict__ out,
                                                       int32_t* __restrict__ bins, const int32_t* __restrict__ sel, int frames_all) {
  extern __shared__ __attribute__((aligned(16))) char hsm[];
  constexpr int T = 256 * CP;
  const int nc = W / 8, W3 = 3 * W;
  uint32_t* excs = reinterpret_cast<uint32_t*>(hsm);                                    // [4096]
  uint8_t* px = reinterpret_cast<uint8_t*>(hsm + HOG_EXC_WORDS * 4);                    // [10][3 W]  (30 W bytes, W % 16 == 0)
  double* mag_all = reinterpret_cast<double*>(px + 10 * W3);                            // [CP][nc][8 rows][8 columns]
  uint32_t* msk_all = reinterpret_cast<uint32_t*>(mag_all + CP * 8 * W);                // [CP][nc][9][2]
  double* hist = reinterpret_cast<double*>(msk_all + CP * nc * 18);                     // [nc][27]
  const int tid_all = threadIdx.x;
  const int grp = CP == 1 ? 0 : tid_all >> 8, tid = CP == 1 ? tid_all : tid_all & 255;   // channel group of this thread
  double* mag = mag_all + grp * 8 * W;
  uint32_t* msk = msk_all + grp * nc * 18;
  for (int i = tid_all; i < HOG_EXC_WORDS; i += T) excs[i] = exc[i];
  const int strips = H / 8;
  const long items = (long)F * strips;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const int fi = (int)(item / strips), cr = (int)(item - (long)fi * strips);
    const int f = sel ? sel[fi] : fi;
    if ((unsigned)f >= (unsigned)frames_all) continue;          // (the same for every thread of the workgroup: no barrier is split)
    const int y0 = cr * 8;
    const uint8_t* img = frames + (long)f * H * W3;
    __syncthreads();                                 // the previous strip's feature stores have read hist; excs is in place
    // rows y0-1 .. y0+8: one contiguous block of the frame, 16 bytes per load; rows outside the frame read as 0
    {
      const long first = (long)(y0 - 1) * W3, last = (long)H * W3;
      for (int v = tid_all; v < (10 * W3) / 16; v += T) {
        const long g0 = first + (long)v * 16;
        uint4 val = make_uint4(0, 0, 0, 0);
        if (g0 >= 0 && g0 < last) val = *reinterpret_cast<const uint4*>(img + g0);
        *reinterpret_cast<uint4*>(px + v * 16) = val;
      }
    }
#pragma unroll 1
    for (int chi = 0; chi < 3 / CP; ++chi) {
      const int ch = CP == 1 ? chi : grp;
      for (int i = tid; i < nc * 18; i += 256) msk[i] = 0u;
      __syncthreads();                               // pixels in place / masks cleared; phase B of the previous channel is done
      // (A) one pixel column per thread, eight rows
      for (int x = tid; x < W; x += 256) {
        const bool xin = x > 0 && x < W - 1;
        const int xo = 3 * x + ch;
#pragma unroll
        for (int ry = 0; ry < 8; ++ry) {
          const int y = y0 + ry;
          int gr = 0, gc = 0;
          if (y > 0 && y < H - 1) gr = (int)px[(ry + 2) * W3 + xo] - (int)px[ry * W3 + xo];
          if (xin) gc = (int)px[(ry + 1) * W3 + xo + 3] - (int)px[(ry + 1) * W3 + xo - 3];
#if defined(HOG_ABLATE) && HOG_ABLATE == 4           // no bin rule
          const int b = (gr + gc) & 7;
#else
          const int b = hog_bin(gr, gc);
#endif
          const int ar = gr < 0 ? -gr : gr, ac = gc < 0 ? -gc : gc;
#if defined(HOG_ABLATE) && HOG_ABLATE == 5           // no magnitude at all
          const double m = (double)(ar + ac);
#else
          const double m = hog_mag(ar, ac, excs[(ar * 256 + ac) >> 4]);
#endif
          mag[(x >> 3) * 64 + ry * 8 + (x & 7)] = m;      // cell-major: phase B addresses a pixel by its bit position alone
          if ((gr | gc) != 0) atomicOr(&msk[((x >> 3) * 9 + b) * 2 + (ry >> 2)], 1u << ((ry & 3) * 8 + (x & 7)));
          if (bins) bins[(((long)f * 3 + ch) * H + y) * W + x] = b;
        }
      }
      __syncthreads();
      // (B) one (cell, bin) per thread: the set bits of its mask in ascending order = the cell's pixels of that bin, row-major
#if defined(HOG_ABLATE) && HOG_ABLATE == 3           // no phase B
      for (int i = tid; i < nc * 9; i += 256) hist[(i / 9) * 27 + ch * 9 + i % 9] = mag[i];     // (diagnostic)
      if (false)
#endif
      for (int i = tid; i < nc * 9; i += 256) {
        const int cc = i / 9, ob = i - cc * 9;
        uint32_t m0 = msk[i * 2], m1 = msk[i * 2 + 1];
        const double* mg = mag + cc * 64;
        float tot = 0.0f;
        // four set bits per trip: the four magnitudes are requested together, the adds stay sequential and in ascending bit
        // order (= row-major in the cell); a bit position beyond the mask's population reads pixel 0 and is not added
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          uint32_t m = half ? m1 : m0;
          const double* mh = mg + half * 32;
          while (m) {
            int p[4];
            bool v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              v[k] = m != 0;
              p[k] = v[k] ? __builtin_ctz(m) : 0;
              m &= m - 1;
            }
            double a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = mh[p[k]];
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (v[k]) tot = (float)((double)tot + a[k]);
          }
        }
        hist[cc * 27 + ch * 9 + ob] = (double)(tot / 64.0f);
      }
      __syncthreads();
    }
    // (C) L2 norm per (cell, channel), in place
    for (int i = tid_all; i < nc * 3; i += T) {
      double* h = hist + (i / 3) * 27 + (i % 3) * 9;
      double s = ((h[0] * h[0] + h[1] * h[1]) + (h[2] * h[2] + h[3] * h[3])) +
                 ((h[4] * h[4] + h[5] * h[5]) + (h[6] * h[6] + h[7] * h[7]));
      s += h[8] * h[8];
      const double nrm = sqrt(s + 1e-5 * 1e-5);
#pragma unroll
      for (int k = 0; k < 9; ++k) h[k] = h[k] / nrm;
    }
    __syncthreads();
    // features: cells 2 pw and 2 pw + 1 of this strip are 54 contiguous doubles of out (dw = 0, 1 at dh = cr & 1)
    {
      const int ph = cr >> 1, dh = cr & 1;
      double* orow = out + (((long)f * (H / 16) + ph) * (W / 16)) * 108 + dh * 54;
      for (int i = tid_all; i < (nc / 2) * 27; i += T) {
        const int pw = i / 27, j = i - pw * 27;
        *reinterpret_cast<double2*>(orow + (long)pw * 108 + 2 * j) = *reinterpret_cast<const double2*>(hist + pw * 54 + 2 * j);
      }
    }
  }
}

// The launch vtx_hog_fwd (hog.hip) and vtx_hog_fwd_sel (stem.hip) share: F work frames (sel == nullptr: the frames 0 .. F-1
// themselves; else frames sel[0 .. F-1] of the frames_all the buffers hold).  The callers check the arguments; `who` names the
// caller in the error string.
static inline int hog_launch(const char* who, const uint8_t* frames, int F, int H, int W, const double* table, double* out,
                             int32_t* bins, const int32_t* sel, int frames_all, void* stream) {
  const uint32_t* exc = reinterpret_cast<const uint32_t*>(table + 256 * 256);   // the correction words behind the 65 536 doubles
  // W <= 256: the three channels side by side (768 threads); wider frames: one channel at a time (256 threads, one magnitude tile)
  const int cp = W <= 256 ? 3 : 1;
  const size_t lds = (size_t)HOG_EXC_WORDS * 4 + (size_t)30 * W + (size_t)cp * 8 * W * 8 + (size_t)cp * (W / 8) * 18 * 4 + (size_t)(W / 8) * 27 * 8;
  // persistent: as many workgroups as fit at once (LDS- and wave-limited), each walks strips with stride gridDim
  const long items = (long)F * (H / 8);
  long per_cu = (long)(160 * 1024) / (long)lds; if (per_cu < 1) per_cu = 1;
  const long wave_cap = 32 / (4 * cp); if (per_cu > wave_cap) per_cu = wave_cap;
  long grid = per_cu * device_cus(); if (grid > items) grid = items;
  if (cp == 3) {
    allow_lds<hog_kernel<3>>(lds);
    hipLaunchKernelGGL(hog_kernel<3>, dim3((unsigned)grid), dim3(768), lds, as_stream(stream), frames, F, H, W, exc, out, bins, sel, frames_all);
  } else {
    allow_lds<hog_kernel<1>>(lds);
    hipLaunchKernelGGL(hog_kernel<1>, dim3((unsigned)grid), dim3(256), lds, as_stream(stream), frames, F, H, W, exc, out, bins, sel, frames_all);
  }
  return check_launch(who);
}

}  // namespace vtx
