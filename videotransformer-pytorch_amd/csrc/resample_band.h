// resample_band.h -- the separable resampling band of clip_resample_u8_kernel (aug.hip), clip_views_u8_kernel (views.hip),
// clips_views_u8_kernel (ragged.hip) and clips_views_yuv420_kernel (yuv.hip), written once: the entry points give the same
// bytes for the same tables and the same RGB values because they run this text.  What differs is the tap reader: an RGB
// frame (RgbTaps, here) or 4:2:0 planes converted tap by tap in registers (yuv.hip).
//
// One thread per output column x (all three channels), one workgroup per (frame, band of BAND_ROWS output rows, 256
// columns).  The band's source rows s = lo .. hi-1 are walked once in ascending order: the thread forms the x-resampled
// value of (s, x) for its three channels in registers -- the x pass -- and adds it, times the y weight, to every output
// row of the band whose tap window holds s -- the y pass, taps in ascending order as torch sums them.  No intermediate
// leaves the registers, so nothing limits the tap counts (antialiased 1080p -> 224 has 20 and more) and source rows need
// no alignment: a tap is three single-byte loads, adjacent lanes read adjacent or overlapping bytes of the same lines.
// Tables per clip: first[n], count[n], w[n][taps] (only w[.][0 .. count-1] is read; the tail is unspecified).
//
// Arithmetic contract (torchvision's tensor path, restated in tests/aug_ref.py): x pass first, then the y pass, both in
// float32 without fma contraction; the result is clamped to [0, 255] and rounded half-to-even (_cast_squeeze_out).
#pragma once
#include "common.h"

namespace vtx {

constexpr int BAND_ROWS = 8;     // output rows per band: 3 * 8 accumulators per thread; the x pass of a source row is
                                 // repeated by every band that needs it ((8 * scale + taps) / (8 * scale) times)
constexpr int MAX_VIEWS = 8;     // views of one launch of views.hip / ragged.hip, each a window of columns (vtx/_lib.py: VIEWS_MAX)

// a tap window [f, f + c) as the table gives it -> inside the source axis [0, len), at most `taps` weights, whatever it says
__device__ inline void clamp_taps(int& f, int& c, int taps, int len) {
  c = c < 0 ? 0 : (c > taps ? taps : c);
  f = f < 0 ? 0 : (f > len ? len : f);
  if (f + c > len) { f = len - c < 0 ? 0 : len - c; c = c > len ? len : c; }
}

// The tap reader of an RGB frame [Hs,Ws,3], the default: a tap is three single-byte loads.  A reader names its Source (what
// the band is given for a frame, passed by value) and has a static row(source, Ws, s, fx) that gives, for source row s and
// first tap column fx, a row object whose tap(k) yields the three channels of column fx + k as floats.  The band calls row()
// once per source row and tap() for k = 0 .. cx-1 in ascending order, all inside the frame.  (Static, and no reader object:
// with one the compiler orders two scalar selects of the y windows differently in the three RGB kernels.)
struct RgbTaps {
  typedef const uint8_t* __restrict__ Source;                      // the frame
  struct Row {
    const uint8_t* __restrict__ p;
    __device__ __forceinline__ float3 tap(int k) const { return make_float3((float)p[3 * k], (float)p[3 * k + 1], (float)p[3 * k + 2]); }
  };
  static __device__ __forceinline__ Row row(Source img, int Ws, int s, int fx) { return Row{img + ((long)s * Ws + fx) * 3}; }
};

// Output rows r0 .. r0 + BAND_ROWS - 1 (those below H) of one column of one frame of Hs x Ws pixels.  src: what Taps reads --
// RgbTaps (the default): the frame [Hs,Ws,3]; yuv.hip's reader: 4:2:0 planes; fx, cx: the column's raw table entries, wx its
// weight row of xt floats; yf, yc, yw: the clip's y table rows of H entries (yw: H * yt).  store(r, red, green, blue) is called
// once per live output row r0 + r with the rounded bytes.
template <typename Taps = RgbTaps, typename Store>
__device__ __forceinline__ void resample_band(typename Taps::Source src, int Hs, int Ws, int H, int r0, int fx, int cx,
                                              const float* __restrict__ wx, int xt, const int* __restrict__ yf,
                                              const int* __restrict__ yc, const float* __restrict__ yw, int yt, Store store) {
#pragma clang fp contract(off)
  clamp_taps(fx, cx, xt, Ws);
  // the band's y windows (the same for every thread: scalar registers)
  int fy[BAND_ROWS], cy[BAND_ROWS];
  int lo = Hs, hi = 0;
#pragma unroll
  for (int r = 0; r < BAND_ROWS; ++r) {
    const int ri = r0 + r < H ? r0 + r : H - 1;
    int f = yf[ri], c = yc[ri];
    clamp_taps(f, c, yt, Hs);
    if (r0 + r >= H) c = 0;
    fy[r] = f; cy[r] = c;
    if (c > 0) { lo = f < lo ? f : lo; hi = f + c > hi ? f + c : hi; }
  }
  float acc[BAND_ROWS][3];
#pragma unroll
  for (int r = 0; r < BAND_ROWS; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.0f;
  for (int s = lo; s < hi; ++s) {
    const auto row = Taps::row(src, Ws, s, fx);
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    for (int k = 0; k < cx; ++k) {
      const float w = wx[k];
      const float3 t = row.tap(k);
      v0 = v0 + w * t.x;
      v1 = v1 + w * t.y;
      v2 = v2 + w * t.z;
    }
#pragma unroll
    for (int r = 0; r < BAND_ROWS; ++r) {
      const int k = s - fy[r];
      if (k >= 0 && k < cy[r]) {
        const float w = yw[(long)(r0 + r) * yt + k];
        acc[r][0] = acc[r][0] + w * v0;
        acc[r][1] = acc[r][1] + w * v1;
        acc[r][2] = acc[r][2] + w * v2;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < BAND_ROWS; ++r) {
    if (r0 + r >= H) break;
    uint8_t q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      q[c] = (uint8_t)(int)__builtin_rintf(fminf(fmaxf(acc[r][c], 0.0f), 255.0f));      // half-to-even, as torch.round
    store(r, q[0], q[1], q[2]);
  }
}

}  // namespace vtx
