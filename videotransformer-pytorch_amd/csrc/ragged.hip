// ragged.hip -- the views of views.hip for a batch whose clips differ in decoded length and frame size, in one launch.
//
// The reference transforms every video on its own (dataset.py:152-205) and collates only the results, so its loader never
// needs clips of one size; Kinetics videos come as 340x256, 256x340, 320x240, 480x360, ... and decoded spans differ in
// length.  vtx_clip_views_u8 takes one tensor [B,Ts,Hs,Ws,3]; here clip b is its own allocation, named by a device table
// of base pointers, with its Ts_b, Hs_b, Ws_b and the width Wr_b of its resized row in a device record.  The OUTPUT is
// uniform, [B,V,T,H,W,3], and so is everything behind it (jitter, RandAugment, Mixup, the patch gathers, hog_targets).
//
//   dst[b, v, t] = columns left[b,v] .. left[b,v] + W of the resized frame  Wy[b] * src[b][frames[b,t]] * Wx[b]^T
//
// The kernel is clip_views_u8_kernel (csrc/views.hip) with the clip's base pointer and Ts / Hs / Ws / Wr read per
// workgroup: b = blockIdx.z / T is the same for every thread, so these are scalar registers.  The x tables have one row
// stride, Wr_max, for all clips; row b is valid for x < Wr_b.  The grid covers Wr_max columns: a column tile beyond a
// clip's Wr_b, or in none of its windows, returns before any load.
//
// Arithmetic contract: that kernel's, because both run resample_band (resample_band.h) behind the same window test -- x pass
// first, then the y pass, taps in ascending order, float32 without fma contraction, clamp to [0, 255], round half-to-even --
// so clip b's views are byte for byte what vtx_clip_views_u8 gives on clip b alone with its rows of the tables.
//
// A library of its own, libvtx_ragged.so (include/vtx_ragged.h): the other six keep their symbols and versions.
// Error plumbing, version and last-error exports: VTX_SIDE_LIB(ragged) (side_lib.h).
#include "side_lib.h"
#include "resample_band.h"
#include "../../include/vtx_ragged.h"

VTX_SIDE_LIB(ragged)

namespace vtx {

// One workgroup per (clip and selected frame, band of BAND_ROWS output rows, 256 columns of the widest resized row), as in
// views.hip.  The two kernels share resample_band; the view-window test in front of it and the store to every view behind
// it are written in each of them (a shared body for those was measured: it cost the views kernel 5 % on one-view batches,
// profiles/resample_band_refactor_bench.txt).  Everything is clamped with the clip's own Ts / Hs / Ws / Wr whatever the
// arrays say; the caller validates them, and the pointers.
__global__ __launch_bounds__(256) void clips_views_u8_kernel(int T, int H, int V, int W, int Wr_max,
                                                             const uint8_t* const* __restrict__ src, const int* __restrict__ geom,
                                                             uint8_t* __restrict__ dst,
                                                             const int* __restrict__ frames, const int* __restrict__ left,
                                                             const int* __restrict__ xf, const int* __restrict__ xc,
                                                             const float* __restrict__ xw, int xt,
                                                             const int* __restrict__ yf, const int* __restrict__ yc,
                                                             const float* __restrict__ yw, int yt) {
  const int b = blockIdx.z / T, t = blockIdx.z - b * T;
  // the clip's descriptor: the same for the whole workgroup
  const int Ts = geom[4 * b], Hs = geom[4 * b + 1], Ws = geom[4 * b + 2];
  int Wr = geom[4 * b + 3];
  Wr = Wr > Wr_max ? Wr_max : Wr;                        // the table rows hold Wr_max entries
  if (Ts < 1 || Hs < 1 || Ws < 1 || Wr < W) return;      // (the host refuses such a record)
  const int r0 = blockIdx.y * BAND_ROWS;
  const int x = blockIdx.x * 256 + threadIdx.x;
  // the views whose window holds this column (the lefts are the same for every thread: scalar registers)
  int off[MAX_VIEWS];
  bool any = false;
#pragma unroll
  for (int v = 0; v < MAX_VIEWS; ++v) {
    off[v] = -1;
    if (v < V) {
      int l = left[b * V + v];
      l = l < 0 ? 0 : (l > Wr - W ? Wr - W : l);
      if (x >= l && x < l + W) { off[v] = x - l; any = true; }
    }
  }
  if (!any) return;                                      // also every x >= Wr: l + W <= Wr <= Wr_max
  int ts = frames ? frames[b * T + t] : t;
  ts = ts < 0 ? 0 : (ts > Ts - 1 ? Ts - 1 : ts);
  const long col = (long)b * Wr_max + x;
  resample_band(src[b] + (long)ts * Hs * Ws * 3, Hs, Ws, H, r0, xf[col], xc[col], xw + col * xt, xt,
                yf + (long)b * H, yc + (long)b * H, yw + (long)b * H * yt, yt, [=](int r, uint8_t q0, uint8_t q1, uint8_t q2) {
#pragma unroll
                  for (int v = 0; v < MAX_VIEWS; ++v) {
                    if (off[v] < 0) continue;
                    uint8_t* o = dst + (((((long)b * V + v) * T + t) * H + r0 + r) * W + off[v]) * 3;
                    o[0] = q0; o[1] = q1; o[2] = q2;
                  }
                });
}

}  // namespace vtx

using namespace vtx;

extern "C" int vtx_clips_views_u8(int B, int T, int H, int V, int W, int Wr_max, const void* const* src, const int32_t* geom,
                                  unsigned char* dst, const int32_t* frames, const int32_t* left, const int32_t* x_first,
                                  const int32_t* x_count, const float* x_weights, int x_taps, const int32_t* y_first,
                                  const int32_t* y_count, const float* y_weights, int y_taps, void* stream) {
  VTX_REQUIRE(B > 0 && T > 0 && H > 0 && V > 0 && W > 0 && Wr_max > 0 && x_taps > 0 && y_taps > 0, VTX_EINVAL,
              "clips_views_u8: B=%d T=%d rows %d views %d of width %d widest resized row %d taps %d/%d must all be positive",
              B, T, H, V, W, Wr_max, x_taps, y_taps);
  VTX_REQUIRE(V <= MAX_VIEWS, VTX_EINVAL, "clips_views_u8: %d views, at most %d are supported", V, MAX_VIEWS);
  VTX_REQUIRE(W <= Wr_max, VTX_EINVAL, "clips_views_u8: a view of %d columns does not fit the widest resized row of %d", W, Wr_max);
  VTX_REQUIRE(src && geom && dst && left && x_first && x_count && x_weights && y_first && y_count && y_weights, VTX_EINVAL,
              "clips_views_u8: null pointer");
  VTX_REQUIRE((reinterpret_cast<uintptr_t>(src) & 7u) == 0, VTX_EALIGN,
              "clips_views_u8: the pointer table must be 8-byte aligned (place it first in a packed upload)");
  const long bands = (H + BAND_ROWS - 1) / BAND_ROWS;
  VTX_REQUIRE((long)B * T <= 65535 && bands <= 65535, VTX_EINVAL, "clips_views_u8: %ld frames / %ld row bands exceed the grid (65535 each)", (long)B * T, bands);
  dim3 grid((unsigned)((Wr_max + 255) / 256), (unsigned)bands, (unsigned)(B * T));
  hipLaunchKernelGGL(clips_views_u8_kernel, grid, dim3(256), 0, as_stream(stream), T, H, V, W, Wr_max,
                     reinterpret_cast<const uint8_t* const*>(src), geom, dst, frames, left, x_first, x_count, x_weights, x_taps,
                     y_first, y_count, y_weights, y_taps);
  return check_launch("clips_views_u8");
}
