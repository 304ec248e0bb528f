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
// The kernel is clip_views_u8_kernel (csrc/views.hip) restated, with the clip's base pointer and Ts / Hs / Ws / Wr read per
// workgroup: b = blockIdx.z / T is the same for every thread, so these are scalar registers.  The x tables have one row
// stride, Wr_max, for all clips; row b is valid for x < Wr_b.  The grid covers Wr_max columns: a column tile beyond a
// clip's Wr_b, or in none of its windows, returns before any load.
//
// Arithmetic contract: that kernel's, statement for statement -- x pass first, then the y pass, taps in ascending order,
// float32 without fma contraction, clamp to [0, 255], round half-to-even -- so clip b's views are byte for byte what
// vtx_clip_views_u8 gives on clip b alone with its rows of the tables.
//
// A library of its own, libvtx_ragged.so (include/vtx_ragged.h): the other six keep their symbols and versions.
// The error plumbing common.h declares is defined here for this library (the link is -Bsymbolic).
#include <math.h>
#include <stdarg.h>
#include <string.h>
#include "common.h"
#include "../../include/vtx_ragged.h"

namespace vtx {

static thread_local char g_ragged_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_ragged_err, sizeof(g_ragged_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return VTX_ELAUNCH;
  }
  return VTX_OK;
}

// One thread per column x of the clip's resized frame (all three channels), one workgroup per (clip and selected frame,
// band of RG_ROWS output rows, 256 columns), as in views.hip.  Frame index, window lefts and tap windows are clamped with
// the clip's own Ts / Hs / Ws / Wr whatever the arrays say; the caller validates them, and the pointers.
constexpr int RG_ROWS = 8;       // output rows per band (views.hip: VW_ROWS)
constexpr int RG_MAX_VIEWS = 8;

__global__ __launch_bounds__(256) void clips_views_u8_kernel(int T, int H, int V, int W, int Wr_max,
                                                             const uint8_t* const* __restrict__ src, const int* __restrict__ geom,
                                                             uint8_t* __restrict__ dst,
                                                             const int* __restrict__ frames, const int* __restrict__ left,
                                                             const int* __restrict__ xf, const int* __restrict__ xc,
                                                             const float* __restrict__ xw, int xt,
                                                             const int* __restrict__ yf, const int* __restrict__ yc,
                                                             const float* __restrict__ yw, int yt) {
#pragma clang fp contract(off)
  const int b = blockIdx.z / T, t = blockIdx.z - b * T;
  // the clip's descriptor: the same for the whole workgroup
  const int Ts = geom[4 * b], Hs = geom[4 * b + 1], Ws = geom[4 * b + 2];
  int Wr = geom[4 * b + 3];
  Wr = Wr > Wr_max ? Wr_max : Wr;                        // the table rows hold Wr_max entries
  if (Ts < 1 || Hs < 1 || Ws < 1 || Wr < W) return;      // (the host refuses such a record)
  const int r0 = blockIdx.y * RG_ROWS;
  const int x = blockIdx.x * 256 + threadIdx.x;
  // the views whose window holds this column (the lefts are the same for every thread: scalar registers)
  int off[RG_MAX_VIEWS];
  bool any = false;
#pragma unroll
  for (int v = 0; v < RG_MAX_VIEWS; ++v) {
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
  // this thread's x taps, clamped into the source row
  int fx = xf[(long)b * Wr_max + x], cx = xc[(long)b * Wr_max + x];
  cx = cx < 0 ? 0 : (cx > xt ? xt : cx);
  fx = fx < 0 ? 0 : (fx > Ws ? Ws : fx);
  if (fx + cx > Ws) { fx = Ws - cx < 0 ? 0 : Ws - cx; cx = cx > Ws ? Ws : cx; }
  const float* wx = xw + ((long)b * Wr_max + x) * xt;
  // the band's y windows
  int fy[RG_ROWS], cy[RG_ROWS];
  int lo = Hs, hi = 0;
#pragma unroll
  for (int r = 0; r < RG_ROWS; ++r) {
    const int ri = r0 + r < H ? r0 + r : H - 1;
    int f = yf[(long)b * H + ri], c = yc[(long)b * H + ri];
    c = c < 0 ? 0 : (c > yt ? yt : c);
    f = f < 0 ? 0 : (f > Hs ? Hs : f);
    if (f + c > Hs) { f = Hs - c < 0 ? 0 : Hs - c; c = c > Hs ? Hs : c; }
    if (r0 + r >= H) c = 0;
    fy[r] = f; cy[r] = c;
    if (c > 0) { lo = f < lo ? f : lo; hi = f + c > hi ? f + c : hi; }
  }
  float acc[RG_ROWS][3];
#pragma unroll
  for (int r = 0; r < RG_ROWS; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.0f;
  const uint8_t* img = src[b] + (long)ts * Hs * Ws * 3;
  for (int s = lo; s < hi; ++s) {
    const uint8_t* p = img + ((long)s * Ws + fx) * 3;
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    for (int k = 0; k < cx; ++k) {
      const float w = wx[k];
      v0 = v0 + w * (float)p[3 * k];
      v1 = v1 + w * (float)p[3 * k + 1];
      v2 = v2 + w * (float)p[3 * k + 2];
    }
#pragma unroll
    for (int r = 0; r < RG_ROWS; ++r) {
      const int k = s - fy[r];
      if (k >= 0 && k < cy[r]) {
        const float w = yw[((long)b * H + r0 + r) * yt + k];
        acc[r][0] = acc[r][0] + w * v0;
        acc[r][1] = acc[r][1] + w * v1;
        acc[r][2] = acc[r][2] + w * v2;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RG_ROWS; ++r) {
    if (r0 + r >= H) break;
    uint8_t q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      q[c] = (uint8_t)(int)__builtin_rintf(fminf(fmaxf(acc[r][c], 0.0f), 255.0f));      // half-to-even, as torch.round
#pragma unroll
    for (int v = 0; v < RG_MAX_VIEWS; ++v) {
      if (off[v] < 0) continue;
      uint8_t* o = dst + (((((long)b * V + v) * T + t) * H + r0 + r) * W + off[v]) * 3;
      o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
    }
  }
}

}  // namespace vtx

using namespace vtx;

extern "C" int vtx_ragged_version(void) { return 100; }  // 0.1.0
extern "C" const char* vtx_ragged_last_error_string(void) { return g_ragged_err; }

extern "C" int vtx_clips_views_u8(int B, int T, int H, int V, int W, int Wr_max, const void* const* src, const int32_t* geom,
                                  unsigned char* dst, const int32_t* frames, const int32_t* left, const int32_t* x_first,
                                  const int32_t* x_count, const float* x_weights, int x_taps, const int32_t* y_first,
                                  const int32_t* y_count, const float* y_weights, int y_taps, void* stream) {
  VTX_REQUIRE(B > 0 && T > 0 && H > 0 && V > 0 && W > 0 && Wr_max > 0 && x_taps > 0 && y_taps > 0, VTX_EINVAL,
              "clips_views_u8: B=%d T=%d rows %d views %d of width %d widest resized row %d taps %d/%d must all be positive",
              B, T, H, V, W, Wr_max, x_taps, y_taps);
  VTX_REQUIRE(V <= RG_MAX_VIEWS, VTX_EINVAL, "clips_views_u8: %d views, at most %d are supported", V, RG_MAX_VIEWS);
  VTX_REQUIRE(W <= Wr_max, VTX_EINVAL, "clips_views_u8: a view of %d columns does not fit the widest resized row of %d", W, Wr_max);
  VTX_REQUIRE(src && geom && dst && left && x_first && x_count && x_weights && y_first && y_count && y_weights, VTX_EINVAL,
              "clips_views_u8: null pointer");
  VTX_REQUIRE((reinterpret_cast<uintptr_t>(src) & 7u) == 0, VTX_EALIGN,
              "clips_views_u8: the pointer table must be 8-byte aligned (place it first in a packed upload)");
  const long bands = (H + RG_ROWS - 1) / RG_ROWS;
  VTX_REQUIRE((long)B * T <= 65535 && bands <= 65535, VTX_EINVAL, "clips_views_u8: %ld frames / %ld row bands exceed the grid (65535 each)", (long)B * T, bands);
  dim3 grid((unsigned)((Wr_max + 255) / 256), (unsigned)bands, (unsigned)(B * T));
  hipLaunchKernelGGL(clips_views_u8_kernel, grid, dim3(256), 0, as_stream(stream), T, H, V, W, Wr_max,
                     reinterpret_cast<const uint8_t* const*>(src), geom, dst, frames, left, x_first, x_count, x_weights, x_taps,
                     y_first, y_count, y_weights, y_taps);
  return check_launch("clips_views_u8");
}
