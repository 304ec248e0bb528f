// views.hip -- test-time views of decoded uint8 clips in one launch: frame selection, Resize and the crops of ThreeCrop, the
// steps of the reference's test pipeline (data_trainer.py:108-121: Resize(short side) -> ThreeCrop(img_size)) that precede
// ToTensor + Normalize, together with the frame gather that precedes every pipeline (TemporalRandomCrop + np.linspace,
// data_transform.py:475-489, dataset.py:160-162).
//
//   dst[b, v, t] = columns left[b,v] .. left[b,v] + W of the resized frame  Wy[b] * src[b, frames[b,t]] * Wx[b]^T
//
// The x tables cover ALL Wr columns of the resized frame and the y tables the H rows of the crop window (the caller cuts
// them, as ClipEval does), so a view is a window of columns of one resized row.  ThreeCrop's windows share their rows and
// overlap in x (256x341 -> lefts 0, 117, 58: 341 distinct columns for 3 x 224 stored ones): the kernel resamples each
// column of the union once and stores it to every view whose window holds it.  Columns in no view are not computed.
//
// Arithmetic contract: that of clip_resample_u8_kernel (csrc/aug.hip), because both run resample_band (resample_band.h) --
// x pass first, then the y pass, taps in ascending order, float32 without fma contraction, clamp to [0, 255], round
// half-to-even -- so a view is byte for byte what vtx_clip_resample_u8 gives on the gathered frames with the same tables,
// sliced to the window.
//
// Bytes: per selected frame Hs*Ws*3 read (the rows of the crop window) and V*H*W*3 written; the composition it
// replaces (gathered copy of the source, one resampling pass per view, concatenating copy) reads and writes the selected
// source frames once more, reads them V times and moves the result three times.
//
// A library of its own, libvtx_views.so (include/vtx_views.h): libvtx_aug.so keeps its seven symbols and its version.
// Error plumbing, version and last-error exports: VTX_SIDE_LIB(views) (side_lib.h).
#include "side_lib.h"
#include "resample_band.h"
#include "../../include/vtx_views.h"

VTX_SIDE_LIB(views)

namespace vtx {

// One thread per column x of the resized frame (all three channels), one workgroup per (selected frame, band of BAND_ROWS
// output rows, 256 columns).  A column is resampled once (resample_band) and stored to every view whose window holds it; a
// column in no view returns before any table load.  Frame index, window lefts and tap windows are clamped here whatever the
// tables say; the caller validates them.
__global__ __launch_bounds__(256) void clip_views_u8_kernel(int Ts, int T, int Hs, int Ws, int H, int Wr, int V, int W,
                                                            const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            const int* __restrict__ frames, const int* __restrict__ left,
                                                            const int* __restrict__ xf, const int* __restrict__ xc,
                                                            const float* __restrict__ xw, int xt,
                                                            const int* __restrict__ yf, const int* __restrict__ yc,
                                                            const float* __restrict__ yw, int yt) {
  const int b = blockIdx.z / T, t = blockIdx.z - b * T;
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
  if (!any) return;                                      // also every x >= Wr: l + W <= Wr
  int ts = frames ? frames[b * T + t] : t;
  ts = ts < 0 ? 0 : (ts > Ts - 1 ? Ts - 1 : ts);
  const long col = (long)b * Wr + x;
  resample_band(src + ((long)b * Ts + ts) * Hs * Ws * 3, Hs, Ws, H, r0, xf[col], xc[col], xw + col * xt, xt,
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

extern "C" int vtx_clip_views_u8(int B, int Ts, int T, int Hs, int Ws, int H, int Wr, int V, int W, const unsigned char* src,
                                 unsigned char* dst, const int32_t* frames, const int32_t* left, const int32_t* x_first,
                                 const int32_t* x_count, const float* x_weights, int x_taps, const int32_t* y_first,
                                 const int32_t* y_count, const float* y_weights, int y_taps, void* stream) {
  VTX_REQUIRE(B > 0 && Ts > 0 && T > 0 && Hs > 0 && Ws > 0 && H > 0 && Wr > 0 && V > 0 && W > 0 && x_taps > 0 && y_taps > 0, VTX_EINVAL,
              "clip_views_u8: B=%d Ts=%d T=%d source %dx%d rows %d resized width %d views %d of width %d taps %d/%d must all be positive",
              B, Ts, T, Hs, Ws, H, Wr, V, W, x_taps, y_taps);
  VTX_REQUIRE(V <= MAX_VIEWS, VTX_EINVAL, "clip_views_u8: %d views, at most %d are supported", V, MAX_VIEWS);
  VTX_REQUIRE(W <= Wr, VTX_EINVAL, "clip_views_u8: a view of %d columns does not fit the resized row of %d", W, Wr);
  VTX_REQUIRE(src && dst && left && x_first && x_count && x_weights && y_first && y_count && y_weights, VTX_EINVAL, "clip_views_u8: null pointer");
  VTX_REQUIRE(frames || T == Ts, VTX_EINVAL, "clip_views_u8: without frame indices every frame is taken: T=%d, Ts=%d", T, Ts);
  VTX_REQUIRE(src != dst, VTX_EINVAL, "clip_views_u8: in place is not supported");
  const long bands = (H + BAND_ROWS - 1) / BAND_ROWS;
  VTX_REQUIRE((long)B * T <= 65535 && bands <= 65535, VTX_EINVAL, "clip_views_u8: %ld frames / %ld row bands exceed the grid (65535 each)", (long)B * T, bands);
  dim3 grid((unsigned)((Wr + 255) / 256), (unsigned)bands, (unsigned)(B * T));
  hipLaunchKernelGGL(clip_views_u8_kernel, grid, dim3(256), 0, as_stream(stream), Ts, T, Hs, Ws, H, Wr, V, W, src, dst, frames, left,
                     x_first, x_count, x_weights, x_taps, y_first, y_count, y_weights, y_taps);
  return check_launch("clip_views_u8");
}
