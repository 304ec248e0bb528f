// yuv.hip -- decoded 4:2:0 YUV clips (NV12, I420) into the clip resampler: the colour conversion happens on each tap, in
// registers, so the RGB source clip that a decoder's CPU conversion would have produced never exists.
//
// No decoder yields RGB: ffmpeg-based readers (the reference's decord, dataset.py:101-113,163) decode to planar 4:2:0 and get
// [T,H,W,3] by a swscale pass on the CPU workers; the GPU's own decode engines write NV12.  4:2:0 is 1.5 bytes per pixel
// against 3, over PCIe and as source bytes of a resampler that is bound by the bytes it reads (aug.hip).
//
//   dst[b, v, t] = columns left[b,v] .. left[b,v] + W of the resized frame  Wy[b] * rgb(clip b)[frames[b,t]] * Wx[b]^T
//
// The conversion (include/vtx_yuv.h has the contract) is a per-pixel integer map, so it commutes with everything the
// resampler does to a tap: clips_views_yuv420_kernel is clips_views_u8_kernel (ragged.hip) with another tap reader handed to
// the same resample_band (resample_band.h) -- x pass, then y pass, taps in ascending order, float32 without fma contraction,
// clamp to [0, 255], round half-to-even -- and gives byte for byte what that kernel gives on the converted clips.
// yuv420_to_rgb_u8_kernel writes those converted clips, for callers that want them and as the tests' second route.
//
// Per tap: one luma byte and the chroma pair of column (fx + k) >> 1 -- adjacent lanes and adjacent taps share it, so the
// chroma loads hit the same lines twice -- and 5 integer multiply-adds, 3 shifts and 3 clamps in front of the 3 conversions to
// float the RGB reader has too.
//
// A library of its own, libvtx_yuv.so (include/vtx_yuv.h): the other eight keep their symbols and versions.
// Error plumbing, version and last-error exports: VTX_SIDE_LIB(yuv) (side_lib.h).
#include "side_lib.h"
#include "resample_band.h"
#include "../../include/vtx_yuv.h"

VTX_SIDE_LIB(yuv)

namespace vtx {

static_assert(sizeof(vtx_yuv420_clip) == 88 && alignof(vtx_yuv420_clip) == 8, "vtx/ops.py packs the record as 22 int32");

// the six matrix entries, as the contract bounds them whatever the record says: no sum below can leave +-2^22
struct YuvMatrix {
  int y_off, c_y, c_rv, c_gu, c_gv, c_bu;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ YuvMatrix load_matrix(const int32_t* m) {
  return YuvMatrix{clampi(m[0], 0, 255), clampi(m[1], -4096, 4096), clampi(m[2], -4096, 4096), clampi(m[3], -4096, 4096),
                   clampi(m[4], -4096, 4096), clampi(m[5], -4096, 4096)};
}

// (Y, U, V) -> R, G, B in 0 .. 255: int32, the shift is arithmetic (floor, also for negative sums)
__device__ __forceinline__ void yuv_to_rgb(const YuvMatrix& m, int Y, int U, int V, int& R, int& G, int& B) {
  const int C = (Y - m.y_off) * m.c_y + 128, D = U - 128, E = V - 128;
  R = clampi((C + m.c_rv * E) >> 8, 0, 255);
  G = clampi((C - m.c_gu * D - m.c_gv * E) >> 8, 0, 255);
  B = clampi((C + m.c_bu * D) >> 8, 0, 255);
}

// a record the kernels can walk without leaving what it describes (the pointers aside); the same for the whole workgroup
__device__ __forceinline__ bool walkable(const vtx_yuv420_clip& d) {
  return d.Ts >= 1 && d.Hs >= 1 && d.Ws >= 1 && (d.c_step == 1 || d.c_step == 2) && d.y_pitch >= d.Ws &&
         d.c_pitch >= ((d.Ws + 1) >> 1) * d.c_step && d.y_frame >= 0 && d.c_frame >= 0;
}

// The tap reader of one 4:2:0 frame for resample_band: the planes at the frame, pitches, chroma step and the matrix.
struct Yuv420Taps {
  struct Source {
    const uint8_t* __restrict__ y;
    const uint8_t* __restrict__ u;
    const uint8_t* __restrict__ v;
    int y_pitch, c_pitch, c_step;
    YuvMatrix m;
  };
  struct Row {
    const uint8_t* __restrict__ py;                      // the luma row at column fx
    const uint8_t* __restrict__ pu;                      // the chroma row (s >> 1) at column 0
    const uint8_t* __restrict__ pv;
    int fx, c_step;
    YuvMatrix m;
    __device__ __forceinline__ float3 tap(int k) const {
      const int c = ((fx + k) >> 1) * c_step;
      int R, G, B;
      yuv_to_rgb(m, py[k], pu[c], pv[c], R, G, B);
      return make_float3((float)R, (float)G, (float)B);
    }
  };
  static __device__ __forceinline__ Row row(const Source& f, int /*Ws*/, int s, int fx) {
    const long c = (long)(s >> 1) * f.c_pitch;
    return Row{f.y + (long)s * f.y_pitch + fx, f.u + c, f.v + c, fx, f.c_step, f.m};
  }
};

// One workgroup per (clip and selected frame, band of BAND_ROWS output rows, 256 columns of the widest resized row):
// clips_views_u8_kernel (ragged.hip) with the clip's record in the place of its base pointer and geometry.  The window test
// in front of the band and the store behind it are that kernel's text (written in each kernel: resample_band.h says why).
// Everything is clamped with the clip's own Ts / Hs / Ws / Wr whatever the arrays say; the caller validates them, and the
// pointers.
__global__ __launch_bounds__(256) void clips_views_yuv420_kernel(int T, int H, int V, int W, int Wr_max,
                                                                 const vtx_yuv420_clip* __restrict__ clips, uint8_t* __restrict__ dst,
                                                                 const int* __restrict__ frames, const int* __restrict__ left,
                                                                 const int* __restrict__ xf, const int* __restrict__ xc,
                                                                 const float* __restrict__ xw, int xt,
                                                                 const int* __restrict__ yf, const int* __restrict__ yc,
                                                                 const float* __restrict__ yw, int yt) {
  const int b = blockIdx.z / T, t = blockIdx.z - b * T;
  // the clip's record: the same for the whole workgroup
  const vtx_yuv420_clip& d = clips[b];
  const int Ts = d.Ts, Hs = d.Hs, Ws = d.Ws;
  int Wr = d.Wr;
  Wr = Wr > Wr_max ? Wr_max : Wr;                        // the table rows hold Wr_max entries
  if (!walkable(d) || Wr < W) return;                    // (the host refuses such a record)
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
  const long fy = (long)ts * d.y_frame, fc = (long)ts * d.c_frame;
  const Yuv420Taps::Source frame{d.y + fy, d.u + fc, d.v + fc, d.y_pitch, d.c_pitch, d.c_step, load_matrix(d.matrix)};
  resample_band<Yuv420Taps>(frame, Hs, Ws, H, r0, xf[col], xc[col], xw + col * xt, xt,
                            yf + (long)b * H, yc + (long)b * H, yw + (long)b * H * yt, yt, [=](int r, uint8_t q0, uint8_t q1, uint8_t q2) {
#pragma unroll
                              for (int v = 0; v < MAX_VIEWS; ++v) {
                                if (off[v] < 0) continue;
                                uint8_t* o = dst + (((((long)b * V + v) * T + t) * H + r0 + r) * W + off[v]) * 3;
                                o[0] = q0; o[1] = q1; o[2] = q2;
                              }
                            });
}

// dst [Ts,Hs,Ws,3] = rgb(*clip).  One workgroup per (row of a frame, 256 columns) tile, grid-stride over the tiles: the tile's
// frame, row and first column are the same for every thread (scalar divisions).  Reads are clamped into the record's own
// Ts / Hs / Ws, stores bounded by the arguments, which describe dst.
__global__ __launch_bounds__(256) void yuv420_to_rgb_u8_kernel(const vtx_yuv420_clip* __restrict__ clip, int Ts, int Hs, int Ws,
                                                               uint8_t* __restrict__ dst) {
  const vtx_yuv420_clip& d = *clip;
  if (!walkable(d)) return;
  const YuvMatrix m = load_matrix(d.matrix);
  const int chunks = (Ws + 255) / 256;
  const long tiles = (long)Ts * Hs * chunks;
  for (long j = blockIdx.x; j < tiles; j += gridDim.x) {
    const int line = (int)(j / chunks);                  // t * Hs + s
    const int x = (int)(j - (long)line * chunks) * 256 + threadIdx.x;
    if (x >= Ws) continue;
    const int t = line / Hs, s = line - t * Hs;
    const int tc = t > d.Ts - 1 ? d.Ts - 1 : t, sc = s > d.Hs - 1 ? d.Hs - 1 : s, xs = x > d.Ws - 1 ? d.Ws - 1 : x;
    const long c = (long)tc * d.c_frame + (long)(sc >> 1) * d.c_pitch + (xs >> 1) * d.c_step;
    int R, G, B;
    yuv_to_rgb(m, d.y[(long)tc * d.y_frame + (long)sc * d.y_pitch + xs], d.u[c], d.v[c], R, G, B);
    uint8_t* o = dst + ((long)line * Ws + x) * 3;
    o[0] = (uint8_t)R; o[1] = (uint8_t)G; o[2] = (uint8_t)B;
  }
}

}  // namespace vtx

using namespace vtx;

extern "C" int vtx_clips_views_yuv420(int B, int T, int H, int V, int W, int Wr_max, const vtx_yuv420_clip* clips, unsigned char* dst,
                                      const int32_t* frames, const int32_t* left, const int32_t* x_first, const int32_t* x_count,
                                      const float* x_weights, int x_taps, const int32_t* y_first, const int32_t* y_count,
                                      const float* y_weights, int y_taps, void* stream) {
  VTX_REQUIRE(B > 0 && T > 0 && H > 0 && V > 0 && W > 0 && Wr_max > 0 && x_taps > 0 && y_taps > 0, VTX_EINVAL,
              "clips_views_yuv420: B=%d T=%d rows %d views %d of width %d widest resized row %d taps %d/%d must all be positive",
              B, T, H, V, W, Wr_max, x_taps, y_taps);
  VTX_REQUIRE(V <= MAX_VIEWS, VTX_EINVAL, "clips_views_yuv420: %d views, at most %d are supported", V, MAX_VIEWS);
  VTX_REQUIRE(W <= Wr_max, VTX_EINVAL, "clips_views_yuv420: a view of %d columns does not fit the widest resized row of %d", W, Wr_max);
  VTX_REQUIRE(clips && dst && left && x_first && x_count && x_weights && y_first && y_count && y_weights, VTX_EINVAL,
              "clips_views_yuv420: null pointer");
  VTX_REQUIRE((reinterpret_cast<uintptr_t>(clips) & 7u) == 0, VTX_EALIGN,
              "clips_views_yuv420: the clip records must be 8-byte aligned (place them first in a packed upload)");
  const long bands = (H + BAND_ROWS - 1) / BAND_ROWS;
  VTX_REQUIRE((long)B * T <= 65535 && bands <= 65535, VTX_EINVAL, "clips_views_yuv420: %ld frames / %ld row bands exceed the grid (65535 each)", (long)B * T, bands);
  dim3 grid((unsigned)((Wr_max + 255) / 256), (unsigned)bands, (unsigned)(B * T));
  hipLaunchKernelGGL(clips_views_yuv420_kernel, grid, dim3(256), 0, as_stream(stream), T, H, V, W, Wr_max, clips, dst, frames, left,
                     x_first, x_count, x_weights, x_taps, y_first, y_count, y_weights, y_taps);
  return check_launch("clips_views_yuv420");
}

extern "C" int vtx_yuv420_to_rgb_u8(const vtx_yuv420_clip* clip, int Ts, int Hs, int Ws, unsigned char* dst, void* stream) {
  VTX_REQUIRE(Ts > 0 && Hs > 0 && Ws > 0, VTX_EINVAL, "yuv420_to_rgb_u8: Ts=%d frames of %dx%d must all be positive", Ts, Hs, Ws);
  VTX_REQUIRE((long)Ts * Hs < (1L << 31), VTX_EINVAL, "yuv420_to_rgb_u8: %ld rows exceed 2^31", (long)Ts * Hs);
  VTX_REQUIRE(clip && dst, VTX_EINVAL, "yuv420_to_rgb_u8: null pointer");
  VTX_REQUIRE((reinterpret_cast<uintptr_t>(clip) & 7u) == 0, VTX_EALIGN, "yuv420_to_rgb_u8: the clip record must be 8-byte aligned");
  const long tiles = (long)Ts * Hs * ((Ws + 255) / 256);
  hipLaunchKernelGGL(yuv420_to_rgb_u8_kernel, dim3(grid_for(tiles * 256, 16384)), dim3(256), 0, as_stream(stream), clip, Ts, Hs, Ws, dst);
  return check_launch("yuv420_to_rgb_u8");
}
