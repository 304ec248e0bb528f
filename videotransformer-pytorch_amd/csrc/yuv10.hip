// yuv10.hip -- decoded 10-bit 4:2:0 YUV clips (P010, yuv420p10le) into the clip resampler, in one launch with 8-bit ones
// (NV12, I420): yuv.hip with a tap reader that loads 8- or 16-bit samples.
//
// Phone cameras, HEVC Main10 and AV1 give 10-bit streams; the GPU's decode engines write them as P010 (16-bit words, the
// sample in the upper 10 bits, chroma interleaved), ffmpeg-based readers as yuv420p10le (planar, the sample in the lower 10
// bits).  3 bytes per pixel, what an RGB24 clip has, but no swscale pass on the CPU workers, and the batch stays one list.
//
//   dst[b, v, t] = columns left[b,v] .. left[b,v] + W of the resized frame  Wy[b] * rgb(clip b)[frames[b,t]] * Wx[b]^T
//
// include/vtx_yuv10.h has the contract: one record type for both depths (pitches in bytes, chroma step in samples, depth,
// shift), a 12-bit integer matrix on the 10-bit samples, the contract of vtx_yuv.h on 8-bit ones.  The depth is the clip's,
// so the branch between the two readers is the same for a whole workgroup; each reader is handed to the same resample_band
// (resample_band.h), which gives byte for byte what clips_views_u8_kernel (ragged.hip) gives on the converted clips.
//
// Per tap: one luma sample and the chroma pair of column (fx + k) >> 1 -- adjacent lanes and adjacent taps share it.  The
// pair of an interleaved 16-bit plane is read as two 16-bit loads, not one 32-bit word: a plane that is a sliced view of a
// wider buffer starts at any even address, two loads of one line cost no more bytes, and the 32-bit load behind a
// per-workgroup alignment test measured slower on every 10-bit path (profiles/clip_yuv10_bench.txt).  A 16-bit sample is one
// bit-field extract (shift, 10 bits) behind its load; the rest is yuv.hip's 5 integer multiply-adds, 3 shifts and 3 clamps.
//
// A library of its own, libvtx_yuv10.so (include/vtx_yuv10.h): the other nine keep their symbols and versions.
// Error plumbing, version and last-error exports: VTX_SIDE_LIB(yuv10) (side_lib.h).
#include "side_lib.h"
#include "resample_band.h"
#include "../../include/vtx_yuv10.h"

VTX_SIDE_LIB(yuv10)

namespace vtx {

static_assert(sizeof(vtx_yuv10_clip) == 96 && alignof(vtx_yuv10_clip) == 8, "vtx/ops.py packs the record as 24 int32");

// What differs between the two contracts: a sample's storage, the chroma centre, the fractional bits of the matrix and the
// bounds that keep the int32 sums in range (8: +-2^22, 10: +-2^26).
template <int DEPTH> struct Contract;
template <> struct Contract<8> {
  typedef uint8_t Sample;
  static constexpr int CENTRE = 128, FRAC = 8, Y_OFF_MAX = 255, C_MAX = 4096;
  static __device__ __forceinline__ int sample(uint8_t w, int /*shift*/) { return w; }
};
template <> struct Contract<10> {
  typedef uint16_t Sample;
  static constexpr int CENTRE = 512, FRAC = 12, Y_OFF_MAX = 1023, C_MAX = 16384;
  // the word moved right by `shift` and masked to 10 bits: what else it holds (P010's low 6, the upper 6 of an LSB-aligned
  // word) does not reach the result
  // (shift-and-mask in C: the compiler sees the 10 bits, forms the products with 24-bit multiplies and folds the pair into
  // one bit-field extract all the same)
  static __device__ __forceinline__ int sample(uint16_t w, int shift) { return ((int)w >> shift) & 1023; }
};

// the six matrix entries, as the contract of the depth bounds them whatever the record says
struct YuvMatrix {
  int y_off, c_y, c_rv, c_gu, c_gv, c_bu;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int DEPTH>
__device__ __forceinline__ YuvMatrix load_matrix(const int32_t* m) {
  constexpr int c = Contract<DEPTH>::C_MAX;
  return YuvMatrix{clampi(m[0], 0, Contract<DEPTH>::Y_OFF_MAX), clampi(m[1], -c, c), clampi(m[2], -c, c), clampi(m[3], -c, c),
                   clampi(m[4], -c, c), clampi(m[5], -c, c)};
}

// (Y, U, V) -> R, G, B in 0 .. 255: int32, the shift is arithmetic (floor, also for negative sums)
template <int DEPTH>
__device__ __forceinline__ void yuv_to_rgb(const YuvMatrix& m, int Y, int U, int V, int& R, int& G, int& B) {
  constexpr int f = Contract<DEPTH>::FRAC;
  const int C = (Y - m.y_off) * m.c_y + (1 << (f - 1)), D = U - Contract<DEPTH>::CENTRE, E = V - Contract<DEPTH>::CENTRE;
  R = clampi((C + m.c_rv * E) >> f, 0, 255);
  G = clampi((C - m.c_gu * D - m.c_gv * E) >> f, 0, 255);
  B = clampi((C + m.c_bu * D) >> f, 0, 255);
}

// a record the kernels can walk without leaving what it describes (the pointers' extents aside); the same for the whole
// workgroup.  With 16-bit samples every address the kernels form is even: bases, pitches and frame strides are.
__device__ __forceinline__ bool walkable(const vtx_yuv10_clip& d) {
  if (d.depth != 8 && d.depth != 10) return false;
  const int size = d.depth == 8 ? 1 : 2;
  if (d.depth == 8 ? d.shift != 0 : (d.shift != 0 && d.shift != 6)) return false;
  if (size == 2 && ((reinterpret_cast<uintptr_t>(d.y) | reinterpret_cast<uintptr_t>(d.u) | reinterpret_cast<uintptr_t>(d.v) |
                     (unsigned)d.y_pitch | (unsigned)d.y_frame | (unsigned)d.c_pitch | (unsigned)d.c_frame) & 1u))
    return false;
  return d.Ts >= 1 && d.Hs >= 1 && d.Ws >= 1 && (d.c_step == 1 || d.c_step == 2) && d.y_pitch >= (long)d.Ws * size &&
         d.c_pitch >= (long)((d.Ws + 1) >> 1) * d.c_step * size && d.y_frame >= 0 && d.c_frame >= 0;
}

// byte offset -> the sample there
template <typename S>
__device__ __forceinline__ const S* at(const void* base, long bytes) {
  return reinterpret_cast<const S*>(static_cast<const uint8_t*>(base) + bytes);
}

// The tap reader of one 4:2:0 frame of depth DEPTH for resample_band: the planes at the frame, pitches (bytes), chroma step
// (samples), shift and the matrix.
template <int DEPTH>
struct Yuv10Taps {
  typedef typename Contract<DEPTH>::Sample S;
  struct Source {
    const S* __restrict__ y;
    const S* __restrict__ u;
    const S* __restrict__ v;
    int y_pitch, c_pitch, c_step, shift;
    YuvMatrix m;
  };
  struct Row {
    const S* __restrict__ py;                            // the luma row at column fx
    const S* __restrict__ pu;                            // the chroma row (s >> 1) at column 0
    const S* __restrict__ pv;
    int fx, c_step, shift;
    YuvMatrix m;
    __device__ __forceinline__ float3 tap(int k) const {
      const int c = ((fx + k) >> 1) * c_step;
      int R, G, B;
      yuv_to_rgb<DEPTH>(m, Contract<DEPTH>::sample(py[k], shift), Contract<DEPTH>::sample(pu[c], shift),
                        Contract<DEPTH>::sample(pv[c], shift), R, G, B);
      return make_float3((float)R, (float)G, (float)B);
    }
  };
  static __device__ __forceinline__ Row row(const Source& f, int /*Ws*/, int s, int fx) {
    const long c = (long)(s >> 1) * f.c_pitch;
    return Row{at<S>(f.y, (long)s * f.y_pitch) + fx, at<S>(f.u, c), at<S>(f.v, c), fx, f.c_step, f.shift, f.m};
  }
  static __device__ __forceinline__ Source frame(const vtx_yuv10_clip& d, int ts) {
    const long fy = (long)ts * d.y_frame, fc = (long)ts * d.c_frame;
    return Source{at<S>(d.y, fy), at<S>(d.u, fc), at<S>(d.v, fc), d.y_pitch, d.c_pitch, d.c_step, d.shift, load_matrix<DEPTH>(d.matrix)};
  }
};

// One workgroup per (clip and selected frame, band of BAND_ROWS output rows, 256 columns of the widest resized row):
// clips_views_yuv420_kernel (yuv.hip) with a reader chosen by the record's depth.  The window test in front of the band and
// the store behind it are that kernel's text (written in each kernel: resample_band.h says why).  Everything is clamped with
// the clip's own Ts / Hs / Ws / Wr whatever the arrays say; the caller validates them, and the pointers.
__global__ __launch_bounds__(256) void clips_views_yuv10_kernel(int T, int H, int V, int W, int Wr_max,
                                                                const vtx_yuv10_clip* __restrict__ clips, uint8_t* __restrict__ dst,
                                                                const int* __restrict__ frames, const int* __restrict__ left,
                                                                const int* __restrict__ xf, const int* __restrict__ xc,
                                                                const float* __restrict__ xw, int xt,
                                                                const int* __restrict__ yf, const int* __restrict__ yc,
                                                                const float* __restrict__ yw, int yt) {
  const int b = blockIdx.z / T, t = blockIdx.z - b * T;
  // the clip's record: the same for the whole workgroup
  const vtx_yuv10_clip& d = clips[b];
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
  const auto store = [=](int r, uint8_t q0, uint8_t q1, uint8_t q2) {
#pragma unroll
    for (int v = 0; v < MAX_VIEWS; ++v) {
      if (off[v] < 0) continue;
      uint8_t* o = dst + (((((long)b * V + v) * T + t) * H + r0 + r) * W + off[v]) * 3;
      o[0] = q0; o[1] = q1; o[2] = q2;
    }
  };
  if (d.depth == 8)                                      // the same for the whole workgroup
    resample_band<Yuv10Taps<8>>(Yuv10Taps<8>::frame(d, ts), Hs, Ws, H, r0, xf[col], xc[col], xw + col * xt, xt,
                                yf + (long)b * H, yc + (long)b * H, yw + (long)b * H * yt, yt, store);
  else
    resample_band<Yuv10Taps<10>>(Yuv10Taps<10>::frame(d, ts), Hs, Ws, H, r0, xf[col], xc[col], xw + col * xt, xt,
                                 yf + (long)b * H, yc + (long)b * H, yw + (long)b * H * yt, yt, store);
}

// the tiles of yuv10_to_rgb_u8_kernel for one depth: yuv420_to_rgb_u8_kernel's (yuv.hip) loop
template <int DEPTH>
__device__ __forceinline__ void to_rgb_tiles(const vtx_yuv10_clip& d, int Ts, int Hs, int Ws, uint8_t* __restrict__ dst) {
  typedef typename Contract<DEPTH>::Sample S;
  const YuvMatrix m = load_matrix<DEPTH>(d.matrix);
  const int chunks = (Ws + 255) / 256;
  const long tiles = (long)Ts * Hs * chunks;
  for (long j = blockIdx.x; j < tiles; j += gridDim.x) {
    const int line = (int)(j / chunks);                  // t * Hs + s
    const int x = (int)(j - (long)line * chunks) * 256 + threadIdx.x;
    if (x >= Ws) continue;
    const int t = line / Hs, s = line - t * Hs;
    const int tc = t > d.Ts - 1 ? d.Ts - 1 : t, sc = s > d.Hs - 1 ? d.Hs - 1 : s, xs = x > d.Ws - 1 ? d.Ws - 1 : x;
    const long c = (long)tc * d.c_frame + (long)(sc >> 1) * d.c_pitch;
    const int cx = (xs >> 1) * d.c_step;
    int R, G, B;
    yuv_to_rgb<DEPTH>(m, Contract<DEPTH>::sample(at<S>(d.y, (long)tc * d.y_frame + (long)sc * d.y_pitch)[xs], d.shift),
                      Contract<DEPTH>::sample(at<S>(d.u, c)[cx], d.shift), Contract<DEPTH>::sample(at<S>(d.v, c)[cx], d.shift), R, G, B);
    uint8_t* o = dst + ((long)line * Ws + x) * 3;
    o[0] = (uint8_t)R; o[1] = (uint8_t)G; o[2] = (uint8_t)B;
  }
}

// dst [Ts,Hs,Ws,3] = rgb(*clip).  One workgroup per (row of a frame, 256 columns) tile, grid-stride over the tiles: the tile's
// frame, row and first column are the same for every thread (scalar divisions).  Reads are clamped into the record's own
// Ts / Hs / Ws, stores bounded by the arguments, which describe dst.
__global__ __launch_bounds__(256) void yuv10_to_rgb_u8_kernel(const vtx_yuv10_clip* __restrict__ clip, int Ts, int Hs, int Ws,
                                                              uint8_t* __restrict__ dst) {
  const vtx_yuv10_clip& d = *clip;
  if (!walkable(d)) return;
  if (d.depth == 8) to_rgb_tiles<8>(d, Ts, Hs, Ws, dst);
  else to_rgb_tiles<10>(d, Ts, Hs, Ws, dst);
}

}  // namespace vtx

using namespace vtx;

extern "C" int vtx_clips_views_yuv10(int B, int T, int H, int V, int W, int Wr_max, const vtx_yuv10_clip* clips, unsigned char* dst,
                                     const int32_t* frames, const int32_t* left, const int32_t* x_first, const int32_t* x_count,
                                     const float* x_weights, int x_taps, const int32_t* y_first, const int32_t* y_count,
                                     const float* y_weights, int y_taps, void* stream) {
  VTX_REQUIRE(B > 0 && T > 0 && H > 0 && V > 0 && W > 0 && Wr_max > 0 && x_taps > 0 && y_taps > 0, VTX_EINVAL,
              "clips_views_yuv10: B=%d T=%d rows %d views %d of width %d widest resized row %d taps %d/%d must all be positive",
              B, T, H, V, W, Wr_max, x_taps, y_taps);
  VTX_REQUIRE(V <= MAX_VIEWS, VTX_EINVAL, "clips_views_yuv10: %d views, at most %d are supported", V, MAX_VIEWS);
  VTX_REQUIRE(W <= Wr_max, VTX_EINVAL, "clips_views_yuv10: a view of %d columns does not fit the widest resized row of %d", W, Wr_max);
  VTX_REQUIRE(clips && dst && left && x_first && x_count && x_weights && y_first && y_count && y_weights, VTX_EINVAL,
              "clips_views_yuv10: null pointer");
  VTX_REQUIRE((reinterpret_cast<uintptr_t>(clips) & 7u) == 0, VTX_EALIGN,
              "clips_views_yuv10: the clip records must be 8-byte aligned (place them first in a packed upload)");
  const long bands = (H + BAND_ROWS - 1) / BAND_ROWS;
  VTX_REQUIRE((long)B * T <= 65535 && bands <= 65535, VTX_EINVAL, "clips_views_yuv10: %ld frames / %ld row bands exceed the grid (65535 each)", (long)B * T, bands);
  dim3 grid((unsigned)((Wr_max + 255) / 256), (unsigned)bands, (unsigned)(B * T));
  hipLaunchKernelGGL(clips_views_yuv10_kernel, grid, dim3(256), 0, as_stream(stream), T, H, V, W, Wr_max, clips, dst, frames, left,
                     x_first, x_count, x_weights, x_taps, y_first, y_count, y_weights, y_taps);
  return check_launch("clips_views_yuv10");
}

extern "C" int vtx_yuv10_to_rgb_u8(const vtx_yuv10_clip* clip, int Ts, int Hs, int Ws, unsigned char* dst, void* stream) {
  VTX_REQUIRE(Ts > 0 && Hs > 0 && Ws > 0, VTX_EINVAL, "yuv10_to_rgb_u8: Ts=%d frames of %dx%d must all be positive", Ts, Hs, Ws);
  VTX_REQUIRE((long)Ts * Hs < (1L << 31), VTX_EINVAL, "yuv10_to_rgb_u8: %ld rows exceed 2^31", (long)Ts * Hs);
  VTX_REQUIRE(clip && dst, VTX_EINVAL, "yuv10_to_rgb_u8: null pointer");
  VTX_REQUIRE((reinterpret_cast<uintptr_t>(clip) & 7u) == 0, VTX_EALIGN, "yuv10_to_rgb_u8: the clip record must be 8-byte aligned");
  const long tiles = (long)Ts * Hs * ((Ws + 255) / 256);
  hipLaunchKernelGGL(yuv10_to_rgb_u8_kernel, dim3(grid_for(tiles * 256, 16384)), dim3(256), 0, as_stream(stream), clip, Ts, Hs, Ws, dst);
  return check_launch("yuv10_to_rgb_u8");
}
