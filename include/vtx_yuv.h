/* vtx_yuv.h -- C ABI of libvtx_yuv.so: decoded 4:2:0 YUV clips (NV12, I420) into the clip resampler, for the MI355X (gfx950).
 *
 * The ninth library, next to libvtx.so (include/vtx.h), libvtx_aug.so (include/vtx_aug.h), libvtx_randaug.so
 * (include/vtx_randaug.h), libvtx_views.so (include/vtx_views.h), libvtx_mix.so (include/vtx_mix.h), libvtx_stem.so
 * (include/vtx_stem.h), libvtx_ragged.so (include/vtx_ragged.h) and libvtx_dropout.so (include/vtx_dropout.h), built by the
 * same csrc/build.py from csrc/yuv.hip: those eight keep their export lists and versions.  Conventions as in vtx.h:
 * extern "C", plain pointers, device pointers borrowed for the call, nothing allocated, work enqueued on `stream` (a
 * hipStream_t passed as void*) of the current device, VTX_OK or a negative VTX_E* code (the codes of vtx.h), never throws;
 * vtx_yuv_last_error_string() gives the reason of the last failure on the calling thread.  Python binds it with ctypes
 * (vtx/_lib.py: YUV_SIGNATURES).
 *
 * THE CONVERSION CONTRACT
 *
 * A 4:2:0 clip of Ts frames of Hs x Ws pixels is a luma plane Y[Ts,Hs,Ws] and chroma of Hc = (Hs + 1) / 2 rows by
 * Wc = (Ws + 1) / 2 columns (integer division: odd sizes are allowed, the last chroma row / column then serves one luma row /
 * column).  The chroma sample of pixel (s, x) is (s >> 1, x >> 1): nearest siting, what an unscaled swscale conversion and
 * most GPU converters use.  Two layouts:
 *
 *   I420   separate planes U[Ts,Hc,Wc] and V[Ts,Hc,Wc]:  c_step 1, u and v their bases
 *   NV12   one interleaved plane UV[Ts,Hc,Wc,2]:         c_step 2, u its base and v = u + 1
 *
 * so the chroma pair of pixel (t, s, x) is u[t * c_frame + (s >> 1) * c_pitch + (x >> 1) * c_step] and the byte at the same
 * offset from v, and its luma y[t * y_frame + s * y_pitch + x].  Row pitches and frame strides (bytes) are free -- decoders
 * pad their line sizes --: y_pitch >= Ws, c_pitch >= Wc * c_step, frame strides >= 0.
 *
 * One matrix of six int32 {y_off, c_y, c_rv, c_gu, c_gv, c_bu} per clip.  With C = (Y - y_off) * c_y, D = U - 128, E = V - 128:
 *
 *   R = clamp(floor((C + c_rv * E + 128) / 256), 0, 255)
 *   G = clamp(floor((C - c_gu * D - c_gv * E + 128) / 256), 0, 255)
 *   B = clamp(floor((C + c_bu * D + 128) / 256), 0, 255)
 *
 * in int32 arithmetic; the division is an arithmetic shift by 8: floor, also for negative sums.  0 <= y_off <= 255 and
 * |c| <= 4096 for the five coefficients, so no sum leaves +-2^22.  The usual matrices (vtx.YUVClip's presets):
 *
 *                          y_off  c_y  c_rv  c_gu  c_gv  c_bu
 *   BT.601 limited range      16  298   409   100   208   516     (what swscale assumes for an untagged stream)
 *   BT.709 limited range      16  298   459    55   136   541
 *   BT.601 full range          0  256   359    88   183   454
 *   BT.709 full range          0  256   403    48   120   475
 *
 * Each is within one step, over all 2^24 (Y, U, V), of its float64 matrix rounded once (tests/test_yuv_host.py).  Byte parity
 * with the RGB output of a particular decoder or of swscale is NOT claimed: those differ among themselves in chroma
 * upsampling, rounding and dither.
 */
#ifndef VTX_YUV_H_
#define VTX_YUV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef VTX_OK
#define VTX_OK 0
#define VTX_EINVAL (-1)   /* bad shape / null pointer / unsupported combination */
#define VTX_EALIGN (-2)   /* pointer not aligned as required                   */
#define VTX_ELAUNCH (-3)  /* hipGetLastError() after launch != hipSuccess      */
#define VTX_EWS (-4)      /* workspace too small                               */
#endif

/* One clip as the kernels read it from DEVICE memory: 88 bytes, 8-byte aligned (the pointers come first), 22 int32 for a
 * caller that packs it into an int32 upload (pointers as little-endian pairs). */
typedef struct vtx_yuv420_clip {
  const unsigned char* y;  /* luma plane                                                        */
  const unsigned char* u;  /* I420: the U plane;  NV12: the UV plane                            */
  const unsigned char* v;  /* I420: the V plane;  NV12: u + 1                                   */
  int32_t Ts, Hs, Ws;      /* frames, rows and columns of the luma                              */
  int32_t Wr;              /* vtx_clips_views_yuv420: columns of the clip's resized row; else 0 */
  int32_t y_pitch, y_frame; /* bytes from row to row and from frame to frame of the luma        */
  int32_t c_pitch, c_frame; /* likewise of the chroma plane(s)                                  */
  int32_t c_step;          /* bytes from chroma column to chroma column: 1 (I420) or 2 (NV12)   */
  int32_t matrix[6];       /* y_off, c_y, c_rv, c_gu, c_gv, c_bu                                */
  int32_t reserved;        /* 0                                                                 */
} vtx_yuv420_clip;

int vtx_yuv_version(void);                    /* 100 = 0.1.0 */
const char* vtx_yuv_last_error_string(void);

/* vtx_clips_views_u8 (include/vtx_ragged.h) on 4:2:0 clips: the same tables, `frames`, `left`, views, grid and device-side
 * clamping, and the source of clip b is clips[b], a DEVICE array of B records (8-byte aligned, VTX_EALIGN otherwise: a caller
 * that packs it into one upload with the int32 tables places it FIRST in that buffer):
 *
 *   dst[b,v,t] = columns left[b,v] .. left[b,v] + W  of  round_half_even(clamp(Wy[b] * rgb(clips[b])[frames[b,t]] * Wx[b]^T, 0, 255))
 *
 * where rgb() is the conversion above.  The x pass forms each tap's R, G, B from one luma byte and its chroma pair in
 * registers and goes on as vtx_clips_views_u8 does -- the same device text (csrc/resample_band.h): x pass, then y pass, taps
 * in ascending order, float32 without contraction, clamp to [0, 255], round half-to-even -- so the result is byte for byte
 * vtx_clips_views_u8 on the clips vtx_yuv420_to_rgb_u8 writes, and those RGB clips never exist.  dst [B,V,T,H,W,3], 1 <= V <= 8.
 *
 * Checked here, on the host, before the launch: positive sizes, V <= 8, W <= Wr_max, B * T <= 65535 (the grid is
 * (ceil(Wr_max / 256), ceil(H / 8), B * T)), no null pointer but `frames`, the alignment of `clips`.  The records live on the
 * device and are NOT read on the host: whoever fills them validates sizes, pitches, the matrix, the pointers and their
 * extents (vtx.YUVClip and vtx.ops.clips_views_yuv do).  On the device every index is clamped with the clip's own numbers
 * whatever the arrays say -- frame index into [0, Ts), tap windows into Ws / Hs, lefts into [0, Wr - W], Wr to at most Wr_max,
 * y_off into [0, 255], the coefficients into [-4096, 4096] -- and a clip whose Ts, Hs, Ws is not positive, whose Wr < W, whose
 * c_step is neither 1 nor 2, whose pitch is shorter than its row or whose frame stride is negative is skipped; a wrong
 * POINTER cannot be caught there. */
int vtx_clips_views_yuv420(int B, int T, int H, int V, int W, int Wr_max, const vtx_yuv420_clip* clips, unsigned char* dst,
                           const int32_t* frames, const int32_t* left, const int32_t* x_first, const int32_t* x_count,
                           const float* x_weights, int x_taps, const int32_t* y_first, const int32_t* y_count,
                           const float* y_weights, int y_taps, void* stream);

/* The plain conversion of one clip: dst uint8 [Ts,Hs,Ws,3] contiguous = rgb(*clip), for callers that want the RGB frames.
 * clip: ONE record in device memory, 8-byte aligned; Ts, Hs, Ws: the shape of dst, equal to the record's (a pixel beyond the
 * record's own Ts / Hs / Ws reads the clamped index; a record the views kernel would skip writes nothing).  A grid-stride
 * kernel over (row, 256 columns) tiles.  Checked here: positive sizes, Ts * Hs < 2^31, no null pointer, the alignment. */
int vtx_yuv420_to_rgb_u8(const vtx_yuv420_clip* clip, int Ts, int Hs, int Ws, unsigned char* dst, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VTX_YUV_H_ */
