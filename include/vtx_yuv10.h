/* vtx_yuv10.h -- C ABI of libvtx_yuv10.so: decoded 10-bit 4:2:0 YUV clips (P010, yuv420p10le), alone or mixed with 8-bit ones
 * (NV12, I420), into the clip resampler, for the MI355X (gfx950).
 *
 * The tenth library, next to libvtx.so (include/vtx.h), libvtx_aug.so (include/vtx_aug.h), libvtx_randaug.so
 * (include/vtx_randaug.h), libvtx_views.so (include/vtx_views.h), libvtx_mix.so (include/vtx_mix.h), libvtx_stem.so
 * (include/vtx_stem.h), libvtx_ragged.so (include/vtx_ragged.h), libvtx_dropout.so (include/vtx_dropout.h) and libvtx_yuv.so
 * (include/vtx_yuv.h), built by the same csrc/build.py from csrc/yuv10.hip: those nine keep their export lists and versions.
 * Conventions as in vtx.h: extern "C", plain pointers, device pointers borrowed for the call, nothing allocated, work enqueued
 * on `stream` (a hipStream_t passed as void*) of the current device, VTX_OK or a negative VTX_E* code (the codes of vtx.h),
 * never throws; vtx_yuv10_last_error_string() gives the reason of the last failure on the calling thread.  Python binds it
 * with ctypes (vtx/_lib.py: YUV10_SIGNATURES).
 *
 * THE LAYOUTS
 *
 * Geometry as in vtx_yuv.h: luma Y[Ts,Hs,Ws], chroma of Hc = (Hs + 1) / 2 rows by Wc = (Ws + 1) / 2 columns, the chroma sample
 * of pixel (s, x) is (s >> 1, x >> 1) (nearest siting).  A sample is one byte (depth 8) or one little-endian 16-bit word
 * (depth 10); the word is moved right by `shift` bits and masked to its lower `depth` bits, so whatever else the word holds
 * does not reach the result:
 *
 *   I420         depth 8,  bytes,                              planar U, V:        c_step 1, shift 0
 *   NV12         depth 8,  bytes,                              interleaved UV:     c_step 2, shift 0, v = u + 1 byte
 *   yuv420p10le  depth 10, the sample in the LOWER 10 bits,    planar U, V:        c_step 1, shift 0
 *   P010         depth 10, the sample in the UPPER 10 bits,    interleaved UV:     c_step 2, shift 6, v = u + 2 bytes
 *
 * (any of the two 10-bit alignments goes with any of the two chroma layouts: shift and c_step are independent).  Pitches
 * and frame strides are BYTES, c_step is SAMPLES: the chroma pair of pixel (t, s, x) is the sample at byte offset
 * t * c_frame + (s >> 1) * c_pitch + (x >> 1) * c_step * size from u and from v, its luma the sample at byte offset
 * t * y_frame + s * y_pitch + x * size from y, size = 1 or 2 bytes.  y_pitch >= Ws * size, c_pitch >= Wc * c_step * size,
 * frame strides >= 0; with 16-bit samples the three plane addresses, pitches and frame strides are even.
 *
 * THE 10-BIT CONVERSION CONTRACT
 *
 * One matrix of six int32 {y_off, c_y, c_rv, c_gu, c_gv, c_bu} per clip, with 12 fractional bits, applied to the 10-bit samples
 * directly.  With Y, U, V in [0, 1023], C = (Y - y_off) * c_y + 2048, D = U - 512, E = V - 512:
 *
 *   R = clamp((C + c_rv * E) >> 12, 0, 255)
 *   G = clamp((C - c_gu * D - c_gv * E) >> 12, 0, 255)
 *   B = clamp((C + c_bu * D) >> 12, 0, 255)
 *
 * in int32 arithmetic with an arithmetic shift (floor, also for negative sums).  0 <= y_off <= 1023 and |c| <= 16384 for the
 * five coefficients, so no sum leaves +-2^26.  The usual matrices (vtx.YUVClip's presets at depth 10), floor(4096 * k + 0.5) of
 * the float64 matrix (vtx.ops.yuv10_matrix) -- limited range: luma 64 .. 940 scaled by 255 / 876, chroma by 255 / 896; full
 * range: 255 / 1023 for both --:
 *
 *                          y_off   c_y  c_rv  c_gu  c_gv  c_bu
 *   BT.601 limited range      64  1192  1634   401   832  2066
 *   BT.709 limited range      64  1192  1836   218   546  2163
 *   BT.601 full range          0  1021  1431   351   729  1809
 *   BT.709 full range          0  1021  1608   191   478  1895
 *
 * Each is within one step of its float64 matrix rounded once, over 2^24 random triples and a grid that holds the range ends
 * (tests/yuv10_ref.py: sample_set; tests/test_yuv10_host.py).  A record of depth 8 is converted by the contract of vtx_yuv.h
 * -- centre 128, + 128, >> 8, 0 <= y_off <= 255, |c| <= 4096 --: the same arithmetic path with other constants, the bytes
 * those of libvtx_yuv.so.  The two contracts meet in one identity: a 10-bit clip whose samples are 4 x an 8-bit clip's, with
 * the matrix (4 * y_off, 4 * c ...), converts to exactly the 8-bit clip's RGB.
 *
 * NOT built: 12-bit and deeper; 4:2:2 / 4:4:4 (P210, P410, ...); chroma sitings other than nearest; transfer functions and tone
 * mapping -- PQ / HLG content is matrixed, not tone-mapped, BT.2020's luma weights go in as six integers --; byte parity with
 * the RGB output of any particular decoder or of swscale.
 */
#ifndef VTX_YUV10_H_
#define VTX_YUV10_H_

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

/* One clip of either depth as the kernels read it from DEVICE memory: 96 bytes, 8-byte aligned (the pointers come first),
 * 24 int32 for a caller that packs it into an int32 upload (pointers as little-endian pairs). */
typedef struct vtx_yuv10_clip {
  const void* y;            /* luma plane                                                             */
  const void* u;            /* planar: the U plane;  interleaved: the UV plane                        */
  const void* v;            /* planar: the V plane;  interleaved: u + one sample                      */
  int32_t Ts, Hs, Ws;       /* frames, rows and columns of the luma                                   */
  int32_t Wr;               /* vtx_clips_views_yuv10: columns of the clip's resized row; else 0       */
  int32_t y_pitch, y_frame; /* BYTES from row to row and from frame to frame of the luma              */
  int32_t c_pitch, c_frame; /* likewise of the chroma plane(s)                                        */
  int32_t c_step;           /* SAMPLES from chroma column to chroma column: 1 planar, 2 interleaved   */
  int32_t depth;            /* 8: one byte per sample;  10: one 16-bit word per sample                */
  int32_t shift;            /* bits a loaded word is moved right before masking to `depth` bits: 6 (P010) or 0; 0 at depth 8 */
  int32_t matrix[6];        /* y_off, c_y, c_rv, c_gu, c_gv, c_bu, of the contract of its depth       */
  int32_t reserved;         /* 0                                                                      */
} vtx_yuv10_clip;

int vtx_yuv10_version(void);                    /* 100 = 0.1.0 */
const char* vtx_yuv10_last_error_string(void);

/* vtx_clips_views_yuv420 (include/vtx_yuv.h) on records of either depth, so a batch that mixes 8-bit and 10-bit clips is ONE
 * launch: the same tables, `frames`, `left`, views, grid and device-side clamping, the source of clip b is clips[b], a DEVICE
 * array of B records (8-byte aligned, VTX_EALIGN otherwise: a caller that packs it into one upload with the int32 tables
 * places it FIRST in that buffer):
 *
 *   dst[b,v,t] = columns left[b,v] .. left[b,v] + W  of  round_half_even(clamp(Wy[b] * rgb(clips[b])[frames[b,t]] * Wx[b]^T, 0, 255))
 *
 * where rgb() is the conversion of the record's depth.  Each tap's R, G, B is formed in registers from one luma sample and
 * its chroma pair and handed to the same device text as vtx_clips_views_u8 (csrc/resample_band.h), so the result is byte for
 * byte vtx_clips_views_u8 on the clips vtx_yuv10_to_rgb_u8 writes, and those RGB clips never exist.  dst [B,V,T,H,W,3],
 * 1 <= V <= 8.
 *
 * Checked here, on the host, before the launch: positive sizes, V <= 8, W <= Wr_max, B * T <= 65535 (the grid is
 * (ceil(Wr_max / 256), ceil(H / 8), B * T)), no null pointer but `frames`, the alignment of `clips`.  The records live on the
 * device and are NOT read on the host: whoever fills them validates sizes, pitches, the matrix, the pointers and their
 * extents (vtx.YUVClip and vtx.ops.clips_views_yuv do).  On the device every index is clamped with the clip's own numbers
 * whatever the arrays say -- frame index into [0, Ts), tap windows into Ws / Hs, lefts into [0, Wr - W], Wr to at most Wr_max,
 * y_off and the coefficients into the bounds of the record's depth -- and a clip whose Ts, Hs, Ws is not positive, whose
 * Wr < W, whose c_step is neither 1 nor 2, whose pitch is shorter than its row, whose frame stride is negative, whose depth
 * is neither 8 nor 10, whose shift is neither 0 nor 6 (depth 8: not 0), or, with 16-bit samples, whose pitch, frame stride
 * or plane address is odd, is skipped; any other wrong POINTER cannot be caught there. */
int vtx_clips_views_yuv10(int B, int T, int H, int V, int W, int Wr_max, const vtx_yuv10_clip* clips, unsigned char* dst,
                          const int32_t* frames, const int32_t* left, const int32_t* x_first, const int32_t* x_count,
                          const float* x_weights, int x_taps, const int32_t* y_first, const int32_t* y_count,
                          const float* y_weights, int y_taps, void* stream);

/* The plain conversion of one clip: dst uint8 [Ts,Hs,Ws,3] contiguous = rgb(*clip), for callers that want the RGB frames.
 * clip: ONE record in device memory, 8-byte aligned; Ts, Hs, Ws: the shape of dst, equal to the record's (a pixel beyond the
 * record's own Ts / Hs / Ws reads the clamped index; a record the views kernel would skip writes nothing).  A grid-stride
 * kernel over (row, 256 columns) tiles.  Checked here: positive sizes, Ts * Hs < 2^31, no null pointer, the alignment. */
int vtx_yuv10_to_rgb_u8(const vtx_yuv10_clip* clip, int Ts, int Hs, int Ws, unsigned char* dst, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VTX_YUV10_H_ */
