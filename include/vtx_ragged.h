/* vtx_ragged.h -- C ABI of libvtx_ragged.so: views of decoded uint8 clips that differ in source size, for the MI355X (gfx950).
 *
 * The seventh library, next to libvtx.so (include/vtx.h), libvtx_aug.so (include/vtx_aug.h), libvtx_randaug.so
 * (include/vtx_randaug.h), libvtx_views.so (include/vtx_views.h), libvtx_mix.so (include/vtx_mix.h) and libvtx_stem.so
 * (include/vtx_stem.h), built by the same csrc/build.py from csrc/ragged.hip: those six keep their export lists and
 * versions.  Conventions as in vtx.h: extern "C", plain pointers, device pointers borrowed for the call, nothing
 * allocated, work enqueued on `stream` (a hipStream_t passed as void*) of the current device, VTX_OK or a negative VTX_E*
 * code (the codes of vtx.h), never throws; vtx_ragged_last_error_string() gives the reason of the last failure on the
 * calling thread.  Python binds it with ctypes (vtx/_lib.py: RAGGED_SIGNATURES).
 */
#ifndef VTX_RAGGED_H_
#define VTX_RAGGED_H_

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

int vtx_ragged_version(void);                    /* 100 = 0.1.0 */
const char* vtx_ragged_last_error_string(void);

/* vtx_clip_views_u8 (include/vtx_views.h) for a batch whose clips differ in decoded length and frame size -- what a loader
 * yields that collates decoded videos as they are (340x256, 256x340, 320x240, ... all occur in Kinetics) -- in one launch:
 *
 *   dst[b,v,t] = columns left[b,v] .. left[b,v] + W  of  round_half_even(clamp(Wy[b] * src[b][frames[b,t]] * Wx[b]^T, 0, 255))
 *
 * src: a DEVICE table of B device pointers, src[b] the base of clip b, uint8 [Ts_b,Hs_b,Ws_b,3] contiguous (channels last).
 * The table is read as 8-byte pointers, so `src` itself must be 8-byte aligned (VTX_EALIGN otherwise): a caller that packs
 * it into one upload with the int32 tables below places it FIRST in that buffer.  geom [B,4] int32 (device): Ts_b, Hs_b,
 * Ws_b and Wr_b, the columns of clip b's resized frame, W <= Wr_b <= Wr_max.  dst [B,V,T,H,W,3], 1 <= V <= 8: the output is
 * uniform.  frames [B,T] int32: indices into the Ts_b frames of the row's own clip; NULL = frames 0 .. T-1 of every clip (the
 * caller then requires Ts_b == T for all b).  left [B,V] int32: the first column of each view in clip b's resized row of
 * Wr_b columns, as vtx_clip_views_u8's.  Tables as vtx_clip_views_u8's, with ONE row stride for all clips: x_first / x_count
 * [B,Wr_max] and x_weights [B,Wr_max,x_taps], row b valid for x < Wr_b (what lies behind is never read); y_first / y_count
 * [B,H] and y_weights [B,H,y_taps].  x_taps / y_taps: the widest window of any clip.
 *
 * Arithmetic: vtx_clip_views_u8's, the same device code (x pass, then y pass, taps in ascending order, float32 without
 * contraction, clamp to [0, 255], round half-to-even): clip b's views are byte for byte that call on clip b alone with its
 * rows of the tables.  With V = 1, left = 0 and Wr_b = W it is vtx_clip_resample_u8 on the gathered frames.
 *
 * Checked here, on the host, before the launch: positive sizes, V <= 8, W <= Wr_max, B * T <= 65535 (the grid is
 * (ceil(Wr_max / 256), ceil(H / 8), B * T); a column tile beyond a clip's Wr_b, or in none of its windows, returns before
 * any load), no null pointer but `frames`, the alignment of `src`.  geom lives on the device and is NOT read on the host:
 * whoever fills it validates Wr_b, the pointers and their extents (vtx.ops.clips_views_u8 does).  On the device every index
 * is clamped with the clip's own numbers whatever the arrays say -- frame index into [0, Ts_b), tap windows into Ws_b / Hs_b,
 * lefts into [0, Wr_b - W], Wr_b to at most Wr_max -- and a clip whose Ts_b, Hs_b, Ws_b is not positive or whose Wr_b < W is
 * skipped; a wrong POINTER cannot be caught there. */
int vtx_clips_views_u8(int B, int T, int H, int V, int W, int Wr_max, const void* const* src, const int32_t* geom,
                       unsigned char* dst, const int32_t* frames, const int32_t* left, const int32_t* x_first,
                       const int32_t* x_count, const float* x_weights, int x_taps, const int32_t* y_first,
                       const int32_t* y_count, const float* y_weights, int y_taps, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VTX_RAGGED_H_ */
