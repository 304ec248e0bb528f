/* vtx_views.h -- C ABI of libvtx_views.so: test-time views of decoded uint8 clips for the MI355X (gfx950).
 *
 * The fourth library, next to libvtx.so (include/vtx.h), libvtx_aug.so (include/vtx_aug.h) and libvtx_randaug.so
 * (include/vtx_randaug.h), built by the same csrc/build.py from csrc/views.hip: those three keep their export lists and
 * versions.  Conventions as in vtx.h: extern "C", plain pointers, device pointers borrowed for the call, nothing
 * allocated, work enqueued on `stream` (a hipStream_t passed as void*) of the current device, VTX_OK or a negative VTX_E*
 * code (the codes of vtx.h), never throws; vtx_views_last_error_string() gives the reason of the last failure on the
 * calling thread.  Python binds it with ctypes (vtx/_lib.py: VIEWS_SIGNATURES).
 */
#ifndef VTX_VIEWS_H_
#define VTX_VIEWS_H_

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

int vtx_views_version(void);                     /* 100 = 0.1.0 */
const char* vtx_views_last_error_string(void);

/* Frame selection + Resize + the crops of ThreeCrop (the test pipeline of data_trainer.py:108-121 in front of ToTensor +
 * Normalize, and the frame gather of dataset.py:160-162) in one launch, on decoded uint8 clips (channels last):
 *
 *   dst[b,v,t] = columns left[b,v] .. left[b,v] + W  of  round_half_even(clamp(Wy[b] * src[b, frames[b,t]] * Wx[b]^T, 0, 255))
 *
 * src [B,Ts,Hs,Ws,3] -> dst [B,V,T,H,W,3], 1 <= V <= 8, W <= Wr.  frames [B,T] int32: indices into Ts; NULL = every frame
 * in order (needs T == Ts).  left [B,V] int32: the first column of each view in the resized row of Wr columns; views may
 * overlap, coincide or leave columns out -- a column is resampled once and stored to every view that holds it, a column in
 * no view is not computed.  Tables as vtx_clip_resample_u8's (vtx_resample_build_table of libvtx_aug.so), per clip:
 * x_first / x_count [B,Wr] int32 and x_weights [B,Wr,x_taps] float32 for ALL Wr columns of the resized frame; y_first /
 * y_count [B,H] and y_weights [B,H,y_taps] for the H output rows (the caller cuts the resized frame's table to the crop
 * window).  Arithmetic: vtx_clip_resample_u8's, the same device code (x pass, then y pass, float32 without
 * contraction), so each view equals that call on the gathered frames, sliced.  Only the first count taps of an output are
 * read; frame indices, lefts and tap windows are clamped into range on the device whatever the arrays say (validate them
 * on the host).  No alignment requirement. */
int vtx_clip_views_u8(int B, int Ts, int T, int Hs, int Ws, int H, int Wr, int V, int W, const unsigned char* src,
                      unsigned char* dst, const int32_t* frames, const int32_t* left, const int32_t* x_first,
                      const int32_t* x_count, const float* x_weights, int x_taps, const int32_t* y_first,
                      const int32_t* y_count, const float* y_weights, int y_taps, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VTX_VIEWS_H_ */
