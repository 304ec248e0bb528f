/* vtx_dropout.h -- C ABI of libvtx_dropout.so: dropout without a stored mask for the MI355X (gfx950).
 *
 * The eighth library, next to libvtx.so (include/vtx.h) and the six input-path libraries, built by the same csrc/build.py
 * from csrc/dropout.hip: those seven keep their export lists and versions.  Conventions as in vtx.h, whose row maps
 * (vtx_rowmap), dtypes and error codes it uses: extern "C", plain pointers, device pointers borrowed for the call, nothing
 * allocated, work enqueued on `stream` (a hipStream_t passed as void*) of the current device, VTX_OK or a negative VTX_E* code,
 * never throws; every argument is checked before anything is launched, and vtx_dropout_last_error_string() gives the reason
 * of the last failure on the calling thread.  Python binds it with ctypes (vtx/_lib.py: DROPOUT_SIGNATURES).
 */
#ifndef VTX_DROPOUT_H_
#define VTX_DROPOUT_H_

#include "vtx.h"

#ifdef __cplusplus
extern "C" {
#endif

int vtx_dropout_version(void);                    /* 100 = 0.1.0 */
const char* vtx_dropout_last_error_string(void);

/* nn.Dropout of Attention.proj_drop (reference transformer.py:176), of the pre-norm attention operators (:265 and its twins),
 * of the FFN (:498-507) and of drop_after_pos / drop_after_time (video_transformer.py:212,238,474,500,523).  For rows x D
 * elements, dtype VTX_F32 or VTX_BF16:
 *
 *     y[ymap(m), c] = post[pmap(m), c] + s(m) * drop_e(x[xmap(m), c] + pre[m % pre_period, c])
 *
 * The mask is a pure function of (seed, site, element index, p).  It is never stored: the backward pass is the same launch on
 * the gradient.
 *   Generator   Philox4x32-10 with the standard constants: multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9
 *               and 0xBB67AE85; key = (seed & 0xffffffff, seed >> 32).
 *   Element     e = e0 + m * D + c as a 64-bit integer; m the LOGICAL row (before any row map), c the column.
 *               Counter = (lo32(e >> 2), hi32(e >> 2), site, 0); the element takes output word e & 3.
 *   Threshold   dropped iff (uint64)word < thr, thr = floor(p * 2^32) in [0, 2^32], computed by the caller in integers.
 *   Scale       scale = float32(1) / float32(1 - p); the caller passes 0 for p == 1.
 *   Value       all float32, in this order, no fma contraction, ONE rounding (the store):
 *               t = float(x) [+ pre];  t = kept ? t * scale : +0.0;  t = t * s(m) if s;  t = t + post if post.
 * post (optional): the residual, same dtype as x.  pre (optional): a float32 [pre_period, D] table (the time embedding).
 * s (optional): the DropPath row scale s[(m / rs_d1) * rs_m1 + (m % rs_d2) * rs_m2], as in vtx_row_scale_copy.  y may alias x
 * when xmap and ymap and the leading dimensions agree (a thread reads its 8 elements before it writes them).
 * D % 8 == 0 and e0 % 4 == 0 are required: four consecutive columns share one Philox evaluation and every access is 16 bytes
 * wide.  Anything else, a null x or y and non-positive sizes return VTX_EINVAL before any launch; pointers that are not 16-byte
 * aligned and leading dimensions that are no multiple of 8 return VTX_EALIGN.  All index arithmetic is 64-bit.  The grid is
 * capped at 4096 workgroups of 256 threads x 8 elements (8 388 608 elements per trip); larger launches stride. */
int vtx_dropout_rows(int dtype, int rows, int D, const void* x, long ldx, vtx_rowmap xmap, void* y, long ldy, vtx_rowmap ymap,
                     const void* post, long ldp, vtx_rowmap pmap, const float* pre, int pre_period,
                     const float* s, int rs_d1, int rs_m1, int rs_d2, int rs_m2, unsigned long long thr, float scale,
                     unsigned long long seed, unsigned int site, unsigned long long e0, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VTX_DROPOUT_H_ */
