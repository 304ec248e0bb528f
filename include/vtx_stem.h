/* vtx_stem.h -- C ABI of libvtx_stem.so: MaskFeat's input path from decoded uint8 clips for the MI355X (gfx950).
 *
 * The sixth library, next to libvtx.so (include/vtx.h), libvtx_aug.so (include/vtx_aug.h), libvtx_randaug.so
 * (include/vtx_randaug.h), libvtx_views.so (include/vtx_views.h) and libvtx_mix.so (include/vtx_mix.h), built by the same
 * csrc/build.py from csrc/stem.hip: those five keep their export lists and versions.  Conventions as in vtx.h: extern "C",
 * plain pointers, device pointers borrowed for the call, nothing allocated, work enqueued on `stream` (a hipStream_t
 * passed as void*) of the current device, VTX_OK or a negative VTX_E* code (the codes of vtx.h), never throws; every
 * argument is checked before anything is launched, and vtx_stem_last_error_string() gives the reason of the last failure on
 * the calling thread.  Python binds it with ctypes (vtx/_lib.py: STEM_SIGNATURES).
 *
 * The float forms are vtx_im2col3d and vtx_hog_fwd of vtx.h.
 */
#ifndef VTX_STEM_H_
#define VTX_STEM_H_

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

int vtx_stem_version(void);                       /* 100 = 0.1.0 */
const char* vtx_stem_last_error_string(void);

/* The rows of vtx_im2col3d (vtx.h) straight from decoded video: the im2col of the MViT stem's overlapping, padded Conv3d
 * (create_conv_patch_embed, video_transformer.py:585-618, 834-843) behind ToTensor (data_transform.py:52-63) and
 * Normalize (data_transform.py:534-539), without the float clip ever being stored.
 *
 *   clip uint8 [B,T,H,W,3] (channels last) -> rows [B*To*Ho*Wo][Kp] of dtype (VTX_F32 / VTX_BF16)
 *   row (b,to,ho,wo), column k -> (c,kt,kh,kw) in weight order; k3 / s3 / p3 = HOST (t,h,w) kernel / stride / padding triples,
 *   To = (T + 2 pt - kt) / st + 1 and so on; host_mean3 / host_std3: three host floats each, read during the call.
 *
 *   an in-bounds tap   n(v,c) = ((float)v / 255.0f - mean[c]) / std[c]     three float32 operations, each rounded on its
 *                      own, no contraction: vtx_patch_rows_u8's normalisation (the kernel reads it from a 3 x 256 table a
 *                      workgroup computes with exactly these operations)
 *   a padding tap      (t, h or w outside the clip) +0.0f, NOT n(0,c): the reference pads the normalised tensor
 *   columns 3*kt*kh*kw .. Kp-1   +0.0f
 *
 * so with VTX_F32 the rows equal vtx_im2col3d of the normalised float clip [B,T,3,H,W] bit for bit, and with VTX_BF16 they
 * are that value rounded once, as vtx_im2col3d rounds.  Kp >= 3*kt*kh*kw and a multiple of 8 (one 16-byte bf16 store per
 * thread).  The clip needs NO alignment (taps are single byte loads: rows of 3*W bytes carry none for odd W); rows must be
 * 16-byte aligned (VTX_EALIGN).  VTX_EINVAL: a null pointer, a zero std, a non-positive size / kernel / stride, a negative
 * padding, Kp too small or no multiple of 8, an empty output grid (the padded clip smaller than the kernel), B*T*H*W*3 or
 * B*To*Ho*Wo*Kp/8 at or beyond 2^31 (32-bit index arithmetic).  Per MaskFeat clip (16 x 224^2, kernel (3,7,7), stride
 * (2,4,4), padding (1,3,3), Kp 448, bf16): 2.4 MB read, 22.5 MB written. */
int vtx_im2col3d_u8(int dtype, int B, int T, int H, int W, const int* k3, const int* s3, const int* p3, int Kp,
                    const unsigned char* clip, const float* host_mean3, const float* host_std3, void* rows, void* stream);

/* HOG targets of selected frames of a clip batch (the reference extracts them on CPU workers for the centre frame of every
 * masked cube only, dataset.py:188-196; extract_hog_features, dataset.py:39-45): frames uint8 [F,H,W,3] are ALL frames of
 * the batch (F = B*T), sel a DEVICE array of n > 0 flat frame indices in 0 .. F-1.  Frame sel[i] is read and its
 * [H/16, W/16, 108] float64 block written to row sel[i] of out [F, H/16, W/16, 108]; rows not selected are not touched (the
 * caller zeroes out), an index outside 0 .. F-1 is skipped.  One launch for the batch; the kernel, and so every bit, is
 * vtx_hog_fwd's (vtx.h; csrc/hog_kernel.h).  table / table_bytes: the blob of vtx_hog_build_table (vtx.h) on the device.
 * H and W multiples of 16, W <= 1024; frames and out 16-byte aligned, sel 4-byte aligned (VTX_EALIGN); an empty selection
 * (n <= 0) is VTX_EINVAL: there is nothing to launch. */
int vtx_hog_fwd_sel(const unsigned char* frames, int F, int H, int W, const int* sel, int n, const double* table,
                    size_t table_bytes, double* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VTX_STEM_H_ */
