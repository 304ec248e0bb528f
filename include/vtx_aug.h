/* vtx_aug.h -- C ABI of libvtx_aug.so: clip augmentation on decoded uint8 frames for the MI355X (gfx950).
 *
 * A library of its own next to libvtx.so (include/vtx.h), built by the same csrc/build.py from csrc/aug.hip: the
 * augmentation sits in front of the model, shares no state with the training path, and libvtx.so's export list and
 * version stay what its users pin.  Conventions as in vtx.h: extern "C", plain pointers, device pointers borrowed for
 * the call, nothing allocated, work enqueued on `stream` (a hipStream_t passed as void*) of the current device,
 * VTX_OK or a negative VTX_E* code (the codes of vtx.h), never throws; vtx_aug_last_error_string() gives the reason
 * of the last failure on the calling thread.  Python binds it with ctypes (vtx/_lib.py: AUG_SIGNATURES).
 */
#ifndef VTX_AUG_H_
#define VTX_AUG_H_

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

int vtx_aug_version(void);                       /* 100 = 0.1.0 */
const char* vtx_aug_last_error_string(void);

/* The steps of transforms_train (data_transform.py:495-531) that precede ToTensor + Normalize, on decoded uint8 clips
 * [B,T,H,W,3] (channels last) on the device: RandomResizedCrop + RandomHorizontalFlip (vtx_clip_resample_u8) and
 * ColorJitter without hue (vtx_clip_jitter_u8); with other tables the resampler is the Resize + CenterCrop of
 * transforms_eval (data_transform.py:546-566).  The random draws stay with the caller (vtx/aug.py).
 *
 * vtx_resample_build_table: HOST ONLY, no device call.  Weights of torch.nn.functional.interpolate(align_corners=False)
 * along one axis for the crop [crop_start, crop_start + crop_len) of a source of src_len samples resampled to out_len
 * samples (what torchvision's resized_crop computes: borders clamp at the crop).  Per output index o: first[o] = first
 * source index (of the uncropped source), count[o] = number of taps, weights[o * max_taps + k], k < count[o]; entries
 * behind count[o] are left as they are.  Computed in float64, rounded once.  antialias = 0: 2 taps (bilinear, centre
 * clamped at 0) or 4 taps (bicubic, a = -0.75), taps beyond the crop folded onto its border sample; antialias = 1: the
 * triangle / cubic (a = -0.5) filter stretched by max(scale, 1) over its clipped window, normalised.  Zero weights at
 * the ends of a window are dropped, so an identity crop is one tap of weight 1.0.  flip = 1 reverses the output order
 * (RandomHorizontalFlip for the x table).  vtx_resample_max_taps: the max_taps the table needs (> 0), or VTX_EINVAL. */
#define VTX_RESAMPLE_BILINEAR 0
#define VTX_RESAMPLE_BICUBIC 1
int vtx_resample_max_taps(int crop_len, int out_len, int mode, int antialias);
int vtx_resample_build_table(int src_len, int crop_start, int crop_len, int out_len, int mode, int antialias, int flip,
                             int max_taps, int32_t* first, int32_t* count, float* weights);
/* dst[b,t] = round_half_even(clamp(Wy[b] * src[b,t] * Wx[b]^T, 0, 255)) per channel: src [B,T,Hs,Ws,3] -> dst [B,T,H,W,3]
 * uint8, x pass first, then y pass, float32 without contraction (torch's order; the cast is torchvision's
 * _cast_squeeze_out).  Device tables per clip (all frames of a clip share them): x_first / x_count [B,W] int32,
 * x_weights [B,W,x_taps] float32, likewise y with H and y_taps -- B uploads of vtx_resample_build_table.  Only the first
 * count taps of an output are read, and tap windows are clamped into the source frame on the device.  No alignment
 * requirement on src, dst or the row length. */
int vtx_clip_resample_u8(int B, int T, int Hs, int Ws, int H, int W, const unsigned char* src, unsigned char* dst,
                         const int32_t* x_first, const int32_t* x_count, const float* x_weights, int x_taps,
                         const int32_t* y_first, const int32_t* y_count, const float* y_weights, int y_taps, void* stream);
/* In place: torchvision's ColorJitter(brightness, contrast, saturation) on a uint8 clip [B,T,H,W,3], one draw per clip
 * as the reference's single call on [T,C,H,W] makes it.  ops [B,4] int32 = {number of ops 0..3, op, op, op} in the
 * order to apply, op = 0 brightness | 1 contrast | 2 saturation (each at most once); factors [B,6] float32 =
 * {r, r, r, 1 - r, 1 - r, 1 - r}, entry i and 3 + i belong to op i of the record (torchvision forms 1.0 - r in float64
 * and rounds it to float32 on its own: so does the caller).  Each op is  trunc(clamp(r * img + (1 - r) * other, 0, 255))
 * in float32 (two products, one add); other = 0 | the frame's mean of grey | the pixel's grey, grey = trunc(0.2989 r + 0.587 g + 0.114 b).
 * The mean is the exact integer sum of the frame's greys, converted to float32 and divided once by the pixel count.
 * Bit-identical to torchvision's arithmetic up to 65 793 pixels per frame (the sum stays below 2^24, so torch.mean of
 * the float32 greys is that value whatever its summation order); on larger frames (448 x 448 = 200 704 pixels)
 * torch.mean's own float32 sum is no longer exact and depends on its order, and the call returns the exactly summed,
 * once-rounded mean instead.  Hue is not built (the reference passes three jitter values).
 * workspace: vtx_clip_jitter_workspace(B, T) bytes, 4-byte aligned, zeroed by the call. */
size_t vtx_clip_jitter_workspace(int B, int T);
int vtx_clip_jitter_u8(int B, int T, int H, int W, unsigned char* clip, const int32_t* ops, const float* factors,
                       void* workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VTX_AUG_H_ */
