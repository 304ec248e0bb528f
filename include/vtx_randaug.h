/* vtx_randaug.h -- C ABI of libvtx_randaug.so: RandAugment on decoded uint8 clips for the MI355X (gfx950).
 *
 * The `auto_augment` branch of the reference's transforms_train (data_transform.py:520-521: a truthy auto_augment puts
 * transforms.autoaugment.RandAugment() where ColorJitter would stand; the flag is model_pretrain.py:94).  What is
 * restated is torchvision's tensor path with RandAugment's defaults (num_ops 2, magnitude 9, 31 bins, nearest, no
 * fill); torchvision is not a dependency and no version is pinned (the behaviour is that of 0.13 .. 0.20).
 *
 * A third library next to libvtx.so (include/vtx.h) and libvtx_aug.so (include/vtx_aug.h), built by csrc/build.py from
 * csrc/randaug.hip: the seven symbols and the version of vtx_aug.h stay what their users pin.  Conventions as there:
 * extern "C", plain pointers, device pointers borrowed for the call, nothing allocated, work enqueued on `stream` (a
 * hipStream_t passed as void*) of the current device, VTX_OK or a negative VTX_E* code, never throws;
 * vtx_randaug_last_error_string() gives the reason of the last failure on the calling thread.  Argument errors (null
 * pointer, non-positive size, short workspace, src == dst) return VTX_EINVAL and launch nothing.  Python binds it with
 * ctypes (vtx/_lib.py: RANDAUG_SIGNATURES).
 *
 * Clips are uint8 [B,T,H,W,3] (channels last), contiguous, without alignment requirement: frames of a multiple of four
 * pixels in a 4-byte aligned clip take a 32-bit path, all others a byte path.  One draw per clip, shared by its frames,
 * as the reference's single call on a [T,C,H,W] tensor makes it.  `sel` is [B] int32 on the device: where sel[b] == 0
 * the clip is left exactly as it is (in-place kernels skip it, out-of-place kernels copy it).  Brightness, Color and
 * Contrast of RandAugment are ops 0 / 2 / 1 of vtx_clip_jitter_u8 (vtx_aug.h) with factor 1 + magnitude.
 */
#ifndef VTX_RANDAUG_H_
#define VTX_RANDAUG_H_

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

int vtx_randaug_version(void);                   /* 100 = 0.1.0 */
const char* vtx_randaug_last_error_string(void);

/* ShearX / ShearY / TranslateX / TranslateY / Rotate (torchvision autoaugment._apply_op -> F.affine / F.rotate with
 * InterpolationMode.NEAREST, fill None; functional_tensor._gen_affine_grid + grid_sample(mode='nearest',
 * padding_mode='zeros', align_corners=False)).  Out of place, src != dst.  theta [B,6] float32 is the inverse matrix
 * of _get_inverse_affine_matrix, formed by the caller in float64 and rounded once.  For output pixel (xo, yo)
 *   sx = M0 (xo - W/2 + .5) + M1 (yo - H/2 + .5) + M2 + W/2 - .5,   sy likewise with M3 .. M5 and H,
 * evaluated in float32; dst = src at (rint sx, rint sy), halves to even, and 0 outside the frame. */
int vtx_clip_warp_nearest_u8(int B, int T, int H, int W, const unsigned char* src, unsigned char* dst, const float* theta,
                             const int32_t* sel, void* stream);
/* Sharpness (F.adjust_sharpness: functional_tensor._blurred_degenerate_image + _blend).  Out of place, src != dst.
 * degenerate = round((8 neighbours + 5 centre) / 13) inside the frame and the frame itself on its one-pixel border;
 * dst = trunc(clamp(r * src + (1 - r) * degenerate, 0, 255)) in float32 (two products, one add), border included.
 * factors [B,2] float32 = {r, 1 - r} (1.0 - r formed in float64 and rounded on its own, as for the jitter).  Frames
 * with H <= 2 or W <= 2 are copied. */
int vtx_clip_sharpness_u8(int B, int T, int H, int W, const unsigned char* src, unsigned char* dst, const float* factors,
                          const int32_t* sel, void* stream);
/* Posterize and Solarize (F.posterize, F.solarize), in place.  ops [B,2] int32 = {op, argument}: 0 = none,
 * 1 = posterize to `argument` bits (0 .. 8): v & ~((1 << (8 - bits)) - 1), 2 = solarize: v >= argument ? 255 - v : v
 * (argument = ceil of torchvision's float threshold).  Any other op code leaves the clip as it is. */
int vtx_clip_pointwise_u8(int B, int T, int H, int W, unsigned char* clip, const int32_t* ops, void* stream);
/* AutoContrast (F.autocontrast), in place, per frame and channel: lo, hi = min, max of the channel; hi == lo leaves it,
 * else v -> trunc(clamp((v - lo) * (255.0f / (hi - lo)), 0, 255)) with the float32 division correctly rounded.
 * workspace: vtx_clip_autocontrast_workspace(B, T) bytes, 4-byte aligned, initialised by the call. */
size_t vtx_clip_autocontrast_workspace(int B, int T);
int vtx_clip_autocontrast_u8(int B, int T, int H, int W, unsigned char* clip, const int32_t* sel, void* workspace,
                             size_t ws_bytes, void* stream);
/* Equalize (F.equalize: functional_tensor._scale_channel), in place, per frame and channel, in integers: hist = the 256-bin
 * histogram, step = (sum of the non-zero bins but the last non-zero one) / 255; step == 0 leaves the channel, else
 * v -> lut[v], lut[0] = 0, lut[i] = min((hist[0] + .. + hist[i - 1] + step / 2) / step, 255).
 * workspace: vtx_clip_equalize_workspace(B, T) bytes (the histograms), 4-byte aligned, initialised by the call. */
size_t vtx_clip_equalize_workspace(int B, int T);
int vtx_clip_equalize_u8(int B, int T, int H, int W, unsigned char* clip, const int32_t* sel, void* workspace,
                         size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VTX_RANDAUG_H_ */
