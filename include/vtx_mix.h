/* vtx_mix.h -- C ABI of libvtx_mix.so: batch-mode Mixup / CutMix on decoded uint8 clips for the MI355X (gfx950).
 *
 * The fifth library, next to libvtx.so (include/vtx.h), libvtx_aug.so (include/vtx_aug.h), libvtx_randaug.so
 * (include/vtx_randaug.h) and libvtx_views.so (include/vtx_views.h), built by the same csrc/build.py from csrc/mix.hip:
 * those four keep their export lists and versions.  Conventions as in vtx.h: extern "C", plain pointers, device pointers
 * borrowed for the call, nothing allocated, work enqueued on `stream` (a hipStream_t passed as void*) of the current
 * device, VTX_OK or a negative VTX_E* code (the codes of vtx.h), never throws; every argument is checked before anything
 * is launched, and vtx_mix_last_error_string() gives the reason of the last failure on the calling thread.  Python binds
 * it with ctypes (vtx/_lib.py: MIX_SIGNATURES).
 *
 * The float forms are vtx_mixup_batch / vtx_cutmix_batch of vtx.h; the pairing is theirs: clip b with clip B-1-b
 * (the reference's x.flip(0), mixup.py:105-113), so B is even.
 */
#ifndef VTX_MIX_H_
#define VTX_MIX_H_

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

int vtx_mix_version(void);                        /* 100 = 0.1.0 */
const char* vtx_mix_last_error_string(void);

/* CutMix, in place on uint8 [B,T,H,W,3] (channels last):
 *
 *   clip[b,t,yl:yh,xl:xh,:] <-> clip[B-1-b,t,yl:yh,xl:xh,:]   for b < B/2
 *
 * (mixup.py:109: x[:, :, yl:yh, xl:xh] = x.flip(0)[...] on the [B,T*C,H,W] view; flip copies, so it is a swap).  ToTensor
 * and Normalize act on each sample alone, so swapping bytes before them equals swapping floats after them.  B even,
 * 0 <= yl <= yh <= H, 0 <= xl <= xh <= W; an empty box returns VTX_OK and launches nothing.  No alignment requirement on
 * clip, W*3 or the box; bytes outside the box are never written.  One thread owns a piece of a box row in both partners
 * (it reads both, then writes both): 16 bytes at a time where both partners' addresses allow it, single bytes at the
 * ends of a row and for pairs whose distance is no multiple of 16.  Moves 2 bytes per box sample each way (the float
 * form: 4 * 2). */
int vtx_cutmix_batch_u8(int B, int T, int H, int W, unsigned char* clip, int yl, int yh, int xl, int xh, void* stream);

/* The rows of vtx_patch_rows_u8 (vtx.h) for the Mixup of the batch, without the mixed clip ever being stored:
 *
 *   n(v,c)       = ((float)v / 255.0f - mean[c]) / std[c]
 *   rows(b, ...) = n(clip[b]) * lam + n(clip[B-1-b]) * one_minus_lam
 *
 * clip uint8 [B,T,H,W,3] -> rows [B*(T/ts)*(H/ps)*(W/ps)][ldr] of dtype (VTX_F32 / VTX_BF16), row order and columns as
 * vtx_patch_rows_u8 (frame_major: (b,t',p), else (b,p,t'); column (c, kt, kh, kw)).  Five float32 operations per operand
 * pair, each rounded on its own (div, sub, div; mul, mul, add; no contraction): vtx_patch_rows_u8's normalisation followed
 * by vtx_mixup_batch's blend, so with VTX_F32 the rows equal vtx_patch_rows of vtx_mixup_batch of the normalised float clip
 * bit for bit, and with VTX_BF16 they are that value rounded once, as vtx_patch_rows_u8 rounds.  Pass lam and
 * one_minus_lam as vtx_mixup_batch gets them (1 - lam formed in double, rounded once).  host_mean3 / host_std3: three host
 * floats each, read during the call.  Preconditions of vtx_patch_rows_u8: ps a multiple of 4, H and W multiples of ps, T
 * of ts, non-zero std, clip 4-byte aligned (VTX_EALIGN); B even; ldr >= 3*ts*ps*ps.  Eight elements per store when ps and
 * ldr are multiples of 8 and rows is 16-byte aligned.  One thread serves both clips of a pair, so a clip byte is read and
 * normalised once: 1 byte read and 2 (bf16) written per sample, against 19 for normalise + mix + gather on a float clip. */
int vtx_patch_rows_mix_u8(int dtype, int B, int T, int H, int W, int ps, int ts, const unsigned char* clip,
                          const float* host_mean3, const float* host_std3, float lam, float one_minus_lam,
                          void* rows, long ldr, int frame_major, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VTX_MIX_H_ */
