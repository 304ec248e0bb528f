// stem.hip -- MaskFeat from decoded uint8 clips [B,T,H,W,3]: the two things the reference's `mim` input path does with the
// bytes behind the crop / flip (data_trainer.py:61-63, dataset.py:171-196) that had no device form.
//
//   vtx_im2col3d_u8   the rows of the MViT stem's overlapping, padded Conv3d (video_transformer.py:585-618, 834-843) with
//                     ToTensor + Normalize applied on the fly: vtx_im2col3d (csrc/mvit.hip) reading bytes.
//   vtx_hog_fwd_sel   the HOG targets of the centre frames of the masked cubes (dataset.py:188-196): hog_kernel
//                     (csrc/hog_kernel.h, the code vtx_hog_fwd runs) behind a list of frame indices, one launch per batch.
//
// Arithmetic contract of the gather (patch_rows_u8_kernel, elementwise.hip, and mix.hip state the same one): an in-bounds tap is
//     n(v,c) = ((float)v / 255.0f - mean[c]) / std[c]          div, sub, div: three fp32 roundings, no fma contraction
// a padding tap (t, h or w outside the clip) is +0.0f -- the reference pads the NORMALISED tensor, so it is not n(0,c) -- and so
// are the columns K .. Kp-1.  The fp32 rows therefore equal im2col3d_kernel's rows of the normalised float clip bit for bit,
// the bf16 rows are that value rounded once (store8).
//
// Bytes: MaskFeat's stem (kernel (3,7,7), stride (2,4,4), padding (1,3,3) on 16 x 224^2) writes 25 088 rows x 448 bf16 columns
// = 22.5 MB per clip and reads 2.4 MB of clip bytes, each about 4.6 times (from L2); the float route reads 9.6 MB per clip
// that a normalising pass had to write first.  Store-bound either way.
//
// A library of its own, libvtx_stem.so (include/vtx_stem.h): the other five keep their export lists and versions.  Error
// plumbing, version and last-error exports, and grid_for: side_lib.h.  -ffp-contract=off as hog.hip.
#include <string.h>
#include "side_lib.h"
#include "hog_kernel.h"
#include "../../include/vtx_stem.h"

VTX_SIDE_LIB(stem)

namespace vtx {

// n(v,c) depends on (v, c) alone: each workgroup computes the 3 x 256 values once into LDS (768 entries over 256 threads: six
// divisions per thread and workgroup, and the launcher sizes the grid so that a workgroup stores some twenty times 4 KiB
// behind them) and a stored element costs one byte load and one ds_read_b32 instead of two divisions.  The table is
// tab[c][v]: its bank is v mod 32, so the lanes of a 32-lane group collide only where their bytes differ by a multiple of 32
// (equal bytes broadcast); eight reads per 16-byte store stay far below the store rate even at several LDS cycles each.
//   The thread mapping is im2col3d_kernel's: a thread owns 8 consecutive columns of one row (one 16-byte store for bf16), a
// wave 1 KiB of consecutive row bytes; the row's (b, to, ho, wo) and the first column's (c, kt, kh, kw) are decoded once, the
// other seven columns by carrying.  Taps are single byte loads (kw runs in steps of 3 bytes, and rows of 3 W bytes carry no
// alignment for odd W): the clip needs NO alignment.  32-bit index arithmetic; the launcher checks both bounds.
template <typename T>
__global__ __launch_bounds__(256) void im2col3d_u8_kernel(int B, int Tc, int H, int W, int KT, int KH, int KW, int st, int sh, int sw,
                                                          int pt, int ph, int pw, int To, int Ho, int Wo, int Kp,
                                                          const uint8_t* __restrict__ clip, float m0, float m1, float m2, float s0,
                                                          float s1, float s2, T* __restrict__ rows) {
#pragma clang fp contract(off)
  __shared__ float s_n[3 * 256];
  {
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
    const float x = (float)threadIdx.x / 255.0f;                        // (blockDim.x == 256: thread v makes n(v, 0 .. 2))
#pragma unroll
    for (int c = 0; c < 3; ++c) s_n[c * 256 + threadIdx.x] = (x - mean[c]) / sd[c];
  }
  __syncthreads();
  const unsigned K8 = (unsigned)Kp / 8;
  const unsigned total = (unsigned)B * To * Ho * Wo * K8;               // < 2^31 (checked by the launcher)
  const int K = 3 * KT * KH * KW;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const unsigned row = i / K8, k0 = (i - row * K8) * 8;
    const unsigned r1 = row / (unsigned)Wo, wo = row - r1 * Wo;
    const unsigned r2 = r1 / (unsigned)Ho, ho = r1 - r2 * Ho;
    const unsigned b = r2 / (unsigned)To, to = r2 - b * To;
    const unsigned q1 = k0 / (unsigned)KW;
    int kw = (int)(k0 - q1 * KW);
    const unsigned q2 = q1 / (unsigned)KH;
    int kh = (int)(q1 - q2 * KH);
    int c = (int)(q2 / (unsigned)KT), kt = (int)(q2 - (unsigned)c * KT);
    const int t0 = (int)to * st - pt, h0 = (int)ho * sh - ph, w0 = (int)wo * sw - pw;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int t = t0 + kt, h = h0 + kh, w = w0 + kw;
      v[j] = 0.f;
      if ((int)k0 + j < K && t >= 0 && t < Tc && h >= 0 && h < H && w >= 0 && w < W)         // (k < K: c is 0, 1 or 2)
        v[j] = s_n[c * 256 + clip[((((unsigned)b * Tc + t) * H + h) * W + w) * 3 + c]];      // clip index < 2^31 (launcher)
      if (++kw == KW) { kw = 0; if (++kh == KH) { kh = 0; if (++kt == KT) { kt = 0; ++c; } } }
    }
    store8(rows + (long)row * Kp + k0, v);
  }
}

}  // namespace vtx

using namespace vtx;

extern "C" int vtx_im2col3d_u8(int dtype, int B, int T, int H, int W, const int* k3, const int* s3, const int* p3, int Kp,
                               const unsigned char* clip, const float* host_mean3, const float* host_std3, void* rows, void* stream) {
  VTX_REQUIRE(clip && rows && k3 && s3 && p3 && host_mean3 && host_std3, VTX_EINVAL, "im2col3d_u8: null pointer");
  VTX_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0, VTX_EINVAL, "im2col3d_u8: B=%d T=%d H=%d W=%d must all be positive", B, T, H, W);
  VTX_REQUIRE(dtype == VTX_F32 || dtype == VTX_BF16, VTX_EINVAL, "im2col3d_u8: bad dtype %d", dtype);
  for (int i = 0; i < 3; ++i)
    VTX_REQUIRE(k3[i] > 0 && k3[i] <= 1024 && s3[i] > 0 && p3[i] >= 0 && p3[i] <= 1024, VTX_EINVAL,
                "im2col3d_u8: axis %d: kernel %d and stride %d must be positive, padding %d not negative (kernel, padding <= 1024)",
                i, k3[i], s3[i], p3[i]);
  VTX_REQUIRE(host_std3[0] != 0.f && host_std3[1] != 0.f && host_std3[2] != 0.f, VTX_EINVAL, "im2col3d_u8: zero std");
  const long K = 3L * k3[0] * k3[1] * k3[2];
  VTX_REQUIRE(Kp >= K && Kp % 8 == 0, VTX_EINVAL, "im2col3d_u8: row width Kp=%d must cover 3*kt*kh*kw=%ld and be a multiple of 8", Kp, K);
  const long Tp = (long)T + 2 * p3[0] - k3[0], Hp = (long)H + 2 * p3[1] - k3[1], Wp = (long)W + 2 * p3[2] - k3[2];
  VTX_REQUIRE(Tp >= 0 && Hp >= 0 && Wp >= 0, VTX_EINVAL, "im2col3d_u8: empty output grid: the padded clip is smaller than the kernel");
  const long To = Tp / s3[0] + 1, Ho = Hp / s3[1] + 1, Wo = Wp / s3[2] + 1;
  const long total = (long)B * To * Ho * Wo * (Kp / 8);
  VTX_REQUIRE(total < (1L << 31) && (long)B * T * H * W * 3 < (1L << 31), VTX_EINVAL,
              "im2col3d_u8: tensor too large for the 32-bit index arithmetic");
  VTX_REQUIRE(aligned16(rows), VTX_EALIGN, "im2col3d_u8: rows must be 16-byte aligned (the clip needs no alignment)");
  // a workgroup's first act is the 768-entry table: at most 8192 workgroups walk the rows instead of one per 256 stores
  const dim3 grid(grid_for(total, 8192)), block(256);
  const float *m = host_mean3, *s = host_std3;
  if (dtype == VTX_F32)
    hipLaunchKernelGGL(im2col3d_u8_kernel<float>, grid, block, 0, as_stream(stream), B, T, H, W, k3[0], k3[1], k3[2], s3[0], s3[1], s3[2],
                       p3[0], p3[1], p3[2], (int)To, (int)Ho, (int)Wo, Kp, clip, m[0], m[1], m[2], s[0], s[1], s[2], (float*)rows);
  else
    hipLaunchKernelGGL(im2col3d_u8_kernel<bf16raw>, grid, block, 0, as_stream(stream), B, T, H, W, k3[0], k3[1], k3[2], s3[0], s3[1], s3[2],
                       p3[0], p3[1], p3[2], (int)To, (int)Ho, (int)Wo, Kp, clip, m[0], m[1], m[2], s[0], s[1], s[2], (bf16raw*)rows);
  return check_launch("im2col3d_u8");
}

extern "C" int vtx_hog_fwd_sel(const unsigned char* frames, int F, int H, int W, const int* sel, int n, const double* table,
                               size_t table_bytes, double* out, void* stream) {
  VTX_REQUIRE(frames && sel && table && out, VTX_EINVAL, "hog_fwd_sel: null pointer");
  VTX_REQUIRE(F > 0 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0 && W <= 1024, VTX_EINVAL,
              "hog_fwd_sel: F=%d must be positive, H=%d and W=%d multiples of 16 (W <= 1024)", F, H, W);
  VTX_REQUIRE(n > 0, VTX_EINVAL, "hog_fwd_sel: empty selection (n=%d)", n);
  // the blob of vtx_hog_build_table (libvtx.so): 65 536 doubles of magnitudes, then the correction words the kernel reads
  const size_t need = (size_t)256 * 256 * sizeof(double) + (size_t)HOG_EXC_WORDS * sizeof(uint32_t);
  VTX_REQUIRE(table_bytes >= need, VTX_EINVAL, "hog_fwd_sel: the table blob holds %zu bytes, vtx_hog_table_bytes() = %zu "
              "(magnitudes + correction words: build it with vtx_hog_build_table)", table_bytes, need);
  // (every frame and every row of out starts a multiple of 768 bytes behind the first: aligned where the buffers are)
  VTX_REQUIRE(aligned16(frames) && aligned16(out), VTX_EALIGN, "hog_fwd_sel: frames and out must be 16-byte aligned");
  VTX_REQUIRE((reinterpret_cast<uintptr_t>(sel) & 3u) == 0, VTX_EALIGN, "hog_fwd_sel: sel must be 4-byte aligned");
  return hog_launch("hog_fwd_sel", frames, n, H, W, table, out, nullptr, sel, F, stream);
}
