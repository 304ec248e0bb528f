// mix.hip -- batch-mode Mixup / CutMix (reference mixup.py:59-126) on decoded uint8 clips [B,T,H,W,3], the last step of the
// reference's training input path (model_trainer.py:87-88,142-143) that had no uint8 form.
//
//   CutMix  swaps a box between clip b and clip B-1-b.  ToTensor + Normalize act per sample, so swapping the bytes before
//           them equals swapping the floats after them: vtx_cutmix_batch_u8, in place.
//   Mixup   is x[b]*lam + x[B-1-b]*(1-lam) on the NORMALISED floats.  The mixed clip has no uint8 form, but it never has to
//           be stored: vtx_patch_rows_mix_u8 is the patch gather of vtx_patch_rows_u8 (csrc/elementwise.hip) reading both
//           partners and writing the mixed rows.
//
// Arithmetic contract of the gather: per operand pair five float32 operations, each rounded on its own, in the order of
// patch_rows_u8_kernel followed by mixup_kernel (csrc/head.hip) --
//     n(v,c) = ((float)v / 255.0f - mean[c]) / std[c]          div, sub, div
//     row    = n(a)*lam + n(c)*one_minus_lam                   mul, mul, add
// without fma contraction, so the fp32 rows equal vtx_patch_rows of vtx_mixup_batch of the normalised float clip bit for
// bit, and the bf16 rows are that value rounded once (the conversion of ET<bf16raw>::st / store8).
//
// Bytes: one thread serves BOTH clips of a pair -- the pair's normalised values are each other's second operand -- so a clip
// byte is read once and normalised once: 1 byte read and 2 written (bf16) per sample, as vtx_patch_rows_u8.  The route it
// replaces (normalise to a float clip, mix it in place, gather) moves 4 + 8 + 6 = 19 bytes per sample with the byte read.
//
// A library of its own, libvtx_mix.so (include/vtx_mix.h): the other four keep their export lists and versions.  Error
// plumbing, version and last-error exports, and grid_for: side_lib.h.
#include <string.h>
#include "side_lib.h"
#include "../../include/vtx_mix.h"

VTX_SIDE_LIB(mix)

namespace vtx {

// ---- CutMix: swap the box rows of clip b and clip B-1-b, b < B/2 -------------------------------------------------------
// A box row of one frame is (xh - xl) * 3 contiguous bytes; nothing about it is aligned (W*3, xl*3 and the clip pointer are
// arbitrary).  The row is cut at the 16-byte boundaries of clip b's ADDRESSES; one thread owns one such piece in both
// partners, reads both, then writes both -- no byte of a pair is touched by two threads, none outside the box is written.
// A whole piece whose partner address is 16-byte aligned too (the partner is a multiple of T*H*W*3 bytes away: every
// usual frame size) moves as one 16-byte access each way; the pieces at the two ends of a row, and every piece of a pair
// with another distance, move byte by byte.
__global__ __launch_bounds__(256) void cutmix_u8_kernel(int half_b, int B, int T, int H, int W, uint8_t* __restrict__ clip,
                                                        int yl, int yh, int xl, int xh, int pieces) {
  const long row_bytes = (long)W * 3, per_clip = (long)T * H * row_bytes;
  const int n = (xh - xl) * 3, bh = yh - yl;
  const long total = (long)half_b * T * bh * pieces;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    long r = i;
    const int k = (int)(r % pieces); r /= pieces;
    const int y = yl + (int)(r % bh); r /= bh;
    const int t = (int)(r % T); r /= T;
    const int b = (int)r;
    const long off = (((long)b * T + t) * H + y) * row_bytes + (long)xl * 3;   // the box row in clip b: bytes [off, off + n)
    const long dist = (long)(B - 1 - 2 * b) * per_clip;                        // ... and in clip B-1-b: dist further on
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(clip) + off;
    const long first = (long)(a0 & 15u);                                       // piece k: row bytes [16k - first, 16k - first + 16)
    long lo = 16L * k - first, hi = lo + 16;
    const bool whole = lo >= 0 && hi <= n;
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    if (lo >= hi) continue;
    uint8_t* pa = clip + off + lo;
    uint8_t* pc = pa + dist;
    if (whole && (reinterpret_cast<uintptr_t>(pc) & 15u) == 0) {
      const uint4 va = *reinterpret_cast<const uint4*>(pa), vc = *reinterpret_cast<const uint4*>(pc);
      *reinterpret_cast<uint4*>(pa) = vc;
      *reinterpret_cast<uint4*>(pc) = va;
    } else {
      const int m = (int)(hi - lo);
      uint8_t va[16], vc[16];
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (j < m) { va[j] = pa[j]; vc[j] = pc[j]; }
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (j < m) { pa[j] = vc[j]; pc[j] = va[j]; }
    }
  }
}

// ---- the patch gather of the mixed batch -----------------------------------------------------------------------------
// N pixels x 3 channels = 3N contiguous bytes of each partner (N = 4 or 8: whole 32-bit words) -> N row elements per channel
// of each partner's row.  da / dc point at channel 0 of the run; the channels of a row are `cs` elements apart.
template <typename T, int N>
__device__ inline void mix_run(const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sc, T* __restrict__ da,
                               T* __restrict__ dc, long cs, const float (&mean)[3], const float (&sd)[3], float lam, float oml) {
#pragma clang fp contract(off)
  constexpr int NW = N * 3 / 4;
  uint32_t wa[NW], wc[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    wa[i] = reinterpret_cast<const uint32_t*>(sa)[i];
    wc[i] = reinterpret_cast<const uint32_t*>(sc)[i];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float ra[N], rc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int e = 3 * j + c;                                                 // byte e of the run: little-endian words
      const float xa = (float)((wa[e >> 2] >> (8 * (e & 3))) & 255u) / 255.0f;
      const float xc = (float)((wc[e >> 2] >> (8 * (e & 3))) & 255u) / 255.0f;
      const float na = (xa - mean[c]) / sd[c], nc = (xc - mean[c]) / sd[c];
      ra[j] = na * lam + nc * oml;
      rc[j] = nc * lam + na * oml;
    }
    if constexpr (N == 8) {
      store8(da + c * cs, ra);
      store8(dc + c * cs, rc);
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        ET<T>::st(da + c * cs + j, ra[j]);
        ET<T>::st(dc + c * cs + j, rc[j]);
      }
    }
  }
}

// One thread per (pair b < B/2, tq, ph, kt, kh, pw) -- patch_rows_u8_kernel's index with the pair in place of the clip: 3*ps
// contiguous bytes of clip b and of clip B-1-b in, ps elements per channel of both clips' rows out.  Eight pixels per step
// (16-byte bf16 / two 16-byte fp32 stores, as patch_rows_kernel's store8 path) when ps, ldr and the pointer allow it.
template <typename T>
__global__ __launch_bounds__(256) void patch_rows_mix_u8_kernel(int B, int Tn, int H, int W, int ps, int ts,
                                                                const uint8_t* __restrict__ clip, float m0, float m1, float m2,
                                                                float s0, float s1, float s2, float lam, float oml,
                                                                T* __restrict__ rows, long ldr, int frame_major) {
  const int gh = H / ps, gw = W / ps, P = gh * gw, Tq = Tn / ts, hb = B / 2;
  const long total = (long)hb * Tq * P * ts * ps;
  const long cs = (long)ts * ps * ps;
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
  const bool vec8 = (ps & 7) == 0 && (ldr & 7) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15u) == 0;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    long r = idx;                                   // idx -> (b, tq, ph, kt, kh, pw): pw fastest
    const int pw = (int)(r % gw); r /= gw;
    const int kh = (int)(r % ps); r /= ps;
    const int kt = (int)(r % ts); r /= ts;
    const int ph = (int)(r % gh); r /= gh;
    const int tq = (int)(r % Tq); r /= Tq;
    const int b = (int)r, bc = B - 1 - b;
    const long in_clip = (((long)(tq * ts + kt) * H + (ph * ps + kh)) * W + pw * ps) * 3;
    const uint8_t* sa = clip + (long)b * Tn * H * W * 3 + in_clip;
    const uint8_t* sc = clip + (long)bc * Tn * H * W * 3 + in_clip;
    const int p = ph * gw + pw;
    const long rowa = frame_major ? ((long)b * Tq + tq) * P + p : ((long)b * P + p) * Tq + tq;
    const long rowc = frame_major ? ((long)bc * Tq + tq) * P + p : ((long)bc * P + p) * Tq + tq;
    const long in_row = ((long)kt * ps + kh) * ps;
    T* da = rows + rowa * ldr + in_row;
    T* dc = rows + rowc * ldr + in_row;
    if (vec8) {
      for (int kw = 0; kw < ps; kw += 8) mix_run<T, 8>(sa + kw * 3, sc + kw * 3, da + kw, dc + kw, cs, mean, sd, lam, oml);
    } else {
      for (int kw = 0; kw < ps; kw += 4) mix_run<T, 4>(sa + kw * 3, sc + kw * 3, da + kw, dc + kw, cs, mean, sd, lam, oml);
    }
  }
}

}  // namespace vtx

using namespace vtx;

extern "C" int vtx_cutmix_batch_u8(int B, int T, int H, int W, unsigned char* clip, int yl, int yh, int xl, int xh, void* stream) {
  VTX_REQUIRE(clip, VTX_EINVAL, "cutmix_batch_u8: null pointer");
  VTX_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0, VTX_EINVAL, "cutmix_batch_u8: B=%d T=%d H=%d W=%d must all be positive", B, T, H, W);
  VTX_REQUIRE(B % 2 == 0, VTX_EINVAL, "cutmix_batch_u8: clip b is paired with clip B-1-b: B=%d must be even", B);
  VTX_REQUIRE(0 <= yl && yl <= yh && yh <= H && 0 <= xl && xl <= xh && xh <= W, VTX_EINVAL,
              "cutmix_batch_u8: box rows [%d,%d) columns [%d,%d) outside the %dx%d frame", yl, yh, xl, xh, H, W);
  if (yl == yh || xl == xh) return VTX_OK;
  const int pieces = ((xh - xl) * 3 + 15) / 16 + 1;          // a row that starts inside a 16-byte block spills into one more
  hipLaunchKernelGGL(cutmix_u8_kernel, dim3(grid_for((long)(B / 2) * T * (yh - yl) * pieces, 16384)), dim3(256), 0, as_stream(stream),
                     B / 2, B, T, H, W, clip, yl, yh, xl, xh, pieces);
  return check_launch("cutmix_batch_u8");
}

extern "C" int vtx_patch_rows_mix_u8(int dtype, int B, int T, int H, int W, int ps, int ts, const unsigned char* clip,
                                     const float* host_mean3, const float* host_std3, float lam, float one_minus_lam, void* rows,
                                     long ldr, int frame_major, void* stream) {
  VTX_REQUIRE(clip && rows && host_mean3 && host_std3, VTX_EINVAL, "patch_rows_mix_u8: null pointer");
  VTX_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && ps > 0 && ts > 0, VTX_EINVAL,
              "patch_rows_mix_u8: B=%d T=%d H=%d W=%d ps=%d ts=%d must all be positive", B, T, H, W, ps, ts);
  VTX_REQUIRE(B % 2 == 0, VTX_EINVAL, "patch_rows_mix_u8: clip b is mixed with clip B-1-b: B=%d must be even", B);
  VTX_REQUIRE(H % ps == 0 && W % ps == 0 && T % ts == 0 && ps % 4 == 0, VTX_EINVAL,
              "patch_rows_mix_u8: H,W must be multiples of ps (itself a multiple of 4), T of ts");
  VTX_REQUIRE(dtype == VTX_F32 || dtype == VTX_BF16, VTX_EINVAL, "patch_rows_mix_u8: bad dtype %d", dtype);
  VTX_REQUIRE(ldr >= 3L * ts * ps * ps, VTX_EINVAL, "patch_rows_mix_u8: ldr=%ld is shorter than a row of %ld", ldr, 3L * ts * ps * ps);
  VTX_REQUIRE(host_std3[0] != 0.f && host_std3[1] != 0.f && host_std3[2] != 0.f, VTX_EINVAL, "patch_rows_mix_u8: zero std");
  VTX_REQUIRE((reinterpret_cast<uintptr_t>(clip) & 3u) == 0, VTX_EALIGN, "patch_rows_mix_u8: clip must be 4-byte aligned");
  const long work = (long)(B / 2) * (T / ts) * (H / ps) * (W / ps) * ts * ps;
  dim3 grid(grid_for(work, 16384)), block(256);
  hipStream_t st = as_stream(stream);
  const float *m = host_mean3, *s = host_std3;
  if (dtype == VTX_F32)
    hipLaunchKernelGGL(patch_rows_mix_u8_kernel<float>, grid, block, 0, st, B, T, H, W, ps, ts, clip, m[0], m[1], m[2], s[0], s[1], s[2],
                       lam, one_minus_lam, (float*)rows, ldr, frame_major);
  else
    hipLaunchKernelGGL(patch_rows_mix_u8_kernel<bf16raw>, grid, block, 0, st, B, T, H, W, ps, ts, clip, m[0], m[1], m[2], s[0], s[1], s[2],
                       lam, one_minus_lam, (bf16raw*)rows, ldr, frame_major);
  return check_launch("patch_rows_mix_u8");
}
