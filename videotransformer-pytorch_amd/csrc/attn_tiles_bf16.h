// attn_tiles_bf16.h -- Bf16Tiles<HD, CHUNK>: the bf16 tile policy of the chunk-streaming kernels (attn_stream.h; read its header
// for what a policy is).  The formulation is the one of attn_mfma.hip (see there for the layout argument; the helpers live in
// attn_common.h): scores with v_mfma_f32_32x32x16_bf16, the transposed operands out of swizzled [rows][64] LDS tiles through
// ds_read_b64_tr_b16 (sw_off / frag_rows_o / frag_cols_o).
//
// A head of HD columns is NS = ceil(HD / 64) column slabs of the [rows][64] tile, the last one half used at 32 and 96 (its upper
// 32 columns are never written and never read):
//   scores         HD / 16 chained k-steps, step ks from slab ks / 4                    (2 | 4 | 6 | 8 MFMAs per 32 x 32 score tile)
//   accumulators   HD / 32 f32x16 tiles, tile n from slab n / 2, column half n % 2      (1 | 2 | 3 | 4)
//   no padded products: the half-used slab costs LDS, not matrix instructions.
// One operand of a chunk is NS slabs of CHUNK rows, a stage holds two operands.  attn_long.hip is Bf16Tiles<64, 128> under the
// bodies of attn_stream.h; attn_hd.hip is Bf16Tiles<HD, 64> at head_dim 32, 96 and 128 under its own three bodies (its header
// says why), and its packed kernels for up to 32 tokens (head_dim 64 among them) take Frag, the slab counts and store_rows from here.
#pragma once
#include "attn_stream.h"

namespace vtx {

template <int HD_, int CHUNK_> struct Bf16Tiles {
  static_assert(HD_ == 32 || HD_ == 64 || HD_ == 96 || HD_ == 128, "head dims of the bf16 streaming kernels");
  typedef bf16raw elem;
  static constexpr int HD = HD_;
  static constexpr int CHUNK = CHUNK_;             // rows of the streamed operands per LDS stage
  static constexpr int NS = (HD + 63) / 64;        // column slabs of a row
  static constexpr int NK = HD / 16;               // k-steps of a score tile
  static constexpr int NT = HD / 32;               // accumulator tiles of a result row
  static constexpr int SLAB = CHUNK * 64;          // elements of one [CHUNK][64] slab
  static constexpr int TILE = NS * SLAB;           // one operand of a chunk
  static constexpr int STAGE = 2 * TILE;           // two tiles per stage
  static constexpr int PR = HD / 8;                // 16-byte pieces of a row
  static constexpr int PER = CHUNK * PR / AS_THREADS;  // pieces of one operand per thread
  static_assert(CHUNK * PR % AS_THREADS == 0, "whole pieces per thread");
  static constexpr int STG = MA_STAGE_ELEMS;
  static constexpr bool MASK_PADDED_DS = true;

  // Rows row0 .. row0 + CHUNK - 1 of two operands of one sequence, in flight between two chunks.
  struct Pre { uint4 a[PER], b[PER]; };

  // Issue the loads of one chunk (rows >= L read as zero; a chunk wholly beyond L issues nothing).
  static __device__ __forceinline__ void chunk_load(Pre& x, const bf16raw* b0, long ld0, const RowLin& r0, const bf16raw* b1, long ld1,
                                                    const RowLin& r1, int row0, int L) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int id = threadIdx.x + i * AS_THREADS;
      const int rr = id / PR, c = id - rr * PR;
      const int r = row0 + rr;
      x.a[i] = make_uint4(0, 0, 0, 0);
      x.b[i] = make_uint4(0, 0, 0, 0);
      if (r < L) {
        x.a[i] = *reinterpret_cast<const uint4*>(b0 + lin_row(r0, r) * ld0 + c * 8);
        x.b[i] = *reinterpret_cast<const uint4*>(b1 + lin_row(r1, r) * ld1 + c * 8);
      }
    }
  }
  static __device__ __forceinline__ void chunk_store(const Pre& x, bf16raw* t0, bf16raw* t1) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int id = threadIdx.x + i * AS_THREADS;
      const int rr = id / PR, c = id - rr * PR;
      const int off = (c >> 3) * SLAB + rr * 64 + (((c & 7) ^ sw_of(rr)) << 3);
      *reinterpret_cast<uint4*>(t0 + off) = x.a[i];
      *reinterpret_cast<uint4*>(t1 + off) = x.b[i];
    }
  }

  // A row's HD columns (this lane's half of every 16) in registers; rows beyond nvalid read row nvalid - 1 (load_row_frags).
  struct Frag { bf16x8 f[NK]; };
  static __device__ __forceinline__ void load_frag(Frag& f, const bf16raw* base, long ld, int col0, const RowLin& rl, int row, int nvalid,
                                                   int lane) {
    const int rc = row < nvalid ? row : nvalid - 1;
    const bf16raw* src = base + lin_row(rl, rc) * ld + col0 + 8 * (lane >> 5);
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      union { bf16x8 v; uint4 u; } x;
      x.u = *reinterpret_cast<const uint4*>(src + ks * 16);
      f.f[ks] = x.v;
    }
  }
  static __device__ __forceinline__ float frag_dot(const Frag& a, const Frag& b) {
    float s = 0.f;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) s = frag_dot2(a.f[ks], b.f[ks], s);
    return s;
  }

  typedef FragOff Lane;
  static __device__ __forceinline__ Lane make_lane(int lane) { return make_frag_off(lane); }

  static __device__ __forceinline__ f32x16 scores(const bf16raw* t, int row0, const Frag& b, const Lane& fo) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(t, row0, 0, fo), b.f[0], zero, 0, 0, 0);
#pragma unroll
    for (int ks = 1; ks < NK; ++ks)
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(t + (ks >> 2) * SLAB, row0, ks & 3, fo), b.f[ks], st, 0, 0, 0);
    return st;
  }
  static __device__ __forceinline__ void accum(f32x16 (&acc)[NT], const bf16raw* t, int row0, const f32x16& c, const Lane& fo) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      float pf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = c[8 * s2 + j];
      const bf16x8 pb = pack8(pf);
#pragma unroll
      for (int n = 0; n < NT; ++n)
        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_o(t + (n >> 1) * SLAB, row0 + 16 * s2, n & 1, fo), pb, acc[n], 0, 0, 0);
    }
  }
  // The dk / dv products of one 32-query tile: the S and dP chains interleaved, then dv and dk fed together.
  static __device__ __forceinline__ void dkv_tile(f32x16 (&dk)[NT], f32x16 (&dv)[NT], const bf16raw* Qs, const bf16raw* Os, const float* Ls,
                                                  const float* Ds, int row0, const Frag& kf, const Frag& vf, float c2, const Lane& fo,
                                                  int lane) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Qs, row0, 0, fo), kf.f[0], zero, 0, 0, 0);
    f32x16 dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Os, row0, 0, fo), vf.f[0], zero, 0, 0, 0);
#pragma unroll
    for (int ks = 1; ks < NK; ++ks) {
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Qs + (ks >> 2) * SLAB, row0, ks & 3, fo), kf.f[ks], st, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Os + (ks >> 2) * SLAB, row0, ks & 3, fo), vf.f[ks], dp, 0, 0, 0);
    }
    float pr[16], ds[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int qrow = row0 + 8 * g + 4 * (lane >> 5);
      const float4 l4 = *reinterpret_cast<const float4*>(Ls + qrow);
      const float4 d4 = *reinterpret_cast<const float4*>(Ds + qrow);
      const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dvv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 4 * g + j;
        const float e = __builtin_amdgcn_exp2f(fmaf(st[r], c2, -lv[j]));
        pr[r] = e;
        ds[r] = e * (dp[r] - dvv[j]);              // the softmax scale is applied once to dk at the store
      }
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const bf16x8 pb = pack8(pr + 8 * s2);
      const bf16x8 dsb = pack8(ds + 8 * s2);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        dv[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_o(Os + (n >> 1) * SLAB, row0 + 16 * s2, n & 1, fo), pb, dv[n], 0, 0, 0);
        dk[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_o(Qs + (n >> 1) * SLAB, row0 + 16 * s2, n & 1, fo), dsb, dk[n], 0, 0, 0);
      }
    }
  }

  // Store a [32 x HD] result held transposed (lane & 31 = row, registers = HD columns in NT C tiles): slab by slab through the
  // wave's swizzled [32][64] staging tile, whole 16-byte pieces of a row per lane (store_rows_T of attn_common.h, for NT tiles).
  // ptr_of_row(r) -> destination of tile row r (HD bf16), or nullptr for a padded row.
  template <typename PtrFn>
  static __device__ __forceinline__ void store_rows(bf16raw* stg, const f32x16 (&acc)[NT], float mul, int lane, PtrFn ptr_of_row) {
    const int row = lane & 31;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int ntile = NT - 2 * s < 2 ? NT - 2 * s : 2;       // C tiles of this slab
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        if (nt < ntile) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int col = nt * 32 + 8 * g + 4 * (lane >> 5);
            union { bf16x4 v; uint2 u; } w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w.v[j] = (__bf16)(acc[2 * s + nt][4 * g + j] * mul);
            *reinterpret_cast<uint2*>(stg + sw_off(row, col)) = w.u;
          }
        }
      wave_lds_sync();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = i * 8 + (lane >> 3), c = lane & 7;
        const uint4 v = *reinterpret_cast<const uint4*>(stg + r * 64 + ((c ^ sw_of(r)) << 3));
        bf16raw* dst = ptr_of_row(r);
        if (dst && c < ntile * 4) *reinterpret_cast<uint4*>(dst + s * 64 + c * 8) = v;
      }
      wave_lds_sync();
    }
  }
};

}  // namespace vtx
