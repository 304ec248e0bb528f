// attn_tiles_f32.h -- F32Tiles<HD, CHUNK>: the exact-fp32 tile policy of the chunk-streaming kernels (attn_stream.h; read its
// header for what a policy is).  Every product runs on v_mfma_f32_32x32x2_f32: fp32 operands, an fma chain with fp32 rounding after
// every step.  Scores, probabilities and accumulators stay fp32 registers from the first product to the store.
//
// Operands.  A 32x32x2 fp32 MFMA takes ONE dword of A and one of B per lane (lane l: A[l & 31][l >> 5], B[l >> 5][l & 31]):
//   scores, transposed (S^T = K Q^T; dP^T = V dO^T; in the dk / dv kernel S = Q K^T, dP = dO V^T): A = a row of the LDS
//     tile per lane, read four columns at a time (ds_read_b128 feeds four MFMAs); B = the lane's own row fragment.  The k
//     index of MFMA (g, j) is column 8 g + 4 (l >> 5) + j for both operands -- any order of the HD columns is a dot product.
//   accumulation (O^T += V^T P^T, dq^T += K^T dS^T, dv^T += dO^T P, dk^T += Q^T dS): B = the score tile exactly as the
//     MFMA left it (register r of lane l holds row crow(r, l) = (r & 3) + 8 (r >> 2) + 4 (l >> 5) of column l & 31), so
//     MFMA r contracts the two rows crow(r, 0) and crow(r, 32); A = those rows of the LDS tile, column (l & 31) + 32 n
//     (ds_read_b32, a whole row per half-wave: conflict-free).  P never leaves its registers.
// What a head of HD columns is:
//   row fragment   HD / 2 floats per lane: [4 g + j] = column 8 g + 4 (lane >> 5) + j, g < HD / 8          (16 | 32 | 48 | 64)
//   score tile     HD / 2 chained MFMAs, one ds_read_b128 of a tile row feeds four                          (16 | 32 | 48 | 64)
//   result row     HD / 32 f32x16 accumulators; a 32-row tile of P or dS feeds 16 MFMAs into each           ( 1 |  2 |  3 |  4)
//   LDS row        HD + 4 floats: 144 | 272 | 400 | 528 B = 9 | 17 | 25 | 33 sixteen-byte slots, all odd, so the 16 rows of a
//                  ds_read_b128 group land on 16 different slots of the 256-byte bank row
//   store_rows     whole rows of HD floats through the wave's [32][HD + 4] staging tile
// A stage is two [CHUNK][HD + 4] tiles.  attn_f32.hip is F32Tiles<64, 64>; attn_hd_f32.hip picks the chunk rows per kernel.
#pragma once
#include "attn_stream.h"

namespace vtx {

template <int HD_, int CHUNK_> struct F32Tiles {
  static_assert(HD_ == 32 || HD_ == 64 || HD_ == 96 || HD_ == 128, "head dims of the fp32 streaming kernels");
  typedef float elem;
  static constexpr int HD = HD_;
  static constexpr int CHUNK = CHUNK_;             // rows of the streamed operands per LDS stage
  static constexpr int LD = HD + 4;                // floats per LDS row (see the bank argument above)
  static constexpr int NG = HD / 8;                // ds_read_b128 groups of a score tile (four MFMAs each)
  static constexpr int NT = HD / 32;               // accumulator tiles of a result row
  static constexpr int FR = HD / 2;                // floats of a row fragment per lane
  static constexpr int PR = HD / 4;                // 16-byte pieces of a row
  static constexpr int TILE = CHUNK * LD;          // floats of one [CHUNK][LD] tile
  static constexpr int STAGE = 2 * TILE;           // two tiles per stage
  static constexpr int PER = CHUNK * PR / AS_THREADS;  // pieces of one tile per thread
  static_assert(CHUNK * PR % AS_THREADS == 0, "whole pieces per thread");
  static constexpr int STG = 32 * LD;              // per-wave [32][LD] staging tile for row stores
  static constexpr bool MASK_PADDED_DS = false;

  struct Pre { float4 a[PER], b[PER]; };           // rows row0 .. row0 + CHUNK - 1 of two operands, in flight between two chunks

  // Issue the loads of one chunk (rows >= L read as zero; a chunk wholly beyond L issues nothing).
  static __device__ __forceinline__ void chunk_load(Pre& x, const float* b0, long ld0, const RowLin& r0, const float* b1, long ld1,
                                                    const RowLin& r1, int row0, int L) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int id = threadIdx.x + i * AS_THREADS;
      const int rr = id / PR, c = id - rr * PR;
      const int r = row0 + rr;
      x.a[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      x.b[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < L) {
        x.a[i] = *reinterpret_cast<const float4*>(b0 + lin_row(r0, r) * ld0 + c * 4);
        x.b[i] = *reinterpret_cast<const float4*>(b1 + lin_row(r1, r) * ld1 + c * 4);
      }
    }
  }
  static __device__ __forceinline__ void chunk_store(const Pre& x, float* t0, float* t1) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int id = threadIdx.x + i * AS_THREADS;
      const int rr = id / PR, c = id - rr * PR;
      const int off = rr * LD + c * 4;
      *reinterpret_cast<float4*>(t0 + off) = x.a[i];
      *reinterpret_cast<float4*>(t1 + off) = x.b[i];
    }
  }

  // A row's HD columns, this lane's half: f[4 g + j] = column 8 g + 4 (lane >> 5) + j.
  // (A plain array, not a struct around one: with the struct the head_dim-64 kernels zero their accumulators in 32-bit moves.)
  typedef float Frag[FR];

  // This lane's half of row `row` (rows beyond nvalid read row nvalid - 1: finite operands for a lane that is never stored).
  static __device__ __forceinline__ void load_frag(Frag& f, const float* base, long ld, int col0, const RowLin& rl, int row, int nvalid,
                                                   int lane) {
    const int rc = row < nvalid ? row : nvalid - 1;
    const float* src = base + lin_row(rl, rc) * ld + col0 + 4 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const float4 v = *reinterpret_cast<const float4*>(src + 8 * g);
      f[4 * g] = v.x; f[4 * g + 1] = v.y; f[4 * g + 2] = v.z; f[4 * g + 3] = v.w;
    }
  }
  static __device__ __forceinline__ float frag_dot(const Frag& a, const Frag& b) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < FR; ++e) s = fmaf(a[e], b[e], s);
    return s;
  }

  // Per-lane LDS offsets (floats) of the two readers; the tile row (a multiple of 32) adds an immediate.
  struct Lane { int rows, cols; };
  static __device__ __forceinline__ Lane make_lane(int lane) {
    return Lane{(lane & 31) * LD + 4 * (lane >> 5), 4 * (lane >> 5) * LD + (lane & 31)};
  }

  // C[i][j] = sum_d tile[row0 + i][d] * b_j[d]: 32 tile rows against the lanes' own row fragments (HD / 2 MFMAs).
  static __device__ __forceinline__ f32x16 scores(const float* t, int row0, const Frag& b, const Lane& ln) {
    f32x16 acc;
    zero16(acc);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const float4 a = *reinterpret_cast<const float4*>(t + ln.rows + row0 * LD + 8 * g);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[4 * g], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[4 * g + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[4 * g + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[4 * g + 3], acc, 0, 0, 0);
    }
    return acc;
  }

  // acc[n][d][j] += sum_i tile[row0 + i][32 n + d] * c[i][j] with c in the accumulator layout of scores() (16 MFMAs per tile n).
  static __device__ __forceinline__ void accum(f32x16 (&acc)[NT], const float* t, int row0, const f32x16& c, const Lane& ln) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* src = t + ln.cols + (row0 + (r & 3) + 8 * (r >> 2)) * LD;
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(src[32 * n], c[r], acc[n], 0, 0, 0);
    }
  }

  // The dk / dv products of one 32-query tile, S -> P -> dv -> dP -> dS -> dk: S and dP are never live together.
  static __device__ __forceinline__ void dkv_tile(f32x16 (&dk)[NT], f32x16 (&dv)[NT], const float* Qs, const float* Os, const float* Ls,
                                                  const float* Ds, int row0, const Frag& kf, const Frag& vf, float c2, const Lane& ln,
                                                  int lane) {
    f32x16 pr = scores(Qs, row0, kf, ln);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 l4 = *reinterpret_cast<const float4*>(Ls + row0 + 8 * g + 4 * (lane >> 5));
      pr[4 * g] = __builtin_amdgcn_exp2f(fmaf(pr[4 * g], c2, -l4.x));
      pr[4 * g + 1] = __builtin_amdgcn_exp2f(fmaf(pr[4 * g + 1], c2, -l4.y));
      pr[4 * g + 2] = __builtin_amdgcn_exp2f(fmaf(pr[4 * g + 2], c2, -l4.z));
      pr[4 * g + 3] = __builtin_amdgcn_exp2f(fmaf(pr[4 * g + 3], c2, -l4.w));
    }
    accum(dv, Os, row0, pr, ln);
    f32x16 ds = scores(Os, row0, vf, ln);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 d4 = *reinterpret_cast<const float4*>(Ds + row0 + 8 * g + 4 * (lane >> 5));
      ds[4 * g] = pr[4 * g] * (ds[4 * g] - d4.x);          // the softmax scale is applied once to dk at the store
      ds[4 * g + 1] = pr[4 * g + 1] * (ds[4 * g + 1] - d4.y);
      ds[4 * g + 2] = pr[4 * g + 2] * (ds[4 * g + 2] - d4.z);
      ds[4 * g + 3] = pr[4 * g + 3] * (ds[4 * g + 3] - d4.w);
    }
    accum(dk, Qs, row0, ds, ln);
  }

  // Store a [32 x HD] result held transposed (lane & 31 = row, registers = HD columns in NT C tiles) through a wave-private LDS
  // tile, so that global memory sees whole rows: HD / 4 lanes x 16 B per row.
  // ptr_of_row(r) -> destination of tile row r (HD floats), or nullptr for a padded row.
  template <typename PtrFn>
  static __device__ __forceinline__ void store_rows(float* stg, const f32x16 (&acc)[NT], float mul, int lane, PtrFn ptr_of_row) {
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(stg + (lane & 31) * LD + n * 32 + 8 * g + 4 * (lane >> 5)) =
            make_float4(acc[n][4 * g] * mul, acc[n][4 * g + 1] * mul, acc[n][4 * g + 2] * mul, acc[n][4 * g + 3] * mul);
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < 32 * PR / 64; ++i) {
      const unsigned id = i * 64 + (unsigned)lane;     // unsigned: id / PR is one shift at 32, 64 and 128, no sign fix per row
      const int r = id / PR, c = id - r * PR;
      const float4 v = *reinterpret_cast<const float4*>(stg + r * LD + c * 4);
      float* dst = ptr_of_row(r);
      if (dst) *reinterpret_cast<float4*>(dst + c * 4) = v;
    }
    wave_lds_sync();
  }
};

}  // namespace vtx
