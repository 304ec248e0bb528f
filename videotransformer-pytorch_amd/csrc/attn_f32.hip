// attn_f32.hip -- exact-fp32 MFMA attention core for fp32 inputs, head_dim 64, more than 32 tokens per sequence
// (joint space-time: 1569; spatial: 197 at 224^2, 785 at 448^2; ViViT encoders).  VTX_ATTN_CONTIG and VTX_ATTN_SPACE,
// forward and backward.  Every product runs on v_mfma_f32_32x32x2_f32: fp32 operands, an fma chain with fp32 rounding after
// every step -- the same arithmetic as the VALU kernels of attn.hip in another summation order.  Scores, probabilities and
// accumulators stay fp32 registers from the first product to the store: no value is ever rounded to bf16.
//
// The structure is the chunk streaming of attn_stream.h (the three kernels, the masking and the launchers live there) in
// chunks of 64 rows; this file is its fp32 tile policy.
// Operands.  A 32x32x2 fp32 MFMA takes ONE dword of A and one of B per lane (lane l: A[l & 31][l >> 5], B[l >> 5][l & 31]):
//   scores, transposed (S^T = K Q^T; dP^T = V dO^T; in the dk / dv kernel S = Q K^T, dP = dO V^T): A = a row of the LDS
//     tile per lane, read four columns at a time (ds_read_b128 feeds four MFMAs); B = the lane's own row fragment.  The k
//     index of MFMA (g, j) is column 8 g + 4 (l >> 5) + j for both operands -- any order of the 64 columns is a dot product.
//   accumulation (O^T += V^T P^T, dq^T += K^T dS^T, dv^T += dO^T P, dk^T += Q^T dS): B = the score tile exactly as the
//     MFMA left it (register r of lane l holds row crow(r, l) = (r & 3) + 8 (r >> 2) + 4 (l >> 5) of column l & 31), so
//     MFMA r contracts the two rows crow(r, 0) and crow(r, 32); A = those rows of the LDS tile, column (l & 31) + 32 n2
//     (ds_read_b32, a whole row per half-wave: conflict-free).  P never leaves its registers.
// LDS rows are padded to 68 floats: the 16 lanes of a ds_read_b128 group read 16 different rows, 68 * 4 B puts them on 16
// different 16-byte slots of the 256-byte bank row.  A stage is two [64][68] fp32 tiles (34 KiB); two stages = 68 KiB
// (+ 1 KiB of lse / delta in the dk / dv kernel).  In the dq kernel a padded key's dS multiplies a zero K row and is not masked.
#include "attn_stream.h"

namespace vtx {

struct F32Tiles {
  typedef float elem;
  static constexpr int CHUNK = 64;                 // rows of the streamed operands per LDS stage (2 tiles of 32)
  static constexpr int LD = 68;                    // floats per LDS row (64 + 4: see the bank argument above)
  static constexpr int TILE = CHUNK * LD;          // floats of one [CHUNK][LD] tile (17 KiB)
  static constexpr int STAGE = 2 * TILE;           // two tiles per stage
  static constexpr int PER = CHUNK * 16 / AS_THREADS;  // 16-byte pieces of one tile per thread
  static constexpr int STG = 32 * LD;              // per-wave [32][LD] staging tile for row stores
  static constexpr bool MASK_PADDED_DS = false;

  struct Pre { float4 a[PER], b[PER]; };           // rows row0 .. row0 + CHUNK - 1 of two operands, in flight between two chunks

  // Issue the loads of one chunk (rows >= L read as zero; a chunk wholly beyond L issues nothing).
  static __device__ __forceinline__ void chunk_load(Pre& x, const float* b0, long ld0, const RowLin& r0, const float* b1, long ld1,
                                                    const RowLin& r1, int row0, int L) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int id = threadIdx.x + i * AS_THREADS;
      const int r = row0 + (id >> 4), c = id & 15;
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
      const int off = (id >> 4) * LD + (id & 15) * 4;
      *reinterpret_cast<float4*>(t0 + off) = x.a[i];
      *reinterpret_cast<float4*>(t1 + off) = x.b[i];
    }
  }

  typedef float Frag[32];                          // a row's 64 columns, this lane's half: [4 g + j] = column 8 g + 4 (lane >> 5) + j

  // This lane's half of row `row` (rows beyond nvalid read row nvalid - 1: finite operands for a lane that is never stored).
  static __device__ __forceinline__ void load_frag(Frag& f, const float* base, long ld, int col0, const RowLin& rl, int row, int nvalid,
                                                   int lane) {
    const int rc = row < nvalid ? row : nvalid - 1;
    const float* src = base + lin_row(rl, rc) * ld + col0 + 4 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const float4 v = *reinterpret_cast<const float4*>(src + 8 * g);
      f[4 * g] = v.x; f[4 * g + 1] = v.y; f[4 * g + 2] = v.z; f[4 * g + 3] = v.w;
    }
  }
  static __device__ __forceinline__ float frag_dot(const Frag& a, const Frag& b) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 32; ++e) s = fmaf(a[e], b[e], s);
    return s;
  }

  // Per-lane LDS offsets (floats) of the two readers; the tile row (a multiple of 32) adds an immediate.
  struct Lane { int rows, cols; };
  static __device__ __forceinline__ Lane make_lane(int lane) {
    return Lane{(lane & 31) * LD + 4 * (lane >> 5), 4 * (lane >> 5) * LD + (lane & 31)};
  }

  // C[i][j] = sum_d tile[row0 + i][d] * b_j[d]: 32 tile rows against the lanes' own row fragments (32 MFMAs).
  static __device__ __forceinline__ f32x16 scores(const float* t, int row0, const Frag& b, const Lane& ln) {
    f32x16 acc;
    zero16(acc);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const float4 a = *reinterpret_cast<const float4*>(t + ln.rows + row0 * LD + 8 * g);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[4 * g], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[4 * g + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[4 * g + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[4 * g + 3], acc, 0, 0, 0);
    }
    return acc;
  }

  // acc[n2][d][j] += sum_i tile[row0 + i][32 n2 + d] * c[i][j] with c in the accumulator layout of scores() (32 MFMAs).
  static __device__ __forceinline__ void accum(f32x16 (&acc)[2], const float* t, int row0, const f32x16& c, const Lane& ln) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* src = t + ln.cols + (row0 + (r & 3) + 8 * (r >> 2)) * LD;
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(src[0], c[r], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(src[32], c[r], acc[1], 0, 0, 0);
    }
  }

  // The dk / dv products of one 32-query tile, S -> P -> dv -> dP -> dS -> dk: S and dP are never live together.
  static __device__ __forceinline__ void dkv_tile(f32x16 (&dk)[2], f32x16 (&dv)[2], const float* Qs, const float* Os, const float* Ls,
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

  // Store a [32 x 64] result held transposed (lane & 31 = row, registers = 64 columns in two C tiles) through a wave-private
  // LDS tile, so that global memory sees whole 256-byte rows: 16 lanes x 16 B, 4 rows per instruction.
  // ptr_of_row(r) -> destination of tile row r (64 floats), or nullptr for a padded row.
  template <typename PtrFn>
  static __device__ __forceinline__ void store_rows(float* stg, const f32x16 (&acc)[2], float mul, int lane, PtrFn ptr_of_row) {
#pragma unroll
    for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(stg + (lane & 31) * LD + n2 * 32 + 8 * g + 4 * (lane >> 5)) =
            make_float4(acc[n2][4 * g] * mul, acc[n2][4 * g + 1] * mul, acc[n2][4 * g + 2] * mul, acc[n2][4 * g + 3] * mul);
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = i * 4 + (lane >> 4), c = lane & 15;
      const float4 v = *reinterpret_cast<const float4*>(stg + r * LD + c * 4);
      float* dst = ptr_of_row(r);
      if (dst) *reinterpret_cast<float4*>(dst + c * 4) = v;
    }
    wave_lds_sync();
  }
};

__global__ __launch_bounds__(AS_THREADS, 2) void attn_fwd_f32_kernel(AttnP p, const float* __restrict__ qkv, float* __restrict__ out,
                                                                     float* __restrict__ lse) {
  stream_fwd<F32Tiles>(p, qkv, out, lse);
}
__global__ __launch_bounds__(AS_THREADS, 2) void attn_bwd_dq_f32_kernel(AttnP p, const float* __restrict__ qkv, const float* __restrict__ o,
                                                                        const float* __restrict__ dout, const float* __restrict__ lse,
                                                                        float* __restrict__ delta, float* __restrict__ dqkv,
                                                                        float* __restrict__ dqkv_cls) {
  stream_bwd_dq<F32Tiles>(p, qkv, o, dout, lse, delta, dqkv, dqkv_cls);
}
__global__ __launch_bounds__(AS_THREADS, 2) void attn_bwd_dkv_f32_kernel(AttnP p, const float* __restrict__ qkv,
                                                                         const float* __restrict__ dout, const float* __restrict__ lse,
                                                                         const float* __restrict__ delta, float* __restrict__ dqkv,
                                                                         float* __restrict__ dqkv_cls) {
  stream_bwd_dkv<F32Tiles>(p, qkv, dout, lse, delta, dqkv, dqkv_cls);
}

// host-side launchers used by attn.hip's entry points --------------------------------------
bool attn_f32_eligible(int dtype, int L, int hd) { return dtype == VTX_F32 && hd == 64 && L > 32; }

int attn_fwd_f32_launch(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st) {
  return stream_fwd_launch<F32Tiles, attn_fwd_f32_kernel>("attn_fwd_f32", p, qkv, out, lse, st);
}

int attn_bwd_f32_launch(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                        void* dqkv_cls, hipStream_t st) {
  return stream_bwd_launch<F32Tiles, attn_bwd_dq_f32_kernel, attn_bwd_dkv_f32_kernel>("attn_bwd_dq_f32", "attn_bwd_dkv_f32", p, qkv, o, dout,
                                                                                      lse, delta, dqkv, dqkv_cls, st);
}

}  // namespace vtx
