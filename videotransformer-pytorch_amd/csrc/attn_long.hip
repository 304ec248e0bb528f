// attn_long.hip -- bf16 MFMA attention core for sequences of more than 256 tokens, head_dim 64
// (joint space-time attention of TimeSformer / ViViT: L = 1 + 196 * 8 = 1569; the divided spatial attention of a
// 448^2 model: L = 785).  Both VTX_ATTN_CONTIG and VTX_ATTN_SPACE, forward and backward.
//
// The structure is the chunk streaming of attn_stream.h (the three kernels live there); this file is its bf16 tile policy.
// The formulation is the one of attn_mfma.hip (see there for the layout argument; the helpers live in attn_common.h):
// scores are computed with v_mfma_f32_32x32x16_bf16, and the transposed operands come out of swizzled [rows][64] LDS tiles
// through ds_read_b64_tr_b16.  K and V (Q and dO in the dk / dv kernel) stream in chunks of 128 rows:
// 2 stages x 2 tiles x 16 KiB = 64 KiB (+ 2 KiB of lse / delta in the dk / dv kernel).
#include "attn_stream.h"

namespace vtx {

struct LongTiles {
  typedef bf16raw elem;
  static constexpr int CHUNK = 128;                // rows of the streamed operands per LDS stage (4 tiles of 32)
  static constexpr int TILE = CHUNK * 64;          // elements of one [CHUNK][64] bf16 tile (16 KiB)
  static constexpr int STAGE = 2 * TILE;           // two tiles per stage
  static constexpr int PER = CHUNK * 8 / AS_THREADS;   // 16-byte pieces of one tile per thread
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
      const int r = row0 + (id >> 3), c = id & 7;
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
      const int r = id >> 3, c = id & 7;
      const int off = r * 64 + ((c ^ sw_of(r)) << 3);
      *reinterpret_cast<uint4*>(t0 + off) = x.a[i];
      *reinterpret_cast<uint4*>(t1 + off) = x.b[i];
    }
  }

  typedef bf16x8 Frag[4];
  static __device__ __forceinline__ void load_frag(Frag& f, const bf16raw* base, long ld, int col0, const RowLin& rl, int row, int nvalid,
                                                   int lane) {
    load_row_frags(f, base, ld, col0, rl, row, nvalid, lane);
  }
  static __device__ __forceinline__ float frag_dot(const Frag& a, const Frag& b) {
    float s = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) s = frag_dot2(a[ks], b[ks], s);
    return s;
  }

  typedef FragOff Lane;
  static __device__ __forceinline__ Lane make_lane(int lane) { return make_frag_off(lane); }

  static __device__ __forceinline__ f32x16 scores(const bf16raw* t, int row0, const Frag& b, const Lane& fo) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(t, row0, 0, fo), b[0], zero, 0, 0, 0);
#pragma unroll
    for (int ks = 1; ks < 4; ++ks) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(t, row0, ks, fo), b[ks], st, 0, 0, 0);
    return st;
  }
  static __device__ __forceinline__ void accum(f32x16 (&acc)[2], const bf16raw* t, int row0, const f32x16& c, const Lane& fo) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      float pf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = c[8 * s2 + j];
      const bf16x8 pb = pack8(pf);
#pragma unroll
      for (int n2 = 0; n2 < 2; ++n2)
        acc[n2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_o(t, row0 + 16 * s2, n2, fo), pb, acc[n2], 0, 0, 0);
    }
  }
  // The dk / dv products of one 32-query tile: the S and dP chains interleaved, then dv and dk fed together.
  static __device__ __forceinline__ void dkv_tile(f32x16 (&dk)[2], f32x16 (&dv)[2], const bf16raw* Qs, const bf16raw* Os, const float* Ls,
                                                  const float* Ds, int row0, const Frag& kf, const Frag& vf, float c2, const Lane& fo,
                                                  int lane) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Qs, row0, 0, fo), kf[0], zero, 0, 0, 0);
    f32x16 dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Os, row0, 0, fo), vf[0], zero, 0, 0, 0);
#pragma unroll
    for (int ks = 1; ks < 4; ++ks) {
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Qs, row0, ks, fo), kf[ks], st, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Os, row0, ks, fo), vf[ks], dp, 0, 0, 0);
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
      for (int n2 = 0; n2 < 2; ++n2) {
        dv[n2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_o(Os, row0 + 16 * s2, n2, fo), pb, dv[n2], 0, 0, 0);
        dk[n2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_o(Qs, row0 + 16 * s2, n2, fo), dsb, dk[n2], 0, 0, 0);
      }
    }
  }
  template <typename PtrFn>
  static __device__ __forceinline__ void store_rows(bf16raw* stg, const f32x16 (&acc)[2], float mul, int lane, PtrFn ptr_of_row) {
    store_rows_T(stg, acc, mul, lane, ptr_of_row);
  }
};

__global__ __launch_bounds__(AS_THREADS, 2) void attn_fwd_long_kernel(AttnP p, const bf16raw* __restrict__ qkv,
                                                                      bf16raw* __restrict__ out, float* __restrict__ lse) {
  stream_fwd<LongTiles>(p, qkv, out, lse);
}
__global__ __launch_bounds__(AS_THREADS, 2) void attn_bwd_dq_long_kernel(AttnP p, const bf16raw* __restrict__ qkv,
                                                                         const bf16raw* __restrict__ o, const bf16raw* __restrict__ dout,
                                                                         const float* __restrict__ lse, float* __restrict__ delta,
                                                                         bf16raw* __restrict__ dqkv, bf16raw* __restrict__ dqkv_cls) {
  stream_bwd_dq<LongTiles>(p, qkv, o, dout, lse, delta, dqkv, dqkv_cls);
}
__global__ __launch_bounds__(AS_THREADS, 2) void attn_bwd_dkv_long_kernel(AttnP p, const bf16raw* __restrict__ qkv,
                                                                          const bf16raw* __restrict__ dout, const float* __restrict__ lse,
                                                                          const float* __restrict__ delta, bf16raw* __restrict__ dqkv,
                                                                          bf16raw* __restrict__ dqkv_cls) {
  stream_bwd_dkv<LongTiles>(p, qkv, dout, lse, delta, dqkv, dqkv_cls);
}

// host-side launchers used by attn.hip's entry points --------------------------------------
bool attn_long_eligible(int dtype, int L, int hd) { return dtype == VTX_BF16 && hd == 64 && L > 32 * MA_MAXT; }

int attn_fwd_long_launch(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st) {
  return stream_fwd_launch<LongTiles, attn_fwd_long_kernel>("attn_fwd_long", p, qkv, out, lse, st);
}

int attn_bwd_long_launch(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                         void* dqkv_cls, hipStream_t st) {
  return stream_bwd_launch<LongTiles, attn_bwd_dq_long_kernel, attn_bwd_dkv_long_kernel>("attn_bwd_dq_long", "attn_bwd_dkv_long", p, qkv, o,
                                                                                         dout, lse, delta, dqkv, dqkv_cls, st);
}

}  // namespace vtx
