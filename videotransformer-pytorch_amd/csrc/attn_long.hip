// attn_long.hip -- bf16 MFMA attention core for sequences of more than 256 tokens, head_dim 64
// (joint space-time attention of TimeSformer / ViViT: L = 1 + 196 * 8 = 1569; the divided spatial attention of a
// 448^2 model: L = 785).  Both VTX_ATTN_CONTIG and VTX_ATTN_SPACE, forward and backward.
//
// The formulation is the one of attn_mfma.hip (see there for the layout argument; the helpers live in attn_common.h):
// scores are computed TRANSPOSED with v_mfma_f32_32x32x16_bf16 so that a lane owns a query column (forward, dq) or a
// key column (dk / dv), and the transposed operands come out of swizzled [rows][64] LDS tiles through
// ds_read_b64_tr_b16.  What differs is that a sequence no longer fits the LDS, so the structure is the chunk streaming
// of xattn_mfma.hip:
//   forward, dq : a workgroup of 4 waves owns 128 queries of one (sequence, head), a wave 32 of them (fragments in
//                 registers); K and V stream through LDS in chunks of 128 keys.  Forward: online softmax per chunk
//                 (running max m of the raw scores, sum l, rescale of the O^T accumulator).  dq: P recomputed from the
//                 saved lse; delta = rowsum(dO * O) is computed in the prologue and written for the dk / dv kernel.
//   dk / dv     : a workgroup owns 128 keys (a wave: one 32-key tile) and streams ALL queries of its sequence
//                 (Q, dO, lse, delta) in chunks of 128.  One workgroup sees every query of its keys: no partial sums,
//                 no workspace, no atomics, a fixed summation order -- two runs are bit-identical.
// Chunks are double buffered: the global loads of chunk c + 1 are issued into registers before the products of chunk c
// and written to the other LDS stage behind them, one workgroup barrier per chunk.  2 stages x 2 tiles x 16 KiB = 64 KiB
// (+ 2 KiB of lse / delta in the dk / dv kernel), two workgroups per CU.  The row-store staging tiles reuse the stages
// after the last chunk.  Grid: S * ceil(L / 128) x H workgroups for each of the three kernels.
//
// Masking: keys >= L of the last chunk score -1e30 before the max (P = 0; every chunk holds at least one real key, so
// a chunk maximum is always finite and exp2(m_old - m_new) never sees inf - inf); query rows >= L keep to their lane
// (operands clamped to row L - 1) and are never stored; in the dk / dv kernel padded query rows carry lse = +1e30, P = 0.
// FLOPs per (sequence, head): forward 4 L^2 64, backward 10 L^2 64 (+ 4 L^2 64 recomputed scores).
#include "attn_common.h"

namespace vtx {

namespace al {

constexpr int THREADS = 256;
constexpr int CHUNK = 128;                       // rows of the streamed operands per LDS stage (4 tiles of 32)
constexpr int TILE = CHUNK * 64;                 // elements of one [CHUNK][64] bf16 tile (16 KiB)
constexpr int STAGE = 2 * TILE;                  // two tiles per stage
constexpr int PER = CHUNK * 8 / THREADS;         // 16-byte pieces of one tile per thread

// Rows row0 .. row0 + CHUNK - 1 of two operands of one sequence, in flight between two chunks.
struct Pre { uint4 a[PER], b[PER]; };

// Issue the loads of one chunk (rows >= L read as zero; a chunk wholly beyond L issues nothing).
__device__ inline void chunk_load(Pre& x, const bf16raw* b0, long ld0, const RowLin& r0, const bf16raw* b1, long ld1, const RowLin& r1,
                                  int row0, int L) {
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int id = threadIdx.x + i * THREADS;
    const int r = row0 + (id >> 3), c = id & 7;
    x.a[i] = make_uint4(0, 0, 0, 0);
    x.b[i] = make_uint4(0, 0, 0, 0);
    if (r < L) {
      x.a[i] = *reinterpret_cast<const uint4*>(b0 + lin_row(r0, r) * ld0 + c * 8);
      x.b[i] = *reinterpret_cast<const uint4*>(b1 + lin_row(r1, r) * ld1 + c * 8);
    }
  }
}
__device__ inline void chunk_store(const Pre& x, bf16raw* t0, bf16raw* t1) {
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int id = threadIdx.x + i * THREADS;
    const int r = id >> 3, c = id & 7;
    const int off = r * 64 + ((c ^ sw_of(r)) << 3);
    *reinterpret_cast<uint4*>(t0 + off) = x.a[i];
    *reinterpret_cast<uint4*>(t1 + off) = x.b[i];
  }
}

// blockIdx.x -> (sequence, 128-row block of that sequence)
__device__ inline void who(const AttnP& p, int& s, int& blk) {
  const int nb = (p.L + CHUNK - 1) / CHUNK;
  s = blockIdx.x / nb;
  blk = blockIdx.x - s * nb;
}

}  // namespace al

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(al::THREADS, 2) void attn_fwd_long_kernel(AttnP p, const bf16raw* __restrict__ qkv,
                                                                       bf16raw* __restrict__ out, float* __restrict__ lse) {
  using namespace al;
  constexpr int KC = CHUNK / 32;
  extern __shared__ __attribute__((aligned(16))) char sm_raw[];
  bf16raw* sm = reinterpret_cast<bf16raw*>(sm_raw);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, D = p.H * 64;
  int s, qb;
  who(p, s, qb);
  const int q0 = qb * CHUNK + wave * 32, qi = q0 + (lane & 31);
  const bool active = q0 < p.L;                    // wave-uniform; an idle wave still fills and meets the barriers
  const RowLin li = lin_in(p, s), lo = lin_out(p, s);
  const bf16raw* kb = qkv + D + h * 64;
  const bf16raw* vb = qkv + 2 * D + h * 64;
  bf16x8 qf[4];
  load_row_frags(qf, qkv, p.ld_qkv, h * 64, li, qi, p.L, lane);
  Pre pre;
  chunk_load(pre, kb, p.ld_qkv, li, vb, p.ld_qkv, li, 0, p.L);
  chunk_store(pre, sm, sm + TILE);
  __syncthreads();
  const FragOff fo = make_frag_off(lane);
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float c2 = p.scale * LOG2E;
  f32x16 acc[2];
  zero16(acc[0]);
  zero16(acc[1]);
  float m = -1e30f, l = 0.f;                       // running max of the RAW scores (scale > 0)
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const bf16raw* Ks = sm + (c & 1) * STAGE;
    const bf16raw* Vs = Ks + TILE;
    chunk_load(pre, kb, p.ld_qkv, li, vb, p.ld_qkv, li, (c + 1) * CHUNK, p.L);
    if (active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
      f32x16 st[KC];                               // (tiles beyond nt stay undefined: every use below is guarded)
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) {
          st[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Ks, t * 32, 0, fo), qf[0], zero, 0, 0, 0);
#pragma unroll
          for (int ks = 1; ks < 4; ++ks)
            st[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Ks, t * 32, ks, fo), qf[ks], st[t], 0, 0, 0);
        }
      float bm = -1e30f;
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) {
          if (t * 32 + 32 > nrows) {               // the tile that holds padded keys
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (t * 32 + crow(r, lane) >= nrows) st[t][r] = -1e30f;
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) bm = fmaxf(bm, st[t][r]);
        }
      bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
      const float mn = fmaxf(m, bm);
      const float alpha = __builtin_amdgcn_exp2f((m - mn) * c2);
      m = mn;
      const float mc = mn * c2;
      float bl = 0.f;
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) {
#pragma unroll
          for (int r = 0; r < 16; ++r) { const float e = __builtin_amdgcn_exp2f(fmaf(st[t][r], c2, -mc)); st[t][r] = e; bl += e; }
        }
      bl += __shfl_xor(bl, 32, 64);
      l = l * alpha + bl;
      if (c > 0) {
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[n2][r] *= alpha;
      }
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) {
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            float pf[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = st[t][8 * s2 + j];
            const bf16x8 pb = pack8(pf);
#pragma unroll
            for (int n2 = 0; n2 < 2; ++n2)
              acc[n2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_o(Vs, t * 32 + 16 * s2, n2, fo), pb, acc[n2], 0, 0, 0);
          }
        }
    }
    if (c + 1 < nch) {
      bf16raw* nx = sm + ((c + 1) & 1) * STAGE;    // last read in iteration c - 1, behind that iteration's barrier
      chunk_store(pre, nx, nx + TILE);
    }
    __syncthreads();
  }
  if (!active) return;
  bf16raw* stg = sm + wave * MA_STAGE_ELEMS;       // every wave is past the last chunk: the stages are free
  store_rows_T(stg, acc, 1.0f / l, lane, [&](int r) -> bf16raw* {
    const int qq = q0 + r;
    return qq < p.L ? out + lin_row(lo, qq) * p.ld_out + h * 64 : nullptr;
  });
  if (qi < p.L && lane < 32) lse[((long)s * p.H + h) * p.L + qi] = (m * c2) * LN2 + __logf(l);
}

// ------------------------------------------------------------------------------------------------ backward: dq (+ delta)
__global__ __launch_bounds__(al::THREADS, 2) void attn_bwd_dq_long_kernel(AttnP p, const bf16raw* __restrict__ qkv,
                                                                          const bf16raw* __restrict__ o, const bf16raw* __restrict__ dout,
                                                                          const float* __restrict__ lse, float* __restrict__ delta,
                                                                          bf16raw* __restrict__ dqkv, bf16raw* __restrict__ dqkv_cls) {
  using namespace al;
  constexpr int KC = CHUNK / 32;
  extern __shared__ __attribute__((aligned(16))) char sm_raw[];
  bf16raw* sm = reinterpret_cast<bf16raw*>(sm_raw);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, D = p.H * 64;
  int s, qb;
  who(p, s, qb);
  const int q0 = qb * CHUNK + wave * 32, qi = q0 + (lane & 31);
  const bool active = q0 < p.L;
  const RowLin li = lin_in(p, s), lo = lin_out(p, s);
  const bf16raw* kb = qkv + D + h * 64;
  const bf16raw* vb = qkv + 2 * D + h * 64;
  bf16x8 qf[4], df[4];
  float dl = 0.f;                                  // delta = rowsum(dO * O): this lane's 32 of the row's 64 columns
  {
    bf16x8 of[4];
    load_row_frags(qf, qkv, p.ld_qkv, h * 64, li, qi, p.L, lane);
    load_row_frags(df, dout, p.ld_dout, h * 64, lo, qi, p.L, lane);
    load_row_frags(of, o, p.ld_out, h * 64, lo, qi, p.L, lane);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) dl = frag_dot2(df[ks], of[ks], dl);
  }
  dl += __shfl_xor(dl, 32, 64);
  float l2 = 0.f;
  if (qi < p.L) {
    const long lidx = ((long)s * p.H + h) * p.L + qi;
    l2 = lse[lidx] * LOG2E;
    if (lane < 32) delta[lidx] = dl;
  }
  Pre pre;
  chunk_load(pre, kb, p.ld_qkv, li, vb, p.ld_qkv, li, 0, p.L);
  chunk_store(pre, sm, sm + TILE);
  __syncthreads();
  const FragOff fo = make_frag_off(lane);
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float c2 = p.scale * LOG2E;
  f32x16 acc[2];
  zero16(acc[0]);
  zero16(acc[1]);
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const bf16raw* Ks = sm + (c & 1) * STAGE;
    const bf16raw* Vs = Ks + TILE;
    chunk_load(pre, kb, p.ld_qkv, li, vb, p.ld_qkv, li, (c + 1) * CHUNK, p.L);
    if (active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) {
          f32x16 st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Ks, t * 32, 0, fo), qf[0], zero, 0, 0, 0);
          f32x16 dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Vs, t * 32, 0, fo), df[0], zero, 0, 0, 0);
#pragma unroll
          for (int ks = 1; ks < 4; ++ks) {
            st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Ks, t * 32, ks, fo), qf[ks], st, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Vs, t * 32, ks, fo), df[ks], dp, 0, 0, 0);
          }
          // dS = P (dP - delta); the softmax scale is applied once to dq at the store.  Padded keys have zero K rows
          // (they add nothing to dq); their probability is masked so that the bf16 pack stays clean.
          float ds[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) ds[r] = __builtin_amdgcn_exp2f(fmaf(st[r], c2, -l2)) * (dp[r] - dl);
          if (t * 32 + 32 > nrows) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (t * 32 + crow(r, lane) >= nrows) ds[r] = 0.f;
          }
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const bf16x8 db = pack8(ds + 8 * s2);
#pragma unroll
            for (int n2 = 0; n2 < 2; ++n2)
              acc[n2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_o(Ks, t * 32 + 16 * s2, n2, fo), db, acc[n2], 0, 0, 0);
          }
        }
    }
    if (c + 1 < nch) {
      bf16raw* nx = sm + ((c + 1) & 1) * STAGE;
      chunk_store(pre, nx, nx + TILE);
    }
    __syncthreads();
  }
  if (!active) return;
  bf16raw* stg = sm + wave * MA_STAGE_ELEMS;
  store_rows_T(stg, acc, p.scale, lane, [&](int r) -> bf16raw* {
    const int qq = q0 + r;
    if (qq >= p.L) return nullptr;
    return (p.mode == VTX_ATTN_SPACE && qq == 0) ? dqkv_cls + (long)s * p.ld_dqkv + h * 64
                                                  : dqkv + lin_row(li, qq) * p.ld_dqkv + h * 64;
  });
}

// ------------------------------------------------------------------------------------------------ backward: dk, dv
// Lanes = keys: wave w of the workgroup of key block kb owns the key tile kb * 4 + w and walks ALL queries of the sequence.
__global__ __launch_bounds__(al::THREADS, 2) void attn_bwd_dkv_long_kernel(AttnP p, const bf16raw* __restrict__ qkv,
                                                                           const bf16raw* __restrict__ dout, const float* __restrict__ lse,
                                                                           const float* __restrict__ delta, bf16raw* __restrict__ dqkv,
                                                                           bf16raw* __restrict__ dqkv_cls) {
  using namespace al;
  constexpr int QC = CHUNK / 32;
  extern __shared__ __attribute__((aligned(16))) char sm_raw[];
  bf16raw* sm = reinterpret_cast<bf16raw*>(sm_raw);
  float* stats = reinterpret_cast<float*>(sm + 2 * STAGE);     // [stage][lse * log2(e) | delta][CHUNK]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, D = p.H * 64;
  int s, kblk;
  who(p, s, kblk);
  const int key0 = kblk * CHUNK + wave * 32, key = key0 + (lane & 31);
  const bool active = key0 < p.L;
  const RowLin li = lin_in(p, s), lo = lin_out(p, s);
  const bf16raw* qb = qkv + h * 64;
  const bf16raw* ob = dout + h * 64;
  const float* lb = lse + ((long)s * p.H + h) * p.L;
  const float* db = delta + ((long)s * p.H + h) * p.L;
  bf16x8 kf[4], vf[4];
  load_row_frags(kf, qkv, p.ld_qkv, D + h * 64, li, key, p.L, lane);
  load_row_frags(vf, qkv, p.ld_qkv, 2 * D + h * 64, li, key, p.L, lane);
  // thread t < 128: lse of chunk row t (scaled; +huge on padded rows -> P = 0); t >= 128: delta of chunk row t - 128
  const int srow = threadIdx.x & (CHUNK - 1);
  const bool is_lse = threadIdx.x < CHUNK;
  auto stat_load = [&](int row0) -> float {
    const int r = row0 + srow;
    if (r >= p.L) return is_lse ? 1e30f : 0.f;
    return is_lse ? lb[r] * LOG2E : db[r];
  };
  Pre pre;
  chunk_load(pre, qb, p.ld_qkv, li, ob, p.ld_dout, lo, 0, p.L);
  float sv = stat_load(0);
  chunk_store(pre, sm, sm + TILE);
  stats[threadIdx.x] = sv;
  __syncthreads();
  const FragOff fo = make_frag_off(lane);
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float c2 = p.scale * LOG2E;
  f32x16 dk[2], dv[2];
  zero16(dk[0]); zero16(dk[1]); zero16(dv[0]); zero16(dv[1]);
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const bf16raw* Qs = sm + (c & 1) * STAGE;
    const bf16raw* Os = Qs + TILE;
    const float* Ls = stats + (c & 1) * 2 * CHUNK;
    const float* Ds = Ls + CHUNK;
    chunk_load(pre, qb, p.ld_qkv, li, ob, p.ld_dout, lo, (c + 1) * CHUNK, p.L);
    sv = stat_load((c + 1) * CHUNK);
    if (active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
#pragma unroll
      for (int t = 0; t < QC; ++t)
        if (t < nt) {
          f32x16 st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Qs, t * 32, 0, fo), kf[0], zero, 0, 0, 0);
          f32x16 dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Os, t * 32, 0, fo), vf[0], zero, 0, 0, 0);
#pragma unroll
          for (int ks = 1; ks < 4; ++ks) {
            st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Qs, t * 32, ks, fo), kf[ks], st, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Os, t * 32, ks, fo), vf[ks], dp, 0, 0, 0);
          }
          // padded query rows: Ls = +huge -> P = 0; padded keys only feed dk / dv rows that are never stored
          float pr[16], ds[16];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int qrow = t * 32 + 8 * g + 4 * (lane >> 5);
            const float4 l4 = *reinterpret_cast<const float4*>(Ls + qrow);
            const float4 d4 = *reinterpret_cast<const float4*>(Ds + qrow);
            const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dvv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int r = 4 * g + j;
              const float e = __builtin_amdgcn_exp2f(fmaf(st[r], c2, -lv[j]));
              pr[r] = e;
              ds[r] = e * (dp[r] - dvv[j]);        // the softmax scale is applied once to dk at the store
            }
          }
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const bf16x8 pb = pack8(pr + 8 * s2);
            const bf16x8 dsb = pack8(ds + 8 * s2);
#pragma unroll
            for (int n2 = 0; n2 < 2; ++n2) {
              dv[n2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_o(Os, t * 32 + 16 * s2, n2, fo), pb, dv[n2], 0, 0, 0);
              dk[n2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_o(Qs, t * 32 + 16 * s2, n2, fo), dsb, dk[n2], 0, 0, 0);
            }
          }
        }
    }
    if (c + 1 < nch) {
      bf16raw* nx = sm + ((c + 1) & 1) * STAGE;
      chunk_store(pre, nx, nx + TILE);
      stats[((c + 1) & 1) * 2 * CHUNK + threadIdx.x] = sv;
    }
    __syncthreads();
  }
  if (!active) return;
  bf16raw* stg = sm + wave * MA_STAGE_ELEMS;
  auto base_of = [&](int r) -> bf16raw* {
    const int kk = key0 + r;
    if (kk >= p.L) return nullptr;
    return (p.mode == VTX_ATTN_SPACE && kk == 0) ? dqkv_cls + (long)s * p.ld_dqkv : dqkv + lin_row(li, kk) * p.ld_dqkv;
  };
  store_rows_T(stg, dk, p.scale, lane, [&](int r) -> bf16raw* { bf16raw* b = base_of(r); return b ? b + D + h * 64 : nullptr; });
  store_rows_T(stg, dv, 1.0f, lane, [&](int r) -> bf16raw* { bf16raw* b = base_of(r); return b ? b + 2 * D + h * 64 : nullptr; });
}

// host-side launchers used by attn.hip's entry points --------------------------------------
bool attn_long_eligible(int dtype, int L, int hd) { return dtype == VTX_BF16 && hd == 64 && L > 32 * MA_MAXT; }

constexpr size_t AL_LDS_KV = (size_t)2 * al::STAGE * 2;                             // 64 KiB: the default limit, no opt-in
constexpr size_t AL_LDS_DKV = AL_LDS_KV + (size_t)2 * 2 * al::CHUNK * sizeof(float);   // + lse / delta of both stages

static dim3 long_grid(const AttnP& p) { return dim3((unsigned)p.S * (unsigned)cdiv(p.L, al::CHUNK), p.H); }

int attn_fwd_long_launch(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st) {
  hipLaunchKernelGGL(attn_fwd_long_kernel, long_grid(p), dim3(al::THREADS), AL_LDS_KV, st, p, (const bf16raw*)qkv, (bf16raw*)out, lse);
  return check_launch("attn_fwd_long");
}

int attn_bwd_long_launch(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                         void* dqkv_cls, hipStream_t st) {
  hipLaunchKernelGGL(attn_bwd_dq_long_kernel, long_grid(p), dim3(al::THREADS), AL_LDS_KV, st, p, (const bf16raw*)qkv, (const bf16raw*)o,
                     (const bf16raw*)dout, lse, delta, (bf16raw*)dqkv, (bf16raw*)dqkv_cls);
  int rc = check_launch("attn_bwd_dq_long");
  if (rc) return rc;
  static std::atomic<unsigned long long> seen{0};  // > 64 KiB of dynamic LDS needs an explicit opt-in, once per device
  if (first_launch_on_device(seen))
    hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_dkv_long_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL(attn_bwd_dkv_long_kernel, long_grid(p), dim3(al::THREADS), AL_LDS_DKV, st, p, (const bf16raw*)qkv,
                     (const bf16raw*)dout, lse, delta, (bf16raw*)dqkv, (bf16raw*)dqkv_cls);
  return check_launch("attn_bwd_dkv_long");
}

}  // namespace vtx
