// attn_f32.hip -- exact-fp32 MFMA attention core for fp32 inputs, head_dim 64, more than 32 tokens per sequence
// (joint space-time: 1569; spatial: 197 at 224^2, 785 at 448^2; ViViT encoders).  VTX_ATTN_CONTIG and VTX_ATTN_SPACE,
// forward and backward.  Every product runs on v_mfma_f32_32x32x2_f32: fp32 operands, an fma chain with fp32 rounding after
// every step -- the same arithmetic as the VALU kernels of attn.hip in another summation order.  Scores, probabilities and
// accumulators stay fp32 registers from the first product to the store: no value is ever rounded to bf16.
//
// Structure: the chunk streaming of attn_long.hip with fp32 tiles.
//   forward, dq : a workgroup of 4 waves owns 128 queries of one (sequence, head), a wave 32 of them (row fragments in
//                 registers); K and V stream through LDS in chunks of 64 keys.  Forward: online softmax per chunk (running
//                 max m of the raw scores, sum l, rescale of the O^T accumulator).  dq: P recomputed from the saved lse;
//                 delta = rowsum(dO * O) is computed in the prologue and written for the dk / dv kernel.
//   dk / dv     : a workgroup owns 128 keys (a wave: 32) and streams ALL queries of its sequence (Q, dO, lse, delta) in
//                 chunks of 64: no partial sums, no workspace, no atomics, a fixed summation order -- two runs are
//                 bit-identical.
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
// (+ 1 KiB of lse / delta in the dk / dv kernel), two workgroups per CU, so one workgroup's softmax and chunk stores run
// beside the other's matrix instructions.  Chunks are double buffered: the global loads of chunk c + 1 are issued into
// registers before the products of chunk c and written to the other stage behind them, one workgroup barrier per chunk.
// The row-store staging tiles reuse the stages after the last chunk.  Grid: S * ceil(L / 128) x H for each kernel.
//
// Masking: keys >= L of the last chunk have zero K / V rows and score -1e30 before the max (P = 0 exactly; every chunk
// holds at least one real key, so a chunk maximum is finite); a 32-row tile wholly beyond L is skipped.  Query rows >= L
// keep to their lane (operands clamped to row L - 1) and are never stored.  In the dq kernel a padded key's dS multiplies
// a zero K row; in the dk / dv kernel padded query rows carry lse = +1e30 (P = 0) and zero Q / dO rows.
// FLOPs per (sequence, head): forward 4 L^2 64, backward 10 L^2 64 (+ 4 L^2 64 recomputed scores).
#include "attn_common.h"

namespace vtx {

namespace af {

constexpr int THREADS = 256;
constexpr int ROWS = 128;                        // queries (keys in the dk / dv kernel) of one workgroup: 4 waves x 32
constexpr int CHUNK = 64;                        // rows of the streamed operands per LDS stage (2 tiles of 32)
constexpr int LD = 68;                           // floats per LDS row (64 + 4: see the bank argument above)
constexpr int TILE = CHUNK * LD;                 // floats of one [CHUNK][LD] tile (17 KiB)
constexpr int STAGE = 2 * TILE;                  // two tiles per stage
constexpr int PER = CHUNK * 16 / THREADS;        // 16-byte pieces of one tile per thread
constexpr int STG = 32 * LD;                     // per-wave [32][LD] staging tile for row stores

typedef float frag[32];                          // a row's 64 columns, this lane's half: [4 g + j] = column 8 g + 4 (lane >> 5) + j

struct Pre { float4 a[PER], b[PER]; };           // rows row0 .. row0 + CHUNK - 1 of two operands, in flight between two chunks

// Issue the loads of one chunk (rows >= L read as zero; a chunk wholly beyond L issues nothing).
__device__ inline void chunk_load(Pre& x, const float* b0, long ld0, const RowLin& r0, const float* b1, long ld1, const RowLin& r1,
                                  int row0, int L) {
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int id = threadIdx.x + i * THREADS;
    const int r = row0 + (id >> 4), c = id & 15;
    x.a[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    x.b[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < L) {
      x.a[i] = *reinterpret_cast<const float4*>(b0 + lin_row(r0, r) * ld0 + c * 4);
      x.b[i] = *reinterpret_cast<const float4*>(b1 + lin_row(r1, r) * ld1 + c * 4);
    }
  }
}
__device__ inline void chunk_store(const Pre& x, float* t0, float* t1) {
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int id = threadIdx.x + i * THREADS;
    const int off = (id >> 4) * LD + (id & 15) * 4;
    *reinterpret_cast<float4*>(t0 + off) = x.a[i];
    *reinterpret_cast<float4*>(t1 + off) = x.b[i];
  }
}

// blockIdx.x -> (sequence, 128-row block of that sequence)
__device__ inline void who(const AttnP& p, int& s, int& blk) {
  const int nb = (p.L + ROWS - 1) / ROWS;
  s = blockIdx.x / nb;
  blk = blockIdx.x - s * nb;
}

// This lane's half of row `row` (rows beyond nvalid read row nvalid - 1: finite operands for a lane that is never stored).
__device__ inline void load_frag(frag& f, const float* base, long ld, int col0, const RowLin& rl, int row, int nvalid, int lane) {
  const int rc = row < nvalid ? row : nvalid - 1;
  const float* src = base + lin_row(rl, rc) * ld + col0 + 4 * (lane >> 5);
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const float4 v = *reinterpret_cast<const float4*>(src + 8 * g);
    f[4 * g] = v.x; f[4 * g + 1] = v.y; f[4 * g + 2] = v.z; f[4 * g + 3] = v.w;
  }
}

// Per-lane LDS offsets (floats) of the two readers; the tile row (a multiple of 32) adds an immediate.
__device__ inline int rows_off(int lane) { return (lane & 31) * LD + 4 * (lane >> 5); }
__device__ inline int cols_off(int lane) { return 4 * (lane >> 5) * LD + (lane & 31); }

// C[i][j] = sum_d tile[row0 + i][d] * b_j[d]: 32 tile rows against the lanes' own row fragments (32 MFMAs).
__device__ inline f32x16 tile_rows(const float* t, int row0, const frag& b) {
  f32x16 acc;
  zero16(acc);
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const float4 a = *reinterpret_cast<const float4*>(t + row0 * LD + 8 * g);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[4 * g], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[4 * g + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[4 * g + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[4 * g + 3], acc, 0, 0, 0);
  }
  return acc;
}

// acc[n2][d][j] += sum_i tile[row0 + i][32 n2 + d] * c[i][j] with c in the accumulator layout of tile_rows (32 MFMAs).
__device__ inline void tile_cols(f32x16 (&acc)[2], const float* t, int row0, const f32x16& c) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float* src = t + (row0 + (r & 3) + 8 * (r >> 2)) * LD;
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(src[0], c[r], acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(src[32], c[r], acc[1], 0, 0, 0);
  }
}

// Store a [32 x 64] result held transposed (lane & 31 = row, registers = 64 columns in two C tiles) through a wave-private
// LDS tile, so that global memory sees whole 256-byte rows: 16 lanes x 16 B, 4 rows per instruction.
// ptr_of_row(r) -> destination of tile row r (64 floats), or nullptr for a padded row.
template <typename PtrFn>
__device__ inline void store_rows(float* stg, const f32x16 (&acc)[2], float mul, int lane, PtrFn ptr_of_row) {
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

}  // namespace af

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(af::THREADS, 2) void attn_fwd_f32_kernel(AttnP p, const float* __restrict__ qkv, float* __restrict__ out,
                                                                      float* __restrict__ lse) {
  using namespace af;
  constexpr int KC = CHUNK / 32;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, D = p.H * 64;
  int s, qb;
  who(p, s, qb);
  const int q0 = qb * ROWS + wave * 32, qi = q0 + (lane & 31);
  const bool active = q0 < p.L;                    // wave-uniform; an idle wave still fills and meets the barriers
  const RowLin li = lin_in(p, s), lo = lin_out(p, s);
  const float* kb = qkv + D + h * 64;
  const float* vb = qkv + 2 * D + h * 64;
  frag qf;
  load_frag(qf, qkv, p.ld_qkv, h * 64, li, qi, p.L, lane);
  Pre pre;
  chunk_load(pre, kb, p.ld_qkv, li, vb, p.ld_qkv, li, 0, p.L);
  chunk_store(pre, sm, sm + TILE);
  __syncthreads();
  const int ro = rows_off(lane), co = cols_off(lane);
  const float c2 = p.scale * LOG2E;
  f32x16 acc[2];
  zero16(acc[0]);
  zero16(acc[1]);
  float m = -1e30f, l = 0.f;                       // running max of the RAW scores (scale > 0)
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const float* Ks = sm + (c & 1) * STAGE;
    const float* Vs = Ks + TILE;
    chunk_load(pre, kb, p.ld_qkv, li, vb, p.ld_qkv, li, (c + 1) * CHUNK, p.L);
    if (active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
      f32x16 st[KC];                               // (tiles beyond nt stay undefined: every use below is guarded)
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) st[t] = tile_rows(Ks + ro, t * 32, qf);
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
        if (t < nt) tile_cols(acc, Vs + co, t * 32, st[t]);
    }
    if (c + 1 < nch) {
      float* nx = sm + ((c + 1) & 1) * STAGE;      // last read in iteration c - 1, behind that iteration's barrier
      chunk_store(pre, nx, nx + TILE);
    }
    __syncthreads();
  }
  if (!active) return;
  float* stg = sm + wave * STG;                    // every wave is past the last chunk: the stages are free
  store_rows(stg, acc, 1.0f / l, lane, [&](int r) -> float* {
    const int qq = q0 + r;
    return qq < p.L ? out + lin_row(lo, qq) * p.ld_out + h * 64 : nullptr;
  });
  if (qi < p.L && lane < 32) lse[((long)s * p.H + h) * p.L + qi] = (m * c2) * LN2 + __logf(l);
}

// ------------------------------------------------------------------------------------------------ backward: dq (+ delta)
__global__ __launch_bounds__(af::THREADS, 2) void attn_bwd_dq_f32_kernel(AttnP p, const float* __restrict__ qkv, const float* __restrict__ o,
                                                                         const float* __restrict__ dout, const float* __restrict__ lse,
                                                                         float* __restrict__ delta, float* __restrict__ dqkv,
                                                                         float* __restrict__ dqkv_cls) {
  using namespace af;
  constexpr int KC = CHUNK / 32;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, D = p.H * 64;
  int s, qb;
  who(p, s, qb);
  const int q0 = qb * ROWS + wave * 32, qi = q0 + (lane & 31);
  const bool active = q0 < p.L;
  const RowLin li = lin_in(p, s), lo = lin_out(p, s);
  const float* kb = qkv + D + h * 64;
  const float* vb = qkv + 2 * D + h * 64;
  frag qf, df;
  float dl = 0.f;                                  // delta = rowsum(dO * O): this lane's 32 of the row's 64 columns
  {
    frag of;
    load_frag(qf, qkv, p.ld_qkv, h * 64, li, qi, p.L, lane);
    load_frag(df, dout, p.ld_dout, h * 64, lo, qi, p.L, lane);
    load_frag(of, o, p.ld_out, h * 64, lo, qi, p.L, lane);
#pragma unroll
    for (int e = 0; e < 32; ++e) dl = fmaf(df[e], of[e], dl);
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
  const int ro = rows_off(lane), co = cols_off(lane);
  const float c2 = p.scale * LOG2E;
  f32x16 acc[2];
  zero16(acc[0]);
  zero16(acc[1]);
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const float* Ks = sm + (c & 1) * STAGE;
    const float* Vs = Ks + TILE;
    chunk_load(pre, kb, p.ld_qkv, li, vb, p.ld_qkv, li, (c + 1) * CHUNK, p.L);
    if (active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) {
          const f32x16 st = tile_rows(Ks + ro, t * 32, qf);
          f32x16 ds = tile_rows(Vs + ro, t * 32, df);
          // dS = P (dP - delta); the softmax scale is applied once to dq at the store.  A padded key has zero K and V rows:
          // its dS is finite and multiplies zeros.
#pragma unroll
          for (int r = 0; r < 16; ++r) ds[r] = __builtin_amdgcn_exp2f(fmaf(st[r], c2, -l2)) * (ds[r] - dl);
          tile_cols(acc, Ks + co, t * 32, ds);
        }
    }
    if (c + 1 < nch) {
      float* nx = sm + ((c + 1) & 1) * STAGE;
      chunk_store(pre, nx, nx + TILE);
    }
    __syncthreads();
  }
  if (!active) return;
  float* stg = sm + wave * STG;
  store_rows(stg, acc, p.scale, lane, [&](int r) -> float* {
    const int qq = q0 + r;
    if (qq >= p.L) return nullptr;
    return (p.mode == VTX_ATTN_SPACE && qq == 0) ? dqkv_cls + (long)s * p.ld_dqkv + h * 64
                                                  : dqkv + lin_row(li, qq) * p.ld_dqkv + h * 64;
  });
}

// ------------------------------------------------------------------------------------------------ backward: dk, dv
// Lanes = keys: wave w of the workgroup of key block kb owns the key tile kb * 4 + w and walks ALL queries of the sequence.
__global__ __launch_bounds__(af::THREADS, 2) void attn_bwd_dkv_f32_kernel(AttnP p, const float* __restrict__ qkv,
                                                                          const float* __restrict__ dout, const float* __restrict__ lse,
                                                                          const float* __restrict__ delta, float* __restrict__ dqkv,
                                                                          float* __restrict__ dqkv_cls) {
  using namespace af;
  constexpr int QC = CHUNK / 32;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* stats = sm + 2 * STAGE;                   // [stage][lse * log2(e) | delta][CHUNK]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, D = p.H * 64;
  int s, kblk;
  who(p, s, kblk);
  const int key0 = kblk * ROWS + wave * 32, key = key0 + (lane & 31);
  const bool active = key0 < p.L;
  const RowLin li = lin_in(p, s), lo = lin_out(p, s);
  const float* qb = qkv + h * 64;
  const float* ob = dout + h * 64;
  const float* lb = lse + ((long)s * p.H + h) * p.L;
  const float* db = delta + ((long)s * p.H + h) * p.L;
  frag kf, vf;
  load_frag(kf, qkv, p.ld_qkv, D + h * 64, li, key, p.L, lane);
  load_frag(vf, qkv, p.ld_qkv, 2 * D + h * 64, li, key, p.L, lane);
  // thread t < 64: lse of chunk row t (scaled; +huge on padded rows -> P = 0); 64 <= t < 128: delta of chunk row t - 64
  const int srow = threadIdx.x & (CHUNK - 1);
  const bool is_lse = threadIdx.x < CHUNK, has_stat = threadIdx.x < 2 * CHUNK;
  auto stat_load = [&](int row0) -> float {
    const int r = row0 + srow;
    if (!has_stat || r >= p.L) return is_lse ? 1e30f : 0.f;
    return is_lse ? lb[r] * LOG2E : db[r];
  };
  Pre pre;
  chunk_load(pre, qb, p.ld_qkv, li, ob, p.ld_dout, lo, 0, p.L);
  float sv = stat_load(0);
  chunk_store(pre, sm, sm + TILE);
  if (has_stat) stats[threadIdx.x] = sv;
  __syncthreads();
  const int ro = rows_off(lane), co = cols_off(lane);
  const float c2 = p.scale * LOG2E;
  f32x16 dk[2], dv[2];
  zero16(dk[0]); zero16(dk[1]); zero16(dv[0]); zero16(dv[1]);
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const float* Qs = sm + (c & 1) * STAGE;
    const float* Os = Qs + TILE;
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
          // padded query rows: Ls = +huge -> P = 0, zero Q / dO rows; padded keys only feed dk / dv rows that are never stored
          f32x16 pr = tile_rows(Qs + ro, t * 32, kf);
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float4 l4 = *reinterpret_cast<const float4*>(Ls + t * 32 + 8 * g + 4 * (lane >> 5));
            pr[4 * g] = __builtin_amdgcn_exp2f(fmaf(pr[4 * g], c2, -l4.x));
            pr[4 * g + 1] = __builtin_amdgcn_exp2f(fmaf(pr[4 * g + 1], c2, -l4.y));
            pr[4 * g + 2] = __builtin_amdgcn_exp2f(fmaf(pr[4 * g + 2], c2, -l4.z));
            pr[4 * g + 3] = __builtin_amdgcn_exp2f(fmaf(pr[4 * g + 3], c2, -l4.w));
          }
          tile_cols(dv, Os + co, t * 32, pr);
          f32x16 ds = tile_rows(Os + ro, t * 32, vf);
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float4 d4 = *reinterpret_cast<const float4*>(Ds + t * 32 + 8 * g + 4 * (lane >> 5));
            ds[4 * g] = pr[4 * g] * (ds[4 * g] - d4.x);          // the softmax scale is applied once to dk at the store
            ds[4 * g + 1] = pr[4 * g + 1] * (ds[4 * g + 1] - d4.y);
            ds[4 * g + 2] = pr[4 * g + 2] * (ds[4 * g + 2] - d4.z);
            ds[4 * g + 3] = pr[4 * g + 3] * (ds[4 * g + 3] - d4.w);
          }
          tile_cols(dk, Qs + co, t * 32, ds);
        }
    }
    if (c + 1 < nch) {
      float* nx = sm + ((c + 1) & 1) * STAGE;
      chunk_store(pre, nx, nx + TILE);
      if (has_stat) stats[((c + 1) & 1) * 2 * CHUNK + threadIdx.x] = sv;
    }
    __syncthreads();
  }
  if (!active) return;
  float* stg = sm + wave * STG;
  auto base_of = [&](int r) -> float* {
    const int kk = key0 + r;
    if (kk >= p.L) return nullptr;
    return (p.mode == VTX_ATTN_SPACE && kk == 0) ? dqkv_cls + (long)s * p.ld_dqkv : dqkv + lin_row(li, kk) * p.ld_dqkv;
  };
  store_rows(stg, dk, p.scale, lane, [&](int r) -> float* { float* b = base_of(r); return b ? b + D + h * 64 : nullptr; });
  store_rows(stg, dv, 1.0f, lane, [&](int r) -> float* { float* b = base_of(r); return b ? b + 2 * D + h * 64 : nullptr; });
}

// host-side launchers used by attn.hip's entry points --------------------------------------
bool attn_f32_eligible(int dtype, int L, int hd) { return dtype == VTX_F32 && hd == 64 && L > 32; }

constexpr size_t AF_LDS_KV = (size_t)2 * af::STAGE * sizeof(float);                       // 68 KiB
constexpr size_t AF_LDS_DKV = AF_LDS_KV + (size_t)2 * 2 * af::CHUNK * sizeof(float);      // + lse / delta of both stages

static dim3 f32_grid(const AttnP& p) { return dim3((unsigned)p.S * (unsigned)cdiv(p.L, af::ROWS), p.H); }

// > 64 KiB of dynamic LDS needs an explicit opt-in, once per kernel and device
static void f32_opt_in(std::atomic<unsigned long long>& seen, const void* kernel) {
  if (first_launch_on_device(seen)) hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

int attn_fwd_f32_launch(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st) {
  static std::atomic<unsigned long long> seen{0};
  f32_opt_in(seen, reinterpret_cast<const void*>(&attn_fwd_f32_kernel));
  hipLaunchKernelGGL(attn_fwd_f32_kernel, f32_grid(p), dim3(af::THREADS), AF_LDS_KV, st, p, (const float*)qkv, (float*)out, lse);
  return check_launch("attn_fwd_f32");
}

int attn_bwd_f32_launch(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                        void* dqkv_cls, hipStream_t st) {
  static std::atomic<unsigned long long> seen_dq{0}, seen_dkv{0};
  f32_opt_in(seen_dq, reinterpret_cast<const void*>(&attn_bwd_dq_f32_kernel));
  hipLaunchKernelGGL(attn_bwd_dq_f32_kernel, f32_grid(p), dim3(af::THREADS), AF_LDS_KV, st, p, (const float*)qkv, (const float*)o,
                     (const float*)dout, lse, delta, (float*)dqkv, (float*)dqkv_cls);
  int rc = check_launch("attn_bwd_dq_f32");
  if (rc) return rc;
  f32_opt_in(seen_dkv, reinterpret_cast<const void*>(&attn_bwd_dkv_f32_kernel));
  hipLaunchKernelGGL(attn_bwd_dkv_f32_kernel, f32_grid(p), dim3(af::THREADS), AF_LDS_DKV, st, p, (const float*)qkv, (const float*)dout,
                     lse, delta, (float*)dqkv, (float*)dqkv_cls);
  return check_launch("attn_bwd_dkv_f32");
}

}  // namespace vtx
