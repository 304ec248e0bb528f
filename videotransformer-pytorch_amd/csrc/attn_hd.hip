// attn_hd.hip -- bf16 MFMA attention core for head_dim 32, 96 and 128: more than 32 tokens per sequence in all four layouts
// (namespace hdim, described here), up to 32 tokens in the layouts CONTIG and TIME_CLS (namespace hdsmall, at the end of the file).
//
// The structure is the chunk streaming of attn_stream.h (read its header first: transposed scores, a workgroup of 4 waves owns 128
// queries -- 128 keys in the dk / dv kernel --, the other operands stream through two LDS stages, one barrier per chunk, dk / dv
// with one workgroup per key block walking all queries: fixed summation order, no atomics, no workspace), and the formulation is
// that of attn_long.hip: v_mfma_f32_32x32x16_bf16, swizzled [rows][64] bf16 tiles, transposed operands through
// ds_read_b64_tr_b16 (sw_off / frag_rows_o / frag_cols_o of attn_common.h, unchanged).  The tile helpers (chunk load / store,
// row fragments, scores, accum, dkv_tile, store_rows) are Bf16Tiles<HD, 64> of attn_tiles_bf16.h, the policy attn_long.hip
// instantiates as <64, 128>; the three kernel bodies are still restated here over HD.  attn_stream.h's bodies over the same policy
// compute the same bits with the same registers and scratch, but their forward at head_dim 128 measured 8.7 % slower at 8 x 1569
// tokens (0.115 -> 0.125 ms; the other 27 rows held: profiles/attn_stream_hd_refactor_bench.txt, section 4), while with the bodies
// kept here this file's device code is byte for byte the one before the helpers moved.  The bodies stay until the schedule of
// that kernel's chunk loop is understood.
//
// A head is NS = ceil(HD / 64) column slabs of the [rows][64] tile, the last one half used at 32 and 96 (its upper 32 columns
// are never written and never read):
//   scores         HD / 16 chained k-steps, step ks from slab ks / 4                    (2 | 6 | 8 MFMAs per 32 x 32 score tile)
//   accumulators   HD / 32 f32x16 tiles, tile n from slab n / 2, column half n % 2      (1 | 3 | 4)
//   no padded products: the half-used slab costs LDS, not matrix instructions.
// LDS: one operand of a chunk is NS slabs of CHUNK = 64 rows: 8 KiB at one slab, 16 KiB at two; a stage holds two operands and
// there are two stages: 32 KiB at head_dim 32, 64 KiB at 96 and 128 (+ 1 KiB of lse / delta in the dk / dv kernel).  At 32 that
// admits three workgroups a CU, and three measured 11 % faster than two with 128-row chunks (the kernel waits on softmax VALU work
// and chunk stores, not on the matrix pipe); at 96 / 128 two fit the CU's 160 KiB.
// Registers (per lane, f32x16 = 16): row fragments HD / 4 per operand; forward acc HD / 2 + CHUNK / 2 of scores; dk / dv holds
// 2 * HD / 2 of accumulators + 2 * HD / 4 of K and V fragments + 64 of S, dP, P, dS: 112 | 208 | 256 at 32 | 96 | 128, and
// 8 | 24 | 32 of the chunk in flight, before addresses.  The dk / dv kernel is therefore bounded to two workgroups a CU at 96 (256 registers, 76 B of scratch a lane:
// 6 - 10 % faster than one workgroup without scratch) and to one at 128 (388 registers; bounded to two it spills 296 B and
// runs 1.4 - 1.8 x slower); forward and dq run two a CU at 96 / 128.  profiles/attn_hd_bench.txt has what the compiler made of it.
//
// Masking as in attn_stream.h: keys >= L have zero K / V rows and score -1e30 before the max; query rows >= L keep to their lane
// and are never stored; in the dk / dv kernel padded query rows carry lse = +1e30.
// FLOPs per (sequence, head): forward 4 L^2 HD, backward 10 L^2 HD (+ 4 L^2 HD recomputed scores).
#include "attn_tiles_bf16.h"

namespace vtx {
namespace hdim {

constexpr int THREADS = 256;
constexpr int ROWS = 128;                          // queries (keys in the dk / dv kernel) of one workgroup: 4 waves x 32

template <int HD> using Geo = Bf16Tiles<HD, 64>;    // the tile policy (attn_tiles_bf16.h): 64-row chunks at every head dim of this file
template <int HD> constexpr size_t LDS_KV = stream_lds_kv<Geo<HD>>();
template <int HD> constexpr size_t LDS_DKV = stream_lds_dkv<Geo<HD>>();
// dynamic LDS of a launch: forward and dq, dk / dv
static_assert(LDS_KV<32> == 32768 && LDS_DKV<32> == 33792, "dynamic LDS of a launch");
static_assert(LDS_KV<96> == 65536 && LDS_DKV<96> == 66560 && LDS_KV<128> == 65536 && LDS_DKV<128> == 66560, "dynamic LDS of a launch");

struct Who {
  int lane, wave, h, D, s, row0, row;              // row0: first of the wave's 32 rows; row: this lane's
  bool active;                                     // wave-uniform; an idle wave still fills and meets the barriers
  RowLin li, lo;
};
template <int HD>
__device__ inline Who who(const AttnP& p) {
  Who w;
  w.lane = threadIdx.x & 63;
  w.wave = threadIdx.x >> 6;
  w.h = blockIdx.y;
  w.D = p.H * HD;
  const int nb = (p.L + ROWS - 1) / ROWS;          // blockIdx.x -> (sequence, 128-row block of that sequence)
  w.s = blockIdx.x / nb;
  w.row0 = (blockIdx.x - w.s * nb) * ROWS + w.wave * 32;
  w.row = w.row0 + (w.lane & 31);
  w.active = w.row0 < p.L;
  w.li = lin_in(p, w.s);
  w.lo = lin_out(p, w.s);
  return w;
}

__device__ inline bf16raw* lds_base() {
  extern __shared__ __attribute__((aligned(16))) char sm_raw[];
  return reinterpret_cast<bf16raw*>(sm_raw);
}

// ------------------------------------------------------------------------------------------------ forward
template <int HD>
__global__ __launch_bounds__(THREADS, HD == 32 ? 3 : 2) void fwd_kernel(AttnP p, const bf16raw* __restrict__ qkv, bf16raw* __restrict__ out,
                                                         float* __restrict__ lse) {
  typedef Geo<HD> G;
  constexpr int CHUNK = G::CHUNK, KC = CHUNK / 32;
  bf16raw* sm = lds_base();
  const Who w = who<HD>(p);
  const int lane = w.lane, h = w.h;
  const bf16raw* kb = qkv + w.D + h * HD;
  const bf16raw* vb = qkv + 2 * w.D + h * HD;
  typename G::Frag qf;
  G::load_frag(qf, qkv, p.ld_qkv, h * HD, w.li, w.row, p.L, lane);
  typename G::Pre pre;
  G::chunk_load(pre, kb, p.ld_qkv, w.li, vb, p.ld_qkv, w.li, 0, p.L);
  G::chunk_store(pre, sm, sm + G::TILE);
  __syncthreads();
  const FragOff ln = make_frag_off(lane);
  const float c2 = p.scale * LOG2E;
  f32x16 acc[G::NT];
#pragma unroll
  for (int n = 0; n < G::NT; ++n) zero16(acc[n]);
  float m = -1e30f, l = 0.f;                       // running max of the RAW scores (scale > 0)
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const bf16raw* Ks = sm + (c & 1) * G::STAGE;
    const bf16raw* Vs = Ks + G::TILE;
    G::chunk_load(pre, kb, p.ld_qkv, w.li, vb, p.ld_qkv, w.li, (c + 1) * CHUNK, p.L);
    if (w.active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
      f32x16 st[KC];                               // (tiles beyond nt stay undefined: every use below is guarded)
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) st[t] = G::scores(Ks, t * 32, qf, ln);
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
        for (int n = 0; n < G::NT; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[n][r] *= alpha;
      }
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) G::accum(acc, Vs, t * 32, st[t], ln);
    }
    if (c + 1 < nch) {
      bf16raw* nx = sm + ((c + 1) & 1) * G::STAGE; // last read in iteration c - 1, behind that iteration's barrier
      G::chunk_store(pre, nx, nx + G::TILE);
    }
    __syncthreads();
  }
  if (!w.active) return;
  bf16raw* stg = sm + w.wave * MA_STAGE_ELEMS;     // every wave is past the last chunk: the stages are free
  G::store_rows(stg, acc, 1.0f / l, lane, [&](int r) -> bf16raw* {
    const int qq = w.row0 + r;
    return qq < p.L ? out + lin_row(w.lo, qq) * p.ld_out + h * HD : nullptr;
  });
  if (w.row < p.L && lane < 32) lse[((long)w.s * p.H + h) * p.L + w.row] = (m * c2) * LN2 + __logf(l);
}

// ------------------------------------------------------------------------------------------------ backward: dq (+ delta)
template <int HD>
__global__ __launch_bounds__(THREADS, HD == 32 ? 3 : 2) void bwd_dq_kernel(AttnP p, const bf16raw* __restrict__ qkv, const bf16raw* __restrict__ o,
                                                            const bf16raw* __restrict__ dout, const float* __restrict__ lse,
                                                            float* __restrict__ delta, bf16raw* __restrict__ dqkv,
                                                            bf16raw* __restrict__ dqkv_cls) {
  typedef Geo<HD> G;
  constexpr int CHUNK = G::CHUNK, KC = CHUNK / 32;
  bf16raw* sm = lds_base();
  const Who w = who<HD>(p);
  const int lane = w.lane, h = w.h;
  const bf16raw* kb = qkv + w.D + h * HD;
  const bf16raw* vb = qkv + 2 * w.D + h * HD;
  typename G::Frag qf, df;
  float dl;                                        // delta = rowsum(dO * O): this lane's half of the row's columns
  {
    typename G::Frag of;
    G::load_frag(qf, qkv, p.ld_qkv, h * HD, w.li, w.row, p.L, lane);
    G::load_frag(df, dout, p.ld_dout, h * HD, w.lo, w.row, p.L, lane);
    G::load_frag(of, o, p.ld_out, h * HD, w.lo, w.row, p.L, lane);
    dl = G::frag_dot(df, of);
  }
  dl += __shfl_xor(dl, 32, 64);
  float l2 = 0.f;
  if (w.row < p.L) {
    const long lidx = ((long)w.s * p.H + h) * p.L + w.row;
    l2 = lse[lidx] * LOG2E;
    if (lane < 32) delta[lidx] = dl;
  }
  typename G::Pre pre;
  G::chunk_load(pre, kb, p.ld_qkv, w.li, vb, p.ld_qkv, w.li, 0, p.L);
  G::chunk_store(pre, sm, sm + G::TILE);
  __syncthreads();
  const FragOff ln = make_frag_off(lane);
  const float c2 = p.scale * LOG2E;
  f32x16 acc[G::NT];
#pragma unroll
  for (int n = 0; n < G::NT; ++n) zero16(acc[n]);
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const bf16raw* Ks = sm + (c & 1) * G::STAGE;
    const bf16raw* Vs = Ks + G::TILE;
    G::chunk_load(pre, kb, p.ld_qkv, w.li, vb, p.ld_qkv, w.li, (c + 1) * CHUNK, p.L);
    if (w.active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) {
          const f32x16 st = G::scores(Ks, t * 32, qf, ln);
          f32x16 ds = G::scores(Vs, t * 32, df, ln);
          // dS = P (dP - delta); the softmax scale is applied once to dq at the store.  A padded key has zero K and V rows:
          // its dS is finite and multiplies zeros; it is zeroed all the same, which keeps the pack clean.
#pragma unroll
          for (int r = 0; r < 16; ++r) ds[r] = __builtin_amdgcn_exp2f(fmaf(st[r], c2, -l2)) * (ds[r] - dl);
          if (t * 32 + 32 > nrows) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (t * 32 + crow(r, lane) >= nrows) ds[r] = 0.f;
          }
          G::accum(acc, Ks, t * 32, ds, ln);
        }
    }
    if (c + 1 < nch) {
      bf16raw* nx = sm + ((c + 1) & 1) * G::STAGE;
      G::chunk_store(pre, nx, nx + G::TILE);
    }
    __syncthreads();
  }
  if (!w.active) return;
  bf16raw* stg = sm + w.wave * MA_STAGE_ELEMS;
  G::store_rows(stg, acc, p.scale, lane, [&](int r) -> bf16raw* {
    const int qq = w.row0 + r;
    if (qq >= p.L) return nullptr;
    return attn_cls_row(p, qq) ? dqkv_cls + (long)w.s * p.ld_dqkv + h * HD : dqkv + lin_row(w.li, qq) * p.ld_dqkv + h * HD;
  });
}

// ------------------------------------------------------------------------------------------------ backward: dk, dv
// Lanes = keys: wave w of the workgroup of key block kb owns the key tile kb * 4 + w and walks ALL queries of the sequence.
template <int HD>
__global__ __launch_bounds__(THREADS, HD == 32 ? 3 : HD == 96 ? 2 : 1) void bwd_dkv_kernel(AttnP p, const bf16raw* __restrict__ qkv,
                                                                            const bf16raw* __restrict__ dout,
                                                                            const float* __restrict__ lse, const float* __restrict__ delta,
                                                                            bf16raw* __restrict__ dqkv, bf16raw* __restrict__ dqkv_cls) {
  typedef Geo<HD> G;
  constexpr int CHUNK = G::CHUNK, QC = CHUNK / 32;
  bf16raw* sm = lds_base();
  float* stats = reinterpret_cast<float*>(sm + 2 * G::STAGE);    // [stage][lse * log2(e) | delta][CHUNK]
  const Who w = who<HD>(p);
  const int lane = w.lane, h = w.h, D = w.D;
  const bf16raw* qb = qkv + h * HD;
  const bf16raw* ob = dout + h * HD;
  const float* lb = lse + ((long)w.s * p.H + h) * p.L;
  const float* db = delta + ((long)w.s * p.H + h) * p.L;
  typename G::Frag kf, vf;
  G::load_frag(kf, qkv, p.ld_qkv, D + h * HD, w.li, w.row, p.L, lane);
  G::load_frag(vf, qkv, p.ld_qkv, 2 * D + h * HD, w.li, w.row, p.L, lane);
  // thread t < CHUNK: lse of chunk row t (scaled; +huge on padded rows -> P = 0); CHUNK <= t < 2 CHUNK: delta of chunk row t - CHUNK
  const int srow = threadIdx.x & (CHUNK - 1);
  const bool is_lse = threadIdx.x < CHUNK, has_stat = threadIdx.x < 2 * CHUNK;
  auto stat_load = [&](int row0) -> float {
    const int r = row0 + srow;
    if (!has_stat || r >= p.L) return is_lse ? 1e30f : 0.f;
    return is_lse ? lb[r] * LOG2E : db[r];
  };
  typename G::Pre pre;
  G::chunk_load(pre, qb, p.ld_qkv, w.li, ob, p.ld_dout, w.lo, 0, p.L);
  float sv = stat_load(0);
  G::chunk_store(pre, sm, sm + G::TILE);
  if (has_stat) stats[threadIdx.x] = sv;
  __syncthreads();
  const FragOff ln = make_frag_off(lane);
  const float c2 = p.scale * LOG2E;
  f32x16 dk[G::NT], dv[G::NT];
#pragma unroll
  for (int n = 0; n < G::NT; ++n) { zero16(dk[n]); zero16(dv[n]); }
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const bf16raw* Qs = sm + (c & 1) * G::STAGE;
    const bf16raw* Os = Qs + G::TILE;
    const float* Ls = stats + (c & 1) * 2 * CHUNK;
    const float* Ds = Ls + CHUNK;
    G::chunk_load(pre, qb, p.ld_qkv, w.li, ob, p.ld_dout, w.lo, (c + 1) * CHUNK, p.L);
    sv = stat_load((c + 1) * CHUNK);
    if (w.active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
#pragma unroll
      for (int t = 0; t < QC; ++t)
        // padded query rows: Ls = +huge -> P = 0, zero Q / dO rows; padded keys only feed dk / dv rows that are never stored
        if (t < nt) G::dkv_tile(dk, dv, Qs, Os, Ls, Ds, t * 32, kf, vf, c2, ln, lane);
    }
    if (c + 1 < nch) {
      bf16raw* nx = sm + ((c + 1) & 1) * G::STAGE;
      G::chunk_store(pre, nx, nx + G::TILE);
      if (has_stat) stats[((c + 1) & 1) * 2 * CHUNK + threadIdx.x] = sv;
    }
    __syncthreads();
  }
  if (!w.active) return;
  bf16raw* stg = sm + w.wave * MA_STAGE_ELEMS;
  auto base_of = [&](int r) -> bf16raw* {
    const int kk = w.row0 + r;
    if (kk >= p.L) return nullptr;
    return attn_cls_row(p, kk) ? dqkv_cls + (long)w.s * p.ld_dqkv : dqkv + lin_row(w.li, kk) * p.ld_dqkv;
  };
  G::store_rows(stg, dk, p.scale, lane, [&](int r) -> bf16raw* { bf16raw* b = base_of(r); return b ? b + D + h * HD : nullptr; });
  G::store_rows(stg, dv, 1.0f, lane, [&](int r) -> bf16raw* { bf16raw* b = base_of(r); return b ? b + 2 * D + h * HD : nullptr; });
}

// host side ---------------------------------------------------------------------------------------
static dim3 grid_of(const AttnP& p) { return dim3((unsigned)p.S * (unsigned)cdiv(p.L, ROWS), p.H); }

template <int HD>
static int fwd_launch(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st) {
  hipLaunchKernelGGL(fwd_kernel<HD>, grid_of(p), dim3(THREADS), LDS_KV<HD>, st, p, (const bf16raw*)qkv, (bf16raw*)out, lse);
  return check_launch("attn_fwd_hd");
}
template <int HD>
static int bwd_launch(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                      void* dqkv_cls, hipStream_t st) {
  hipLaunchKernelGGL(bwd_dq_kernel<HD>, grid_of(p), dim3(THREADS), LDS_KV<HD>, st, p, (const bf16raw*)qkv, (const bf16raw*)o,
                     (const bf16raw*)dout, lse, delta, (bf16raw*)dqkv, (bf16raw*)dqkv_cls);
  const int rc = check_launch("attn_bwd_dq_hd");
  if (rc) return rc;
  allow_lds<bwd_dkv_kernel<HD>>(LDS_DKV<HD>);
  hipLaunchKernelGGL(bwd_dkv_kernel<HD>, grid_of(p), dim3(THREADS), LDS_DKV<HD>, st, p, (const bf16raw*)qkv, (const bf16raw*)dout,
                     lse, (const float*)delta, (bf16raw*)dqkv, (bf16raw*)dqkv_cls);
  return check_launch("attn_bwd_dkv_hd");
}

}  // namespace hdim

// =====================================================================================================================
// Up to 32 tokens, layouts CONTIG and TIME_CLS: the packed formulation of attn_mfma.hip's attn_fwd_small_kernel /
// attn_bwd_small_kernel (read the comment there), over HD.  G = 32 / L sequences share one 32-row tile under a block-diagonal
// mask, ONE WAVE handles a (tile, head) pair end to end, row fragments come straight from HBM, the transposed operands sit in
// wave-private LDS tiles, whole rows are stored through the idle tile, delta is neither read nor written.
// A wave-private tile is Geo<HD>::NS slabs of the swizzled [32][64] tile (4 KiB at head_dim 32, 8 KiB at 96 and 128; the
// upper half of the last slab is never written and never read at 32 and 96: a 32-column slab would need a swizzle and readers
// of its own for 2 KiB a wave).  Forward: one tile (V).  Backward: tile A (K, then Q), tile B (dO) and 32 lse + 32 delta:
// 8.25 KiB at 32, 16.25 KiB at 96 / 128 -- that is what bounds the waves of a CU there (9 of them in 160 KiB; a workgroup
// of 4 takes 65 KiB, hence the opt-in), and the register bound follows it: two waves a SIMD, 256 registers.
// attn_hw_fwd / attn_hw_bwd mean what they mean at head_dim 64 (n heads of a row tile per workgroup, head groups of a tile in
// consecutive workgroups; 0 = one head, four row tiles), capped at MAXW = 8 waves: at 96 / 128 for the forward's registers and
// the backward's LDS (D = 768 has 8 and 6 heads there), at 32 because 8 heads measured faster than 16 (temporal forward at 24
// heads: 0.191 against 0.245 ms, profiles/attn_hd_small_bench.txt).
// =====================================================================================================================
namespace hdsmall {

using hdim::Geo;                                  // NS / NK / NT, Frag and store_rows of a head
template <int HD> using Frag = typename Geo<HD>::Frag;

template <int HD> struct Sm {
  static constexpr int SLAB = 32 * 64;                                  // elements of one [32][64] slab
  static constexpr int TILE = Geo<HD>::NS * SLAB;
  static constexpr int LDS_FWD = TILE * 2;                              // V tile
  static constexpr int LDS_BWD = 2 * TILE * 2 + 2 * 32 * 4;             // tile A (K, then Q), tile B (dO) + lse + delta
  static constexpr int MAXW = 8;                                        // waves of a heads-per-workgroup launch
};

// SmallRows / small_rows of attn_mfma.hip, restated (that file stays as it is).  Tile row j < used belongs to sequence
// sq = tile * G + j / L, token i = j % L; CLS = VTX_ATTN_TIME_CLS.  grad: row of dqkv, or -1 - (row of dqkv_cls).
struct Rows { long in, out, grad, lse; };
template <bool CLS>
__device__ inline Rows rows_of(const AttnP& p, int tile, int G, int j) {
  Rows r;
  const int L = p.L;
  if (!CLS) {
    const long row = (long)tile * (G * L) + j;
    const long sq = row / L;
    r.in = r.out = r.grad = row;
    r.lse = sq * p.H * L + (row - sq * L);
    return r;
  }
  const int g = j / L, i = j - g * L;
  const long sq = (long)tile * G + g;
  const long b = sq / p.P;
  r.in = i == 0 ? b * (1 + (long)p.P * p.T) : sq * p.T + b + i;
  r.out = i == 0 ? (long)p.B * p.P * p.T + sq : sq * p.T + (i - 1);
  r.grad = i == 0 ? -1 - sq : r.in;
  r.lse = sq * p.H * L + i;
  return r;
}

// A row's HD columns straight from HBM (an invalid lane reads nothing and holds zeros).
template <int HD>
__device__ __forceinline__ void load_frags(Frag<HD>& f, const bf16raw* base, long ld, int col0, long row, bool valid, int lane) {
#pragma unroll
  for (int ks = 0; ks < Geo<HD>::NK; ++ks) {
    union { bf16x8 v; uint4 u; } x;
    x.u = make_uint4(0, 0, 0, 0);
    if (valid) x.u = *reinterpret_cast<const uint4*>(base + row * ld + col0 + ks * 16 + 8 * (lane >> 5));
    f.f[ks] = x.v;
  }
}
// The row fragments of a 32-row tile (one row per lane) into the wave's tile, slab by slab.
template <int HD>
__device__ __forceinline__ void put_tile(bf16raw* t, const Frag<HD>& f, const FragOff& fo) {
#pragma unroll
  for (int ks = 0; ks < Geo<HD>::NK; ++ks) *reinterpret_cast<bf16x8*>(t + (ks >> 2) * Sm<HD>::SLAB + fo.rows[ks & 3]) = f.f[ks];
}
// acc[n][d][j] += sum_i tile[i][32 n + d] c[i][j] over the tile's 32 rows, c = 16 values per lane in accumulator order
template <int HD>
__device__ __forceinline__ void accum(f32x16 (&acc)[Geo<HD>::NT], const bf16raw* t, const float* c, const FragOff& fo) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const bf16x8 pb = pack8(c + 8 * s2);
#pragma unroll
    for (int n = 0; n < Geo<HD>::NT; ++n)
      acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_o(t + (n >> 1) * Sm<HD>::SLAB, 16 * s2, n & 1, fo), pb, acc[n], 0, 0, 0);
  }
}

struct Who {
  int lane, wave, tile, h;
  bool run;
};
// HW: wave w of the workgroup works on head w of its head group, (head group, tile) folded into blockIdx.x, head group fastest;
// otherwise one head (blockIdx.y) and four row tiles per workgroup.
template <bool HW>
__device__ inline Who who(const AttnP& p, int ntiles) {
  Who w;
  w.lane = threadIdx.x & 63;
  w.wave = threadIdx.x >> 6;
  const int hw_w = blockDim.x >> 6, hw_ng = HW ? (p.H + hw_w - 1) / hw_w : 1;
  w.tile = HW ? (int)(blockIdx.x / hw_ng) : blockIdx.x * 4 + w.wave;
  w.h = HW ? w.wave + (int)(blockIdx.x % hw_ng) * hw_w : blockIdx.y;
  w.run = w.tile < ntiles && w.h < p.H;
  return w;
}

template <int HD, bool HW, bool CLS>
__global__ __launch_bounds__(HW ? 64 * Sm<HD>::MAXW : MA_THREADS) void fwd_kernel(AttnP p, int ntiles, const bf16raw* __restrict__ qkv,
                                                                              bf16raw* __restrict__ out, float* __restrict__ lse) {
  typedef Geo<HD> G_;
  extern __shared__ __attribute__((aligned(16))) char sm_raw[];
  const Who w = who<HW>(p, ntiles);
  if (!w.run) return;                              // (no workgroup barrier below: a wave is on its own)
  const int lane = w.lane, h = w.h, tile = w.tile, D = p.H * HD;
  bf16raw* Vs = reinterpret_cast<bf16raw*>(sm_raw + w.wave * Sm<HD>::LDS_FWD);
  const int L = p.L, G = 32 / L, used = G * L;
  const long row0 = (long)tile * used, total = (long)p.S * L;
  const int i = lane & 31;
  const bool valid = i < used && row0 + i < total;
  const Rows me = rows_of<CLS>(p, tile, G, valid ? i : 0);
  const FragOff fo = make_frag_off(lane);
  Frag<HD> qf, kf, vf;
  load_frags<HD>(qf, qkv, p.ld_qkv, h * HD, me.in, valid, lane);
  load_frags<HD>(kf, qkv, p.ld_qkv, D + h * HD, me.in, valid, lane);
  load_frags<HD>(vf, qkv, p.ld_qkv, 2 * D + h * HD, me.in, valid, lane);
  put_tile<HD>(Vs, vf, fo);
  f32x16 st;
  zero16(st);
#pragma unroll
  for (int ks = 0; ks < G_::NK; ++ks) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf.f[ks], qf.f[ks], st, 0, 0, 0);
  const float c2 = p.scale * LOG2E;
  const int qseq = i / L;
  float m = -INFINITY;
  float pr[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int key = crow(r, lane);
    const bool ok = valid && key < used && key / L == qseq && row0 + key < total;
    pr[r] = ok ? st[r] * c2 : -INFINITY;
    m = fmaxf(m, pr[r]);
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  if (!valid) m = 0.f;
  float l = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) { pr[r] = __builtin_amdgcn_exp2f(pr[r] - m); l += pr[r]; }
  l += __shfl_xor(l, 32, 64);
  wave_lds_sync();
  f32x16 acc[G_::NT];
#pragma unroll
  for (int n = 0; n < G_::NT; ++n) zero16(acc[n]);
  accum<HD>(acc, Vs, pr, fo);
  // whole rows through the (now idle) V tile
  Geo<HD>::store_rows(Vs, acc, valid ? 1.0f / l : 0.f, lane, [&](int r) -> bf16raw* {
    return (r < used && row0 + r < total) ? out + rows_of<CLS>(p, tile, G, r).out * p.ld_out + h * HD : nullptr;
  });
  if (valid && lane < 32) lse[me.lse + (long)h * L] = m * LN2 + __logf(l);
}

template <int HD, bool HW, bool CLS>
__global__ __launch_bounds__(HW ? 64 * Sm<HD>::MAXW : MA_THREADS, HW ? 1 : HD == 32 ? 4 : 2) void bwd_kernel(
    AttnP p, int ntiles, const bf16raw* __restrict__ qkv, const bf16raw* __restrict__ o, const bf16raw* __restrict__ dout,
    const float* __restrict__ lse, bf16raw* __restrict__ dqkv, bf16raw* __restrict__ dqkv_cls) {
  typedef Geo<HD> G_;
  extern __shared__ __attribute__((aligned(16))) char sm_raw[];
  const Who w = who<HW>(p, ntiles);
  if (!w.run) return;
  const int lane = w.lane, h = w.h, tile = w.tile, D = p.H * HD;
  // two wave-private tiles: A holds K for phase 1 (and stages dQ), then Q for phase 2 (and stages dK); B holds dO (and stages dV)
  char* wl = sm_raw + w.wave * Sm<HD>::LDS_BWD;
  bf16raw* Ks = reinterpret_cast<bf16raw*>(wl);
  bf16raw* Qs = Ks;
  bf16raw* Os = Ks + Sm<HD>::TILE;
  float* Ls = reinterpret_cast<float*>(Os + Sm<HD>::TILE);
  float* Ds = Ls + 32;
  const int L = p.L, G = 32 / L, used = G * L;
  const long row0 = (long)tile * used, total = (long)p.S * L;
  const int i = lane & 31;
  const bool valid = i < used && row0 + i < total;
  const Rows me = rows_of<CLS>(p, tile, G, valid ? i : 0);
  const FragOff fo = make_frag_off(lane);
  Frag<HD> qf, kf, vf, df;
  load_frags<HD>(qf, qkv, p.ld_qkv, h * HD, me.in, valid, lane);
  load_frags<HD>(kf, qkv, p.ld_qkv, D + h * HD, me.in, valid, lane);
  load_frags<HD>(vf, qkv, p.ld_qkv, 2 * D + h * HD, me.in, valid, lane);
  load_frags<HD>(df, dout, p.ld_dout, h * HD, me.out, valid, lane);
  float dl = 0.f;
  {
    Frag<HD> of;
    load_frags<HD>(of, o, p.ld_out, h * HD, me.out, valid, lane);
#pragma unroll
    for (int ks = 0; ks < G_::NK; ++ks) dl += frag_dot(df.f[ks], of.f[ks]);
  }
  dl += __shfl_xor(dl, 32, 64);
  float l2 = 1e30f;
  if (valid) l2 = lse[me.lse + (long)h * L] * LOG2E;
  // destination of tile row r's gradient (column origin col of the [3D] row)
  auto dst = [&](int r, int col) -> bf16raw* {
    if (!(r < used && row0 + r < total)) return nullptr;
    const long g = rows_of<CLS>(p, tile, G, r).grad;
    return (CLS && g < 0 ? dqkv_cls + (-1 - g) * p.ld_dqkv : dqkv + g * p.ld_dqkv) + col + h * HD;
  };
  put_tile<HD>(Ks, kf, fo);
  put_tile<HD>(Os, df, fo);
  if (lane < 32) { Ls[i] = l2; Ds[i] = dl; }
  const float c2 = p.scale * LOG2E;
  const int myseq = i / L;
  // ---- phase 1: lanes = queries.  dQ^T = K^T dS^T
  {
    f32x16 st, dp;
    zero16(st);
    zero16(dp);
#pragma unroll
    for (int ks = 0; ks < G_::NK; ++ks) {
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf.f[ks], qf.f[ks], st, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf.f[ks], df.f[ks], dp, 0, 0, 0);
    }
    float ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = crow(r, lane);
      const bool ok = valid && key < used && key / L == myseq && row0 + key < total;
      const float pr = ok ? __builtin_amdgcn_exp2f(st[r] * c2 - l2) : 0.f;
      ds[r] = pr * (dp[r] - dl) * p.scale;
    }
    wave_lds_sync();
    f32x16 acc[G_::NT];
#pragma unroll
    for (int n = 0; n < G_::NT; ++n) zero16(acc[n]);
    accum<HD>(acc, Ks, ds, fo);
    // K tile: its last reader was the MFMA chain above
    Geo<HD>::store_rows(Ks, acc, 1.0f, lane, [&](int r) -> bf16raw* { return dst(r, 0); });
  }
  // ---- phase 2: lanes = keys.  dV^T = dO^T P, dK^T = Q^T dS.  Only this phase's accumulators are live from here on.
  {
    put_tile<HD>(Qs, qf, fo);                      // tile A is free again: store_rows above ends with a wave-level sync
    wave_lds_sync();
    f32x16 st, dp;
    zero16(st);
    zero16(dp);
#pragma unroll
    for (int ks = 0; ks < G_::NK; ++ks) {
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf.f[ks], kf.f[ks], st, 0, 0, 0);
      // dO row fragments come back from tile B (it holds dO until dv is staged there) instead of living across the two phases
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows_o(Os + (ks >> 2) * Sm<HD>::SLAB, 0, ks & 3, fo), vf.f[ks], dp, 0, 0, 0);
    }
    float pr[16], ds[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int qrow = 8 * g + 4 * (lane >> 5);
      const float4 l4 = *reinterpret_cast<const float4*>(Ls + qrow);
      const float4 d4 = *reinterpret_cast<const float4*>(Ds + qrow);
      const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dvv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 4 * g + j;
        const int q = qrow + j;
        const bool ok = valid && q < used && q / L == myseq;
        const float e = ok ? __builtin_amdgcn_exp2f(st[r] * c2 - lv[j]) : 0.f;
        pr[r] = e;
        ds[r] = e * (dp[r] - dvv[j]) * p.scale;
      }
    }
    f32x16 dk[G_::NT], dv[G_::NT];
#pragma unroll
    for (int n = 0; n < G_::NT; ++n) { zero16(dk[n]); zero16(dv[n]); }
    accum<HD>(dv, Os, pr, fo);
    accum<HD>(dk, Qs, ds, fo);
    Geo<HD>::store_rows(Qs, dk, 1.0f, lane, [&](int r) -> bf16raw* { return dst(r, D); });
    Geo<HD>::store_rows(Os, dv, 1.0f, lane, [&](int r) -> bf16raw* { return dst(r, 2 * D); });
  }
}

// host side ---------------------------------------------------------------------------------------
// heads per workgroup: option value n > 0, capped at the head dim's MAXW waves and at H
template <int HD> static int hw_waves(int n, int H) { n = n < H ? n : H; return n < Sm<HD>::MAXW ? n : Sm<HD>::MAXW; }

template <int HD, bool CLS>
static int fwd_launch(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st) {
  const int G = 32 / p.L;
  const int ntiles = (p.S + G - 1) / G;
  if (options().attn_hw_fwd > 0) {
    const int w = hw_waves<HD>(options().attn_hw_fwd, p.H);
    hipLaunchKernelGGL((fwd_kernel<HD, true, CLS>), dim3((unsigned)cdiv(p.H, w) * ntiles), dim3(64 * w), (size_t)w * Sm<HD>::LDS_FWD, st, p, ntiles,
                       (const bf16raw*)qkv, (bf16raw*)out, lse);
  } else {
    hipLaunchKernelGGL((fwd_kernel<HD, false, CLS>), dim3((ntiles + 3) / 4, p.H), dim3(MA_THREADS), 4 * Sm<HD>::LDS_FWD, st, p, ntiles,
                       (const bf16raw*)qkv, (bf16raw*)out, lse);
  }
  return check_launch("attn_fwd_hd_small");
}
template <int HD, bool CLS>
static int bwd_launch(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, void* dqkv_cls,
                      hipStream_t st) {
  const int G = 32 / p.L;
  const int ntiles = (p.S + G - 1) / G;
  if (options().attn_hw_bwd > 0) {
    const int w = hw_waves<HD>(options().attn_hw_bwd, p.H);
    const size_t lds = (size_t)w * Sm<HD>::LDS_BWD;
    allow_lds<bwd_kernel<HD, true, CLS>>(lds);
    hipLaunchKernelGGL((bwd_kernel<HD, true, CLS>), dim3((unsigned)cdiv(p.H, w) * ntiles), dim3(64 * w), lds, st, p, ntiles, (const bf16raw*)qkv,
                       (const bf16raw*)o, (const bf16raw*)dout, lse, (bf16raw*)dqkv, (bf16raw*)dqkv_cls);
  } else {
    const size_t lds = (size_t)4 * Sm<HD>::LDS_BWD;
    allow_lds<bwd_kernel<HD, false, CLS>>(lds);
    hipLaunchKernelGGL((bwd_kernel<HD, false, CLS>), dim3((ntiles + 3) / 4, p.H), dim3(MA_THREADS), lds, st, p, ntiles, (const bf16raw*)qkv,
                       (const bf16raw*)o, (const bf16raw*)dout, lse, (bf16raw*)dqkv, (bf16raw*)dqkv_cls);
  }
  return check_launch("attn_bwd_hd_small");
}
template <int HD>
static int fwd_launch_m(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st) {
  return p.mode == VTX_ATTN_TIME_CLS ? fwd_launch<HD, true>(p, qkv, out, lse, st) : fwd_launch<HD, false>(p, qkv, out, lse, st);
}
template <int HD>
static int bwd_launch_m(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, void* dqkv_cls,
                        hipStream_t st) {
  return p.mode == VTX_ATTN_TIME_CLS ? bwd_launch<HD, true>(p, qkv, o, dout, lse, dqkv, dqkv_cls, st)
                                     : bwd_launch<HD, false>(p, qkv, o, dout, lse, dqkv, dqkv_cls, st);
}

}  // namespace hdsmall

bool attn_hd_eligible(int dtype, int L, int hd) { return dtype == VTX_BF16 && (hd == 32 || hd == 96 || hd == 128) && L > 32; }
// up to 32 tokens: the two layouts whose packed tile is addressed row by row (rows_of); SPACE and SPACE_NOCLS stay on the VALU kernels
bool attn_hd_small_eligible(int dtype, int mode, int L, int hd) {
  return dtype == VTX_BF16 && (hd == 32 || hd == 96 || hd == 128) && (mode == VTX_ATTN_CONTIG || mode == VTX_ATTN_TIME_CLS) && L >= 1 && L <= 32;
}

int attn_fwd_hd_small_launch(const AttnP& p, int hd, const void* qkv, void* out, float* lse, hipStream_t st) {
  switch (hd) {
    case 32: return hdsmall::fwd_launch_m<32>(p, qkv, out, lse, st);
    case 96: return hdsmall::fwd_launch_m<96>(p, qkv, out, lse, st);
    case 128: return hdsmall::fwd_launch_m<128>(p, qkv, out, lse, st);
  }
  VTX_REQUIRE(false, VTX_EINVAL, "attn_fwd_hd_small: head_dim %d", hd);
}

int attn_bwd_hd_small_launch(const AttnP& p, int hd, const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv,
                             void* dqkv_cls, hipStream_t st) {
  switch (hd) {
    case 32: return hdsmall::bwd_launch_m<32>(p, qkv, o, dout, lse, dqkv, dqkv_cls, st);
    case 96: return hdsmall::bwd_launch_m<96>(p, qkv, o, dout, lse, dqkv, dqkv_cls, st);
    case 128: return hdsmall::bwd_launch_m<128>(p, qkv, o, dout, lse, dqkv, dqkv_cls, st);
  }
  VTX_REQUIRE(false, VTX_EINVAL, "attn_bwd_hd_small: head_dim %d", hd);
}

int attn_fwd_hd_launch(const AttnP& p, int hd, const void* qkv, void* out, float* lse, hipStream_t st) {
  switch (hd) {
    case 32: return hdim::fwd_launch<32>(p, qkv, out, lse, st);
    case 96: return hdim::fwd_launch<96>(p, qkv, out, lse, st);
    case 128: return hdim::fwd_launch<128>(p, qkv, out, lse, st);
  }
  VTX_REQUIRE(false, VTX_EINVAL, "attn_fwd_hd: head_dim %d", hd);
}

int attn_bwd_hd_launch(const AttnP& p, int hd, const void* qkv, const void* o, const void* dout, const float* lse, float* delta,
                       void* dqkv, void* dqkv_cls, hipStream_t st) {
  switch (hd) {
    case 32: return hdim::bwd_launch<32>(p, qkv, o, dout, lse, delta, dqkv, dqkv_cls, st);
    case 96: return hdim::bwd_launch<96>(p, qkv, o, dout, lse, delta, dqkv, dqkv_cls, st);
    case 128: return hdim::bwd_launch<128>(p, qkv, o, dout, lse, delta, dqkv, dqkv_cls, st);
  }
  VTX_REQUIRE(false, VTX_EINVAL, "attn_bwd_hd: head_dim %d", hd);
}

}  // namespace vtx
