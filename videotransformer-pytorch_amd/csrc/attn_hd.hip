// attn_hd.hip -- bf16 MFMA attention core over the head dim: more than 32 tokens per sequence at head_dim 32, 96 and 128 in all
// four layouts (namespace hdim, described here), and the packed kernels for up to 32 tokens in the layouts CONTIG and TIME_CLS at
// head_dim 32, 64, 96 and 128 (at the end of the file).
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
// NOTE for whoever edits or moves the hdim kernels: the packed kernels at the end of this file compile to their present registers only
// with the hdim forward or dq kernel in the same translation unit; without them every attn_bwd_small_kernel comes out at its register cap
// (32: 90 -> 128), scratch at 64 and 128.  Cause not found: profiles/attn_small_refactor_bench.txt, 3b; test_attn_hd_small_host.py holds scratch at 0.
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

bool attn_hd_eligible(int dtype, int L, int hd) { return dtype == VTX_BF16 && (hd == 32 || hd == 96 || hd == 128) && L > 32; }

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

// =====================================================================================================================
// Up to 32 tokens, layouts CONTIG and TIME_CLS, head_dim 32, 64, 96 and 128: the packed kernels (attn_fwd_small_kernel /
// attn_bwd_small_kernel).  Temporal attention of the divided block (L = T = 8), T + 1 in the space-then-time order, ViViT's
// temporal encoder (L = 9).  The formulation is the one of attn_mfma.hip (read its header for the transposed scores and the
// swizzled tiles).
//
// G = 32 / L sequences are packed into one 32-row MFMA tile under a block-diagonal mask; ONE WAVE handles a (tile, head) pair end
// to end: the row fragments come straight from HBM (the row-wise fragment pattern covers the tile exactly once), the transposed
// operands sit in wave-private LDS tiles, whole rows are stored through the tile that has just gone idle, delta is neither read
// nor written.  HBM-bound: the forward moves 4 and the backward 8 row-blocks of [rows][HD] per head.
// A wave-private tile is Bf16Tiles<HD, 64>::NS slabs of the swizzled [32][64] tile (4 KiB at head_dim 32 and 64, 8 KiB at 96
// and 128; the upper half of the last slab is never written and never read at 32 and 96: a 32-column slab would need a swizzle
// and readers of its own for 2 KiB a wave).  Forward: one tile (V).  Backward: tile A (K, then Q), tile B (dO) and 32 lse + 32
// delta: 8.25 KiB at one slab, 16.25 KiB at two -- that is what bounds the waves of a CU there (9 of them in 160 KiB; a workgroup
// of 4 takes 65 KiB, hence the opt-in), and the register bound follows it: two waves a SIMD, 256 registers.
//
// What differs per head dim is Small<HD> and nothing else.  Why head_dim 64 is here and not in a file of the packed kernels: the NOTE at the top.
// =====================================================================================================================

// How a lane finds its pieces of a swizzled [32][64] slab.  FragOff (attn_common.h) keeps the 12 per-lane offsets in registers;
// LaneIdx computes them at each read with the generic readers frag_rows / frag_cols.  The backward at head_dim 64 is bound to
// four waves a SIMD = 128 registers and has no room for the 12 (profiles/attn_small_refactor_bench.txt, section 3c).
struct LaneIdx { int lane; };
__device__ __forceinline__ void make_reader(LaneIdx& r, int lane) { r.lane = lane; }
__device__ __forceinline__ void make_reader(FragOff& r, int lane) { r = make_frag_off(lane); }
// element offset of this lane's piece ks of its row (lane & 31)
__device__ __forceinline__ int row_piece(int ks, const LaneIdx& r) { return sw_off(r.lane & 31, 16 * ks + 8 * (r.lane >> 5)); }
__device__ __forceinline__ int row_piece(int ks, const FragOff& r) { return r.rows[ks]; }
__device__ __forceinline__ bf16x8 read_rows(const bf16raw* t, int ks, const LaneIdx& r) { return frag_rows(t, 0, ks, r.lane); }
__device__ __forceinline__ bf16x8 read_rows(const bf16raw* t, int ks, const FragOff& r) { return frag_rows_o(t, 0, ks, r); }
__device__ __forceinline__ bf16x8 read_cols(const bf16raw* t, int row0, int n2, const LaneIdx& r) { return frag_cols(t, row0, n2 * 32, r.lane); }
__device__ __forceinline__ bf16x8 read_cols(const bf16raw* t, int row0, int n2, const FragOff& r) { return frag_cols_o(t, row0, n2, r); }

template <int HD> struct SmallReader { typedef FragOff type; };
template <> struct SmallReader<64> { typedef LaneIdx type; };
template <int HD> struct Small {
  typedef Bf16Tiles<HD, 64> Geo;                                         // NS / NK / NT, Frag and store_rows of a head
  typedef typename Geo::Frag Frag;
  typedef typename SmallReader<HD>::type Reader;
  static constexpr int SLAB = 32 * 64;                                   // elements of one [32][64] slab
  static constexpr int TILE = Geo::NS * SLAB;
  static constexpr int LDS_FWD = TILE * 2;                               // V tile
  static constexpr int LDS_BWD = 2 * TILE * 2 + 2 * 32 * 4;              // tile A (K, then Q), tile B (dO) + lse + delta
  // Waves of a heads-per-workgroup launch.  8 at 96 / 128 for the forward's registers and the backward's LDS (D = 768 has 8 and
  // 6 heads there), at 32 because 8 heads measured faster than 16 (profiles/attn_hd_small_bench.txt); 16 at 64 (D = 768: 12 heads).
  static constexpr int MAXW = HD == 64 ? 16 : 8;
  static constexpr int BWD_BLOCKS = HD <= 64 ? 4 : 2;                    // minimum workgroups a CU of the four-tile backward
  // dv and dk fed from one loop, not one accum after the other (same products and order per accumulator): keeps the lse / delta reads whole
  static constexpr bool PAIRED = HD == 64;
};

// Rows of a packed tile.  Tile row j < used belongs to sequence sq = tile * G + j / L, token i = j % L.  CONTIG: all tensors
// hold it at row0 + j.  CLS (VTX_ATTN_TIME_CLS, sequence (b, p) = the clip's cls row + T consecutive token rows): qkv holds
// token i >= 1 at sq * T + b + i and the cls row at b * (1 + P*T); out / dout hold it at sq * T + i - 1, the sequence's cls
// row behind the B*P*T token rows; the gradient of the gathered cls row goes to dqkv_cls[sq], the P of them of a clip are
// summed by vtx_cls_qkv_reduce.  lse is [S, H, L] in every layout: index (sq * H + h) * L + i.
struct SmallRows {
  long in, out;          // rows of qkv / of out and dout
  long grad;             // row of dqkv, or -1 - (row of dqkv_cls)
  long lse;              // sq * H * L + i (without the head)
};
template <bool CLS>
__device__ inline SmallRows small_rows(const AttnP& p, int tile, int G, int j) {
  SmallRows r;
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
__device__ __forceinline__ void load_frags(typename Small<HD>::Frag& f, const bf16raw* base, long ld, int col0, long row, bool valid, int lane) {
#pragma unroll
  for (int ks = 0; ks < Small<HD>::Geo::NK; ++ks) {
    union { bf16x8 v; uint4 u; } x;
    x.u = make_uint4(0, 0, 0, 0);
    if (valid) x.u = *reinterpret_cast<const uint4*>(base + row * ld + col0 + ks * 16 + 8 * (lane >> 5));
    f.f[ks] = x.v;
  }
}
// The row fragments of a 32-row tile (one row per lane) into the wave's tile, slab by slab.
template <int HD>
__device__ __forceinline__ void put_tile(bf16raw* t, const typename Small<HD>::Frag& f, const typename Small<HD>::Reader& rd) {
#pragma unroll
  for (int ks = 0; ks < Small<HD>::Geo::NK; ++ks) *reinterpret_cast<bf16x8*>(t + (ks >> 2) * Small<HD>::SLAB + row_piece(ks & 3, rd)) = f.f[ks];
}
// acc[n][d][j] += sum_i tile[i][32 n + d] c[i][j] over the tile's 32 rows, c = 16 values per lane in accumulator order
template <int HD>
__device__ __forceinline__ void accum(f32x16 (&acc)[Small<HD>::Geo::NT], const bf16raw* t, const float* c, const typename Small<HD>::Reader& rd) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const bf16x8 pb = pack8(c + 8 * s2);
#pragma unroll
    for (int n = 0; n < Small<HD>::Geo::NT; ++n)
      acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_cols(t + (n >> 1) * Small<HD>::SLAB, 16 * s2, n & 1, rd), pb, acc[n], 0, 0, 0);
  }
}

struct SmallWho {
  int lane, wave, tile, h;
  bool run;
};
// HW (heads in the workgroup): wave w of a workgroup works on head w of ONE row tile's head group, so that the workgroup as a
// whole reads the tile's rows contiguously at one moment -- instead of one 128-B line out of every row per workgroup, with the
// other heads' lines of the same rows requested by other CUs at other times.  (head group, tile) is folded into blockIdx.x
// (grid.y stops at 65535), head group fastest: the groups of a tile are CONSECUTIVE workgroups, they run at the same time and
// read neighbouring segments of the same rows (temporal backward, 4 heads per workgroup: 356 -> 332 us against tile fastest).
// Otherwise one head (blockIdx.y) and four row tiles per workgroup.
template <bool HW>
__device__ inline SmallWho small_who(const AttnP& p, int ntiles) {
  SmallWho w;
  w.lane = threadIdx.x & 63;
  w.wave = threadIdx.x >> 6;
  const int hw_w = blockDim.x >> 6, hw_ng = HW ? (p.H + hw_w - 1) / hw_w : 1;
  w.tile = HW ? (int)(blockIdx.x / hw_ng) : blockIdx.x * 4 + w.wave;
  w.h = HW ? w.wave + (int)(blockIdx.x % hw_ng) * hw_w : blockIdx.y;
  w.run = w.tile < ntiles && w.h < p.H;
  return w;
}

template <int HD, bool HW, bool CLS>
__global__ __launch_bounds__(HW ? 64 * Small<HD>::MAXW : MA_THREADS) void attn_fwd_small_kernel(AttnP p, int ntiles, const bf16raw* __restrict__ qkv,
                                                                                          bf16raw* __restrict__ out, float* __restrict__ lse) {
  typedef Small<HD> Sm;
  typedef typename Sm::Geo Geo;
  extern __shared__ __attribute__((aligned(16))) char sm_raw[];
  const SmallWho w = small_who<HW>(p, ntiles);
  if (!w.run) return;                              // (no workgroup barrier below: a wave is on its own)
  const int lane = w.lane, h = w.h, tile = w.tile, D = p.H * HD;
  bf16raw* Vs = reinterpret_cast<bf16raw*>(sm_raw + w.wave * Sm::LDS_FWD);
  const int L = p.L, G = 32 / L, used = G * L;
  const long row0 = (long)tile * used, total = (long)p.S * L;
  const int i = lane & 31;
  const bool valid = i < used && row0 + i < total;
  const SmallRows me = small_rows<CLS>(p, tile, G, valid ? i : 0);
  typename Sm::Reader rd;
  make_reader(rd, lane);
  typename Sm::Frag qf, kf, vf;
  load_frags<HD>(qf, qkv, p.ld_qkv, h * HD, me.in, valid, lane);
  load_frags<HD>(kf, qkv, p.ld_qkv, D + h * HD, me.in, valid, lane);
  load_frags<HD>(vf, qkv, p.ld_qkv, 2 * D + h * HD, me.in, valid, lane);
  put_tile<HD>(Vs, vf, rd);
  f32x16 st;
  zero16(st);
#pragma unroll
  for (int ks = 0; ks < Geo::NK; ++ks) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf.f[ks], qf.f[ks], st, 0, 0, 0);
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
  f32x16 acc[Geo::NT];
#pragma unroll
  for (int n = 0; n < Geo::NT; ++n) zero16(acc[n]);
  accum<HD>(acc, Vs, pr, rd);
  // whole rows through the (now idle) V tile: a direct store writes 8-byte pieces of 32 different rows per instruction
  Geo::store_rows(Vs, acc, valid ? 1.0f / l : 0.f, lane, [&](int r) -> bf16raw* {
    return (r < used && row0 + r < total) ? out + small_rows<CLS>(p, tile, G, r).out * p.ld_out + h * HD : nullptr;
  });
  if (valid && lane < 32) lse[me.lse + (long)h * L] = m * LN2 + __logf(l);
}

template <int HD, bool HW, bool CLS>
__global__ __launch_bounds__(HW ? 64 * Small<HD>::MAXW : MA_THREADS, HW ? 1 : Small<HD>::BWD_BLOCKS) void attn_bwd_small_kernel(
    AttnP p, int ntiles, const bf16raw* __restrict__ qkv, const bf16raw* __restrict__ o, const bf16raw* __restrict__ dout,
    const float* __restrict__ lse, bf16raw* __restrict__ dqkv, bf16raw* __restrict__ dqkv_cls) {
  typedef Small<HD> Sm;
  typedef typename Sm::Geo Geo;
  extern __shared__ __attribute__((aligned(16))) char sm_raw[];
  const SmallWho w = small_who<HW>(p, ntiles);
  if (!w.run) return;
  const int lane = w.lane, h = w.h, tile = w.tile, D = p.H * HD;
  // two wave-private tiles: A holds K for phase 1 (and stages dQ), then Q for phase 2 (and stages dK); B holds dO (and stages
  // dV) -- a third of the LDS less than a tile per operand: LDS is what bounds the waves per CU of this kernel
  char* wl = sm_raw + w.wave * Sm::LDS_BWD;
  bf16raw* Ks = reinterpret_cast<bf16raw*>(wl);
  bf16raw* Qs = Ks;
  bf16raw* Os = Ks + Sm::TILE;
  float* Ls = reinterpret_cast<float*>(Os + Sm::TILE);
  float* Ds = Ls + 32;
  const int L = p.L, G = 32 / L, used = G * L;
  const long row0 = (long)tile * used, total = (long)p.S * L;
  const int i = lane & 31;
  const bool valid = i < used && row0 + i < total;
  const SmallRows me = small_rows<CLS>(p, tile, G, valid ? i : 0);
  typename Sm::Reader rd;
  make_reader(rd, lane);
  typename Sm::Frag qf, kf, vf, df;
  load_frags<HD>(qf, qkv, p.ld_qkv, h * HD, me.in, valid, lane);
  load_frags<HD>(kf, qkv, p.ld_qkv, D + h * HD, me.in, valid, lane);
  load_frags<HD>(vf, qkv, p.ld_qkv, 2 * D + h * HD, me.in, valid, lane);
  load_frags<HD>(df, dout, p.ld_dout, h * HD, me.out, valid, lane);
  float dl = 0.f;
  {
    typename Sm::Frag of;
    load_frags<HD>(of, o, p.ld_out, h * HD, me.out, valid, lane);
#pragma unroll
    for (int ks = 0; ks < Geo::NK; ++ks) dl += frag_dot(df.f[ks], of.f[ks]);
  }
  dl += __shfl_xor(dl, 32, 64);
  float l2 = 1e30f;
  if (valid) l2 = lse[me.lse + (long)h * L] * LOG2E;
  // destination of tile row r's gradient (column origin col of the [3D] row)
  auto dst = [&](int r, int col) -> bf16raw* {
    if (!(r < used && row0 + r < total)) return nullptr;
    const long g = small_rows<CLS>(p, tile, G, r).grad;
    return (CLS && g < 0 ? dqkv_cls + (-1 - g) * p.ld_dqkv : dqkv + g * p.ld_dqkv) + col + h * HD;
  };
  put_tile<HD>(Ks, kf, rd);
  put_tile<HD>(Os, df, rd);
  if (lane < 32) { Ls[i] = l2; Ds[i] = dl; }
  const float c2 = p.scale * LOG2E;
  const int myseq = i / L;
  // ---- phase 1: lanes = queries.  dQ^T = K^T dS^T
  {
    f32x16 st, dp;
    zero16(st);
    zero16(dp);
#pragma unroll
    for (int ks = 0; ks < Geo::NK; ++ks) {
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
    f32x16 acc[Geo::NT];
#pragma unroll
    for (int n = 0; n < Geo::NT; ++n) zero16(acc[n]);
    accum<HD>(acc, Ks, ds, rd);
    // K tile: its last reader was the MFMA chain above
    Geo::store_rows(Ks, acc, 1.0f, lane, [&](int r) -> bf16raw* { return dst(r, 0); });
  }
  // ---- phase 2: lanes = keys.  dV^T = dO^T P, dK^T = Q^T dS.  Only this phase's accumulators are live from here on.
  {
    put_tile<HD>(Qs, qf, rd);                      // tile A is free again: store_rows above ends with a wave-level sync
    wave_lds_sync();
    f32x16 st, dp;
    zero16(st);
    zero16(dp);
#pragma unroll
    for (int ks = 0; ks < Geo::NK; ++ks) {
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf.f[ks], kf.f[ks], st, 0, 0, 0);
      // dO row fragments come back from tile B (it holds dO until dv is staged there): kept in registers across the two
      // phases they cost head_dim 64 its fourth wave a SIMD
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_rows(Os + (ks >> 2) * Sm::SLAB, ks & 3, rd), vf.f[ks], dp, 0, 0, 0);
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
    f32x16 dk[Geo::NT], dv[Geo::NT];
#pragma unroll
    for (int n = 0; n < Geo::NT; ++n) { zero16(dk[n]); zero16(dv[n]); }
    if constexpr (Sm::PAIRED) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pb = pack8(pr + 8 * s2);
        const bf16x8 db = pack8(ds + 8 * s2);
#pragma unroll
        for (int n = 0; n < Geo::NT; ++n) {
          dv[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_cols(Os + (n >> 1) * Sm::SLAB, 16 * s2, n & 1, rd), pb, dv[n], 0, 0, 0);
          dk[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_cols(Qs + (n >> 1) * Sm::SLAB, 16 * s2, n & 1, rd), db, dk[n], 0, 0, 0);
        }
      }
    } else {
      accum<HD>(dv, Os, pr, rd);
      accum<HD>(dk, Qs, ds, rd);
    }
    Geo::store_rows(Qs, dk, 1.0f, lane, [&](int r) -> bf16raw* { return dst(r, D); });
    Geo::store_rows(Os, dv, 1.0f, lane, [&](int r) -> bf16raw* { return dst(r, 2 * D); });
  }
}

// host side ---------------------------------------------------------------------------------------
// the two layouts whose packed tile is addressed row by row (small_rows); SPACE and SPACE_NOCLS of up to 32 tokens run elsewhere
bool attn_small_eligible(int dtype, int mode, int L, int hd) {
  return dtype == VTX_BF16 && (hd == 32 || hd == 64 || hd == 96 || hd == 128) && (mode == VTX_ATTN_CONTIG || mode == VTX_ATTN_TIME_CLS) &&
         L >= 1 && L <= 32;
}

// Grid, block and dynamic LDS of a launch: hw > 0 heads of a row tile per workgroup (capped at maxw waves and at H), else one head, four tiles
struct SmallGeom { dim3 grid, block; size_t lds; int ntiles; };
static SmallGeom small_geom(const AttnP& p, int hw, int maxw, size_t wave_lds) {
  const int G = 32 / p.L;
  const int ntiles = (p.S + G - 1) / G;
  if (hw <= 0) return {dim3((ntiles + 3) / 4, p.H), dim3(MA_THREADS), 4 * wave_lds, ntiles};
  int w = hw < p.H ? hw : p.H;
  if (w > maxw) w = maxw;
  return {dim3((unsigned)cdiv(p.H, w) * ntiles), dim3(64 * w), w * wave_lds, ntiles};
}

template <int HD, bool HW, bool CLS>
static int fwd_launch(const AttnP& p, const SmallGeom& g, const void* qkv, void* out, float* lse, hipStream_t st) {
  hipLaunchKernelGGL((attn_fwd_small_kernel<HD, HW, CLS>), g.grid, g.block, g.lds, st, p, g.ntiles, (const bf16raw*)qkv, (bf16raw*)out, lse);
  return check_launch("attn_fwd_small");
}
template <int HD, bool HW, bool CLS>
static int bwd_launch(const AttnP& p, const SmallGeom& g, const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv,
                      void* dqkv_cls, hipStream_t st) {
  allow_lds<attn_bwd_small_kernel<HD, HW, CLS>>(g.lds);
  hipLaunchKernelGGL((attn_bwd_small_kernel<HD, HW, CLS>), g.grid, g.block, g.lds, st, p, g.ntiles, (const bf16raw*)qkv, (const bf16raw*)o,
                     (const bf16raw*)dout, lse, (bf16raw*)dqkv, (bf16raw*)dqkv_cls);
  return check_launch("attn_bwd_small");
}

// the instantiation for the run-time workgroup shape (attn_hw_* > 0: heads of a tile) and layout
template <int HD>
static int fwd_launch_hd(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st) {
  const int hw = options().attn_hw_fwd;
  const bool cls = p.mode == VTX_ATTN_TIME_CLS;
  const SmallGeom g = small_geom(p, hw, Small<HD>::MAXW, Small<HD>::LDS_FWD);
  if (hw > 0) return cls ? fwd_launch<HD, true, true>(p, g, qkv, out, lse, st) : fwd_launch<HD, true, false>(p, g, qkv, out, lse, st);
  return cls ? fwd_launch<HD, false, true>(p, g, qkv, out, lse, st) : fwd_launch<HD, false, false>(p, g, qkv, out, lse, st);
}
template <int HD>
static int bwd_launch_hd(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, void* dqkv_cls,
                         hipStream_t st) {
  const int hw = options().attn_hw_bwd;
  const bool cls = p.mode == VTX_ATTN_TIME_CLS;
  const SmallGeom g = small_geom(p, hw, Small<HD>::MAXW, Small<HD>::LDS_BWD);
  if (hw > 0)
    return cls ? bwd_launch<HD, true, true>(p, g, qkv, o, dout, lse, dqkv, dqkv_cls, st)
               : bwd_launch<HD, true, false>(p, g, qkv, o, dout, lse, dqkv, dqkv_cls, st);
  return cls ? bwd_launch<HD, false, true>(p, g, qkv, o, dout, lse, dqkv, dqkv_cls, st)
             : bwd_launch<HD, false, false>(p, g, qkv, o, dout, lse, dqkv, dqkv_cls, st);
}

int attn_fwd_small_launch(const AttnP& p, int hd, const void* qkv, void* out, float* lse, hipStream_t st) {
  switch (hd) {
    case 32: return fwd_launch_hd<32>(p, qkv, out, lse, st);
    case 64: return fwd_launch_hd<64>(p, qkv, out, lse, st);
    case 96: return fwd_launch_hd<96>(p, qkv, out, lse, st);
    case 128: return fwd_launch_hd<128>(p, qkv, out, lse, st);
  }
  VTX_REQUIRE(false, VTX_EINVAL, "attn_fwd_small: head_dim %d", hd);
}

int attn_bwd_small_launch(const AttnP& p, int hd, const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv,
                          void* dqkv_cls, hipStream_t st) {
  switch (hd) {
    case 32: return bwd_launch_hd<32>(p, qkv, o, dout, lse, dqkv, dqkv_cls, st);
    case 64: return bwd_launch_hd<64>(p, qkv, o, dout, lse, dqkv, dqkv_cls, st);
    case 96: return bwd_launch_hd<96>(p, qkv, o, dout, lse, dqkv, dqkv_cls, st);
    case 128: return bwd_launch_hd<128>(p, qkv, o, dout, lse, dqkv, dqkv_cls, st);
  }
  VTX_REQUIRE(false, VTX_EINVAL, "attn_bwd_small: head_dim %d", hd);
}

}  // namespace vtx
