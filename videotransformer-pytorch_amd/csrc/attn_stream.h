// attn_stream.h -- the chunk-streaming attention kernels (forward, dq, dk / dv) for sequences that do not fit the LDS of one
// workgroup, written once over a tile policy E, for both element types and every head dim.  The two policy templates are
// Bf16Tiles<HD, CHUNK> (attn_tiles_bf16.h: v_mfma_f32_32x32x16_bf16) and F32Tiles<HD, CHUNK> (attn_tiles_f32.h: exact fp32,
// v_mfma_f32_32x32x2_f32); attn_long.hip and attn_f32.hip (head_dim 64) and attn_hd_f32.hip (fp32 at 32, 96, 128) each
// instantiate a policy per kernel and hold three one-line __global__ kernels; everything else is here.  (attn_hd.hip, bf16 at
// 32, 96 and 128, uses the bf16 policy under three bodies of its own: see its header.)
//
// Scores are computed TRANSPOSED, so that a lane owns a query column (forward, dq) or a key column (dk / dv):
//   forward, dq : a workgroup of 4 waves owns 128 queries of one (sequence, head), a wave 32 of them (row fragments in
//                 registers); K and V stream through LDS in chunks of E::CHUNK keys.  Forward: online softmax per chunk
//                 (running max m of the raw scores, sum l, rescale of the O^T accumulator).  dq: P recomputed from the
//                 saved lse; delta = rowsum(dO * O) is computed in the prologue and written for the dk / dv kernel.
//   dk / dv     : a workgroup owns 128 keys (a wave: one 32-key tile) and streams ALL queries of its sequence
//                 (Q, dO, lse, delta) in chunks of E::CHUNK.  One workgroup sees every query of its keys: no partial sums,
//                 no workspace, no atomics, a fixed summation order -- two runs are bit-identical.
// Chunks are double buffered: the global loads of chunk c + 1 are issued into registers before the products of chunk c
// and written to the other LDS stage behind them, one workgroup barrier per chunk.  A stage is two [CHUNK][HD] tiles in the
// policy's layout; the dk / dv kernel adds [stage][lse | delta][CHUNK] floats.  The other workgroups of the CU (the kernels'
// launch bounds say how many) run their softmax and chunk stores beside this one's matrix instructions.  The row-store staging
// tiles reuse the stages after the last chunk.  Grid: S * ceil(L / 128) x H workgroups for each of the three kernels.
//
// Masking: keys >= L of the last chunk have zero K / V rows and score -1e30 before the max (P = 0 exactly; every chunk holds
// at least one real key, so a chunk maximum is always finite and exp2(m_old - m_new) never sees inf - inf); a 32-row tile
// wholly beyond L is skipped.  Query rows >= L keep to their lane (operands clamped to row L - 1) and are never stored; in
// the dk / dv kernel padded query rows carry lse = +1e30 (P = 0) and zero Q / dO rows.
// FLOPs per (sequence, head): forward 4 L^2 HD, backward 10 L^2 HD (+ 4 L^2 HD recomputed scores).
//
// The policy E carries what differs between the element types and nothing else:
//   elem, HD, NT                          element type; columns of a head; f32x16 accumulator tiles of a result row (HD / 32)
//   CHUNK, TILE, STAGE, STG               rows per chunk; elements of a tile, of a stage, of a wave's staging tile
//   Pre, chunk_load, chunk_store          two operands' rows of one chunk in flight; global -> registers; registers -> LDS tiles
//   Frag, load_frag, frag_dot             a row's HD columns (this lane's half) in registers; its load; sum_d a[d] b[d] of the half
//   Lane, make_lane                       per-lane LDS offsets of the tile readers
//   scores(tile, row0, frag, lane)        C[i][j] = sum_d tile[row0 + i][d] frag_j[d] for 32 tile rows, as an f32x16 MFMA tile
//   accum(acc, tile, row0, c, lane)       acc[n][d][j] += sum_i tile[row0 + i][32 n + d] c[i][j], c as scores() left it
//   store_rows(stg, acc, mul, lane, fn)   [32 x HD] result held transposed -> whole global rows through the staging tile
//   MASK_PADDED_DS                        dq: zero the dS of padded keys before accum (bf16: keeps the pack clean; fp32: the
//                                         zero K rows already do it, and masking would turn -0 into +0)
//   dkv_tile(dk, dv, Qs, Os, Ls, Ds, ..)  the dk / dv products of one 32-query tile: P = exp2(S c2 - lse), dv += dO^T P,
//                                         dS = P (dP - delta), dk += Q^T dS.  Which of the four independent accumulators
//                                         (S, dP, dv, dk) is fed when is the policy's: bf16 interleaves the S and dP chains and
//                                         feeds dv and dk together (dependent 32x32x16 MFMAs back to back stall, and the
//                                         compiler packs the dP - delta subtractions only when both statistics are at hand);
//                                         fp32 goes S -> P -> dv -> dP -> dS -> dk so that S and dP are never live together
//                                         (252 of 256 registers at head_dim 64).  One order for both costs the bf16 kernel 17
//                                         more hazard s_nops and its packed adds, or the fp32 kernel its registers.
// The kernels of one backward need not share a chunk size (fp32 at head_dim 96 and 128: attn_hd_f32.hip), so the launchers take
// a policy per kernel, and the dynamic LDS of a launch is that kernel's policy's.
#pragma once
#include "attn_common.h"

namespace vtx {

constexpr int AS_THREADS = 256;
constexpr int AS_ROWS = 128;                       // queries (keys in the dk / dv kernel) of one workgroup: 4 waves x 32

// What every kernel starts with: who am I, which rows are mine.
struct StreamWho {
  int lane, wave, h, D, s, row0, row;              // row0: first of the wave's 32 rows; row: this lane's
  bool active;                                     // wave-uniform; an idle wave still fills and meets the barriers
  RowLin li, lo;
};
__device__ inline StreamWho stream_who(const AttnP& p, int hd) {
  StreamWho w;
  w.lane = threadIdx.x & 63;
  w.wave = threadIdx.x >> 6;
  w.h = blockIdx.y;
  w.D = p.H * hd;
  const int nb = (p.L + AS_ROWS - 1) / AS_ROWS;    // blockIdx.x -> (sequence, 128-row block of that sequence)
  w.s = blockIdx.x / nb;
  w.row0 = (blockIdx.x - w.s * nb) * AS_ROWS + w.wave * 32;
  w.row = w.row0 + (w.lane & 31);
  w.active = w.row0 < p.L;
  w.li = lin_in(p, w.s);
  w.lo = lin_out(p, w.s);
  return w;
}

template <class E>
__device__ inline typename E::elem* stream_lds() {
  static_assert(4 * E::STG <= 2 * E::STAGE, "four staging tiles fit in the two stages");
  extern __shared__ __attribute__((aligned(16))) char sm_raw[];
  return reinterpret_cast<typename E::elem*>(sm_raw);
}

// ------------------------------------------------------------------------------------------------ forward
template <class E>
__device__ __forceinline__ void stream_fwd(const AttnP& p, const typename E::elem* __restrict__ qkv, typename E::elem* __restrict__ out,
                                           float* __restrict__ lse) {
  typedef typename E::elem T;
  constexpr int CHUNK = E::CHUNK, KC = CHUNK / 32;
  T* sm = stream_lds<E>();
  const StreamWho w = stream_who(p, E::HD);
  const int lane = w.lane, h = w.h;
  const T* kb = qkv + w.D + h * E::HD;
  const T* vb = qkv + 2 * w.D + h * E::HD;
  typename E::Frag qf;
  E::load_frag(qf, qkv, p.ld_qkv, h * E::HD, w.li, w.row, p.L, lane);
  typename E::Pre pre;
  E::chunk_load(pre, kb, p.ld_qkv, w.li, vb, p.ld_qkv, w.li, 0, p.L);
  E::chunk_store(pre, sm, sm + E::TILE);
  __syncthreads();
  const typename E::Lane ln = E::make_lane(lane);
  const float c2 = p.scale * LOG2E;
  f32x16 acc[E::NT];
#pragma unroll
  for (int n = 0; n < E::NT; ++n) zero16(acc[n]);
  float m = -1e30f, l = 0.f;                       // running max of the RAW scores (scale > 0)
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const T* Ks = sm + (c & 1) * E::STAGE;
    const T* Vs = Ks + E::TILE;
    E::chunk_load(pre, kb, p.ld_qkv, w.li, vb, p.ld_qkv, w.li, (c + 1) * CHUNK, p.L);
    if (w.active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
      f32x16 st[KC];                               // (tiles beyond nt stay undefined: every use below is guarded)
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) st[t] = E::scores(Ks, t * 32, qf, ln);
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
        for (int n = 0; n < E::NT; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[n][r] *= alpha;
      }
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) E::accum(acc, Vs, t * 32, st[t], ln);
    }
    if (c + 1 < nch) {
      T* nx = sm + ((c + 1) & 1) * E::STAGE;       // last read in iteration c - 1, behind that iteration's barrier
      E::chunk_store(pre, nx, nx + E::TILE);
    }
    __syncthreads();
  }
  if (!w.active) return;
  T* stg = sm + w.wave * E::STG;                   // every wave is past the last chunk: the stages are free
  E::store_rows(stg, acc, 1.0f / l, lane, [&](int r) -> T* {
    const int qq = w.row0 + r;
    return qq < p.L ? out + lin_row(w.lo, qq) * p.ld_out + h * E::HD : nullptr;
  });
  if (w.row < p.L && lane < 32) lse[((long)w.s * p.H + h) * p.L + w.row] = (m * c2) * LN2 + __logf(l);
}

// ------------------------------------------------------------------------------------------------ backward: dq (+ delta)
template <class E>
__device__ __forceinline__ void stream_bwd_dq(const AttnP& p, const typename E::elem* __restrict__ qkv, const typename E::elem* __restrict__ o,
                                              const typename E::elem* __restrict__ dout, const float* __restrict__ lse,
                                              float* __restrict__ delta, typename E::elem* __restrict__ dqkv,
                                              typename E::elem* __restrict__ dqkv_cls) {
  typedef typename E::elem T;
  constexpr int CHUNK = E::CHUNK, KC = CHUNK / 32;
  T* sm = stream_lds<E>();
  const StreamWho w = stream_who(p, E::HD);
  const int lane = w.lane, h = w.h;
  const T* kb = qkv + w.D + h * E::HD;
  const T* vb = qkv + 2 * w.D + h * E::HD;
  typename E::Frag qf, df;
  float dl;                                        // delta = rowsum(dO * O): this lane's half of the row's columns
  {
    typename E::Frag of;
    E::load_frag(qf, qkv, p.ld_qkv, h * E::HD, w.li, w.row, p.L, lane);
    E::load_frag(df, dout, p.ld_dout, h * E::HD, w.lo, w.row, p.L, lane);
    E::load_frag(of, o, p.ld_out, h * E::HD, w.lo, w.row, p.L, lane);
    dl = E::frag_dot(df, of);
  }
  dl += __shfl_xor(dl, 32, 64);
  float l2 = 0.f;
  if (w.row < p.L) {
    const long lidx = ((long)w.s * p.H + h) * p.L + w.row;
    l2 = lse[lidx] * LOG2E;
    if (lane < 32) delta[lidx] = dl;
  }
  typename E::Pre pre;
  E::chunk_load(pre, kb, p.ld_qkv, w.li, vb, p.ld_qkv, w.li, 0, p.L);
  E::chunk_store(pre, sm, sm + E::TILE);
  __syncthreads();
  const typename E::Lane ln = E::make_lane(lane);
  const float c2 = p.scale * LOG2E;
  f32x16 acc[E::NT];
#pragma unroll
  for (int n = 0; n < E::NT; ++n) zero16(acc[n]);
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const T* Ks = sm + (c & 1) * E::STAGE;
    const T* Vs = Ks + E::TILE;
    E::chunk_load(pre, kb, p.ld_qkv, w.li, vb, p.ld_qkv, w.li, (c + 1) * CHUNK, p.L);
    if (w.active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) {
          const f32x16 st = E::scores(Ks, t * 32, qf, ln);
          f32x16 ds = E::scores(Vs, t * 32, df, ln);
          // dS = P (dP - delta); the softmax scale is applied once to dq at the store.  A padded key has zero K and V rows:
          // its dS is finite and multiplies zeros (MASK_PADDED_DS: see the policy table above).
#pragma unroll
          for (int r = 0; r < 16; ++r) ds[r] = __builtin_amdgcn_exp2f(fmaf(st[r], c2, -l2)) * (ds[r] - dl);
          if (E::MASK_PADDED_DS && t * 32 + 32 > nrows) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (t * 32 + crow(r, lane) >= nrows) ds[r] = 0.f;
          }
          E::accum(acc, Ks, t * 32, ds, ln);
        }
    }
    if (c + 1 < nch) {
      T* nx = sm + ((c + 1) & 1) * E::STAGE;
      E::chunk_store(pre, nx, nx + E::TILE);
    }
    __syncthreads();
  }
  if (!w.active) return;
  T* stg = sm + w.wave * E::STG;
  E::store_rows(stg, acc, p.scale, lane, [&](int r) -> T* {
    const int qq = w.row0 + r;
    if (qq >= p.L) return nullptr;
    return attn_cls_row(p, qq) ? dqkv_cls + (long)w.s * p.ld_dqkv + h * E::HD
                                                  : dqkv + lin_row(w.li, qq) * p.ld_dqkv + h * E::HD;
  });
}

// ------------------------------------------------------------------------------------------------ backward: dk, dv
// Lanes = keys: wave w of the workgroup of key block kb owns the key tile kb * 4 + w and walks ALL queries of the sequence.
template <class E>
__device__ __forceinline__ void stream_bwd_dkv(const AttnP& p, const typename E::elem* __restrict__ qkv,
                                               const typename E::elem* __restrict__ dout, const float* __restrict__ lse,
                                               const float* __restrict__ delta, typename E::elem* __restrict__ dqkv,
                                               typename E::elem* __restrict__ dqkv_cls) {
  typedef typename E::elem T;
  constexpr int CHUNK = E::CHUNK, QC = CHUNK / 32;
  T* sm = stream_lds<E>();
  float* stats = reinterpret_cast<float*>(sm + 2 * E::STAGE);    // [stage][lse * log2(e) | delta][CHUNK]
  const StreamWho w = stream_who(p, E::HD);
  const int lane = w.lane, h = w.h, D = w.D;
  const T* qb = qkv + h * E::HD;
  const T* ob = dout + h * E::HD;
  const float* lb = lse + ((long)w.s * p.H + h) * p.L;
  const float* db = delta + ((long)w.s * p.H + h) * p.L;
  typename E::Frag kf, vf;
  E::load_frag(kf, qkv, p.ld_qkv, D + h * E::HD, w.li, w.row, p.L, lane);
  E::load_frag(vf, qkv, p.ld_qkv, 2 * D + h * E::HD, w.li, w.row, p.L, lane);
  // thread t < CHUNK: lse of chunk row t (scaled; +huge on padded rows -> P = 0); CHUNK <= t < 2 CHUNK: delta of chunk row t - CHUNK
  const int srow = threadIdx.x & (CHUNK - 1);
  const bool is_lse = threadIdx.x < CHUNK, has_stat = 2 * CHUNK >= AS_THREADS || threadIdx.x < 2 * CHUNK;
  auto stat_load = [&](int row0) -> float {
    const int r = row0 + srow;
    if (!has_stat || r >= p.L) return is_lse ? 1e30f : 0.f;
    return is_lse ? lb[r] * LOG2E : db[r];
  };
  typename E::Pre pre;
  E::chunk_load(pre, qb, p.ld_qkv, w.li, ob, p.ld_dout, w.lo, 0, p.L);
  float sv = stat_load(0);
  E::chunk_store(pre, sm, sm + E::TILE);
  if (has_stat) stats[threadIdx.x] = sv;
  __syncthreads();
  const typename E::Lane ln = E::make_lane(lane);
  const float c2 = p.scale * LOG2E;
  f32x16 dk[E::NT], dv[E::NT];
#pragma unroll
  for (int n = 0; n < E::NT; ++n) { zero16(dk[n]); zero16(dv[n]); }
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const T* Qs = sm + (c & 1) * E::STAGE;
    const T* Os = Qs + E::TILE;
    const float* Ls = stats + (c & 1) * 2 * CHUNK;
    const float* Ds = Ls + CHUNK;
    E::chunk_load(pre, qb, p.ld_qkv, w.li, ob, p.ld_dout, w.lo, (c + 1) * CHUNK, p.L);
    sv = stat_load((c + 1) * CHUNK);
    if (w.active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
#pragma unroll
      for (int t = 0; t < QC; ++t)
        // padded query rows: Ls = +huge -> P = 0, zero Q / dO rows; padded keys only feed dk / dv rows that are never stored
        if (t < nt) E::dkv_tile(dk, dv, Qs, Os, Ls, Ds, t * 32, kf, vf, c2, ln, lane);
    }
    if (c + 1 < nch) {
      T* nx = sm + ((c + 1) & 1) * E::STAGE;
      E::chunk_store(pre, nx, nx + E::TILE);
      if (has_stat) stats[((c + 1) & 1) * 2 * CHUNK + threadIdx.x] = sv;
    }
    __syncthreads();
  }
  if (!w.active) return;
  T* stg = sm + w.wave * E::STG;
  auto base_of = [&](int r) -> T* {
    const int kk = w.row0 + r;
    if (kk >= p.L) return nullptr;
    return attn_cls_row(p, kk) ? dqkv_cls + (long)w.s * p.ld_dqkv : dqkv + lin_row(w.li, kk) * p.ld_dqkv;
  };
  E::store_rows(stg, dk, p.scale, lane, [&](int r) -> T* { T* b = base_of(r); return b ? b + D + h * E::HD : nullptr; });
  E::store_rows(stg, dv, 1.0f, lane, [&](int r) -> T* { T* b = base_of(r); return b ? b + 2 * D + h * E::HD : nullptr; });
}

// host side ---------------------------------------------------------------------------------------
template <class E> constexpr size_t stream_lds_kv() { return (size_t)2 * E::STAGE * sizeof(typename E::elem); }
template <class E> constexpr size_t stream_lds_dkv() { return stream_lds_kv<E>() + (size_t)2 * 2 * E::CHUNK * sizeof(float); }   // + lse / delta of both stages

inline dim3 stream_grid(const AttnP& p) { return dim3((unsigned)p.S * (unsigned)cdiv(p.L, AS_ROWS), p.H); }

// One launch.
template <auto Kernel, class... Args>
int stream_launch(const char* what, size_t lds, const AttnP& p, hipStream_t st, Args... args) {
  allow_lds<Kernel>(lds);
  hipLaunchKernelGGL(Kernel, stream_grid(p), dim3(AS_THREADS), lds, st, p, args...);
  return check_launch(what);
}

template <class E, auto Fwd>
int stream_fwd_launch(const char* what, const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st) {
  typedef typename E::elem T;
  return stream_launch<Fwd>(what, stream_lds_kv<E>(), p, st, (const T*)qkv, (T*)out, lse);
}

// The two kernels of a backward, each with its own policy (its chunk rows and hence its LDS).
template <class Edq, auto Dq, class Edkv, auto Dkv>
int stream_bwd_launch(const char* what_dq, const char* what_dkv, const AttnP& p, const void* qkv, const void* o, const void* dout,
                      const float* lse, float* delta, void* dqkv, void* dqkv_cls, hipStream_t st) {
  typedef typename Edq::elem T;
  const int rc = stream_launch<Dq>(what_dq, stream_lds_kv<Edq>(), p, st, (const T*)qkv, (const T*)o, (const T*)dout, lse, delta, (T*)dqkv,
                                   (T*)dqkv_cls);
  if (rc) return rc;
  return stream_launch<Dkv>(what_dkv, stream_lds_dkv<Edkv>(), p, st, (const T*)qkv, (const T*)dout, lse, (const float*)delta, (T*)dqkv,
                            (T*)dqkv_cls);
}

}  // namespace vtx
