// attn_hd_f32.hip -- exact-fp32 MFMA attention core for fp32 inputs, head_dim 32, 96 and 128, more than 32 tokens per sequence,
// all four layouts, forward and backward.  Every product runs on v_mfma_f32_32x32x2_f32: fp32 operands, an fma chain with fp32
// rounding after every step -- the arithmetic of the VALU kernels of attn.hip in another summation order.  Scores, probabilities
// and accumulators stay fp32 registers from the first product to the store: no value is ever rounded to bf16.
//
// The structure is the chunk streaming of attn_stream.h (read its header first: transposed scores, a workgroup of 4 waves owns 128
// queries -- 128 keys in the dk / dv kernel --, the other operands stream through two LDS stages, one barrier per chunk, dk / dv
// with one workgroup per key block walking all queries: fixed summation order, no atomics, no workspace) and the formulation is
// that of attn_f32.hip's F32Tiles (read its header for the operand layouts of the 32x32x2 MFMA).  attn_stream.h fixes 64 columns
// (h * 64, two accumulator tiles) and stays as it is, so that the head_dim-64 kernels compile to the same objects; the three bodies
// are restated here over HD, as attn_hd.hip restates them for bf16.
//
// What a head of HD columns is:
//   row fragment   HD / 2 floats per lane: [4 g + j] = column 8 g + 4 (lane >> 5) + j, g < HD / 8                (16 | 48 | 64)
//   score tile     HD / 2 chained MFMAs, one ds_read_b128 of a tile row feeds four                                (16 | 48 | 64)
//   result row     HD / 32 f32x16 accumulators; a 32-row tile of P or dS feeds 16 MFMAs into each                 ( 1 |  3 |  4)
//   LDS row        HD + 4 floats: 144 | 400 | 528 B = 9 | 25 | 33 sixteen-byte slots, all odd, so the 16 rows of a ds_read_b128
//                  group land on 16 different slots of the 256-byte bank row
//   store_rows     whole rows of HD floats through the wave's [32][HD + 4] staging tile
//
// Resources (chunk_of / occ_of below; the compiler's figures per instantiation and the timings behind the choices are in
// profiles/attn_hd_f32_bench.txt).  A stage is two [CHUNK][HD + 4] tiles and there are two stages:
//   head_dim 32    64-row chunks, 36 KiB; all three kernels bounded to three workgroups a CU (168 registers; they take 126 - 158).
//   head_dim 96    forward and dq: 32-row chunks, 50 KiB, two workgroups a CU (190 / 242 registers); with 64-row chunks (100 KiB,
//                  one workgroup a CU) the forward took 1.17 - 1.28 x as long.  dk / dv holds 96 accumulator registers and 96 of
//                  K and V fragments beside the S / dP tile and the chunk in flight: bounded to two workgroups a CU it spills
//                  (160 B a lane), so it is bounded to one (the 512-entry file: 255 + 112).
//   head_dim 128   forward: 32-row chunks, 66 KiB, two workgroups a CU (226 registers).  dq (128 registers of Q / dO fragments, 64
//                  of accumulators, two 16-register tiles and the chunk in flight: 256 + 116) and dk / dv (128 of accumulators,
//                  128 of fragments: 256 + 175) are bounded to one workgroup a CU: bounded to two they spill 192 and 484 B a lane.
//   A kernel that is alone on its CU streams 64-row chunks (101 KiB at 96, 132 / 133 KiB at 128): half the barriers, and nothing
//   else wants the LDS.  Measured against 32-row chunks: backward 3 - 4 % faster at 96, 4 - 7 % at 128.
// No instantiation uses scratch.
//
// Masking as in attn_stream.h: keys >= L have zero K / V rows and score -1e30 before the max; query rows >= L keep to their lane
// (operands clamped to row L - 1) and are never stored; in the dk / dv kernel padded query rows carry lse = +1e30 and zero
// Q / dO rows.  In the dq kernel a padded key's dS multiplies a zero K row and is not masked (masking would turn -0 into +0).
// FLOPs per (sequence, head): forward 4 L^2 HD, backward 10 L^2 HD (+ 4 L^2 HD recomputed scores).
#include "attn_common.h"

namespace vtx {
namespace hdf32 {

constexpr int THREADS = 256;
constexpr int ROWS = 128;                          // queries (keys in the dk / dv kernel) of one workgroup: 4 waves x 32

// rows per chunk and workgroups per CU of (head dim, kernel): see Resources above
enum Kern { FWD, DQ, DKV };
constexpr int occ_of(int hd, Kern k) { return hd == 32 ? 3 : hd == 96 ? (k == DKV ? 1 : 2) : (k == FWD ? 2 : 1); }
constexpr int chunk_of(int hd, Kern k) { return hd == 32 || occ_of(hd, k) == 1 ? 64 : 32; }    // alone on its CU: half the barriers

// what a head of HD columns is
template <int HD> struct Head {
  static_assert(HD == 32 || HD == 96 || HD == 128, "head dims of this file");
  static constexpr int LD = HD + 4;                // floats per LDS row
  static constexpr int NG = HD / 8;                // ds_read_b128 groups of a score tile (four MFMAs each)
  static constexpr int NT = HD / 32;               // accumulator tiles of a result row
  static constexpr int FR = HD / 2;                // floats of a row fragment per lane
  static constexpr int PR = HD / 4;                // 16-byte pieces of a row
  static constexpr int STG = 32 * LD;              // per-wave [32][LD] staging tile for row stores
};
// and the chunks of kernel K at that head dim
template <int HD, Kern K> struct Geo : Head<HD> {
  using Head<HD>::LD;
  using Head<HD>::PR;
  using Head<HD>::STG;
  static constexpr int CHUNK = chunk_of(HD, K);    // rows of the streamed operands per LDS stage
  static constexpr int KC = CHUNK / 32;
  static constexpr int TILE = CHUNK * LD;          // floats of one [CHUNK][LD] tile
  static constexpr int STAGE = 2 * TILE;           // two tiles per stage
  static constexpr int PER = CHUNK * PR / THREADS; // pieces of one tile per thread
  static_assert(CHUNK * PR % THREADS == 0, "whole pieces per thread");
  static_assert(4 * STG <= 2 * STAGE, "the staging tiles reuse the stages");
  static constexpr size_t LDS = (size_t)2 * STAGE * sizeof(float) + (K == DKV ? (size_t)2 * 2 * CHUNK * sizeof(float) : 0);   // dk / dv: + lse / delta of both stages
};

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

__device__ inline float* lds_base() {
  extern __shared__ __attribute__((aligned(16))) char sm_raw[];
  return reinterpret_cast<float*>(sm_raw);
}

// Rows row0 .. row0 + CHUNK - 1 of two operands of one sequence, in flight between two chunks.
template <int HD, Kern K> struct Pre { float4 a[Geo<HD, K>::PER], b[Geo<HD, K>::PER]; };

// Issue the loads of one chunk (rows >= L read as zero; a chunk wholly beyond L issues nothing).
template <int HD, Kern K>
__device__ __forceinline__ void chunk_load(Pre<HD, K>& x, const float* b0, long ld0, const RowLin& r0, const float* b1, long ld1,
                                           const RowLin& r1, int row0, int L) {
  typedef Geo<HD, K> G;
#pragma unroll
  for (int i = 0; i < G::PER; ++i) {
    const int id = threadIdx.x + i * THREADS;
    const int rr = id / G::PR, c = id - rr * G::PR;
    const int r = row0 + rr;
    x.a[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    x.b[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < L) {
      x.a[i] = *reinterpret_cast<const float4*>(b0 + lin_row(r0, r) * ld0 + c * 4);
      x.b[i] = *reinterpret_cast<const float4*>(b1 + lin_row(r1, r) * ld1 + c * 4);
    }
  }
}
template <int HD, Kern K>
__device__ __forceinline__ void chunk_store(const Pre<HD, K>& x, float* t0, float* t1) {
  typedef Geo<HD, K> G;
#pragma unroll
  for (int i = 0; i < G::PER; ++i) {
    const int id = threadIdx.x + i * THREADS;
    const int rr = id / G::PR, c = id - rr * G::PR;
    const int off = rr * G::LD + c * 4;
    *reinterpret_cast<float4*>(t0 + off) = x.a[i];
    *reinterpret_cast<float4*>(t1 + off) = x.b[i];
  }
}

// A row's HD columns, this lane's half: f[4 g + j] = column 8 g + 4 (lane >> 5) + j.
template <int HD> struct Frag { float f[Head<HD>::FR]; };

// This lane's half of row `row` (rows beyond nvalid read row nvalid - 1: finite operands for a lane that is never stored).
template <int HD>
__device__ __forceinline__ void load_frag(Frag<HD>& f, const float* base, long ld, int col0, const RowLin& rl, int row, int nvalid,
                                          int lane) {
  const int rc = row < nvalid ? row : nvalid - 1;
  const float* src = base + lin_row(rl, rc) * ld + col0 + 4 * (lane >> 5);
#pragma unroll
  for (int g = 0; g < Head<HD>::NG; ++g) {
    const float4 v = *reinterpret_cast<const float4*>(src + 8 * g);
    f.f[4 * g] = v.x; f.f[4 * g + 1] = v.y; f.f[4 * g + 2] = v.z; f.f[4 * g + 3] = v.w;
  }
}
template <int HD>
__device__ __forceinline__ float frag_dot(const Frag<HD>& a, const Frag<HD>& b) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < Head<HD>::FR; ++e) s = fmaf(a.f[e], b.f[e], s);
  return s;
}

// Per-lane LDS offsets (floats) of the two readers; the tile row (a multiple of 32) adds an immediate.
struct Lane { int rows, cols; };
template <int HD>
__device__ __forceinline__ Lane make_lane(int lane) {
  return Lane{(lane & 31) * Head<HD>::LD + 4 * (lane >> 5), 4 * (lane >> 5) * Head<HD>::LD + (lane & 31)};
}

// C[i][j] = sum_d tile[row0 + i][d] * b_j[d]: 32 tile rows against the lanes' own row fragments (HD / 2 MFMAs).
template <int HD>
__device__ __forceinline__ f32x16 scores(const float* t, int row0, const Frag<HD>& b, const Lane& ln) {
  typedef Head<HD> G;
  f32x16 acc;
  zero16(acc);
#pragma unroll
  for (int g = 0; g < G::NG; ++g) {
    const float4 a = *reinterpret_cast<const float4*>(t + ln.rows + row0 * G::LD + 8 * g);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.f[4 * g], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.f[4 * g + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.f[4 * g + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.f[4 * g + 3], acc, 0, 0, 0);
  }
  return acc;
}

// acc[n][d][j] += sum_i tile[row0 + i][32 n + d] * c[i][j] with c in the accumulator layout of scores() (16 MFMAs per tile n).
template <int HD>
__device__ __forceinline__ void accum(f32x16 (&acc)[Head<HD>::NT], const float* t, int row0, const f32x16& c, const Lane& ln) {
  typedef Head<HD> G;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float* src = t + ln.cols + (row0 + (r & 3) + 8 * (r >> 2)) * G::LD;
#pragma unroll
    for (int n = 0; n < G::NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(src[32 * n], c[r], acc[n], 0, 0, 0);
  }
}

// The dk / dv products of one 32-query tile, S -> P -> dv -> dP -> dS -> dk: S and dP are never live together.
template <int HD>
__device__ __forceinline__ void dkv_tile(f32x16 (&dk)[Head<HD>::NT], f32x16 (&dv)[Head<HD>::NT], const float* Qs, const float* Os,
                                         const float* Ls, const float* Ds, int row0, const Frag<HD>& kf, const Frag<HD>& vf, float c2,
                                         const Lane& ln, int lane) {
  f32x16 pr = scores<HD>(Qs, row0, kf, ln);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 l4 = *reinterpret_cast<const float4*>(Ls + row0 + 8 * g + 4 * (lane >> 5));
    pr[4 * g] = __builtin_amdgcn_exp2f(fmaf(pr[4 * g], c2, -l4.x));
    pr[4 * g + 1] = __builtin_amdgcn_exp2f(fmaf(pr[4 * g + 1], c2, -l4.y));
    pr[4 * g + 2] = __builtin_amdgcn_exp2f(fmaf(pr[4 * g + 2], c2, -l4.z));
    pr[4 * g + 3] = __builtin_amdgcn_exp2f(fmaf(pr[4 * g + 3], c2, -l4.w));
  }
  accum<HD>(dv, Os, row0, pr, ln);
  f32x16 ds = scores<HD>(Os, row0, vf, ln);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 d4 = *reinterpret_cast<const float4*>(Ds + row0 + 8 * g + 4 * (lane >> 5));
    ds[4 * g] = pr[4 * g] * (ds[4 * g] - d4.x);          // the softmax scale is applied once to dk at the store
    ds[4 * g + 1] = pr[4 * g + 1] * (ds[4 * g + 1] - d4.y);
    ds[4 * g + 2] = pr[4 * g + 2] * (ds[4 * g + 2] - d4.z);
    ds[4 * g + 3] = pr[4 * g + 3] * (ds[4 * g + 3] - d4.w);
  }
  accum<HD>(dk, Qs, row0, ds, ln);
}

// Store a [32 x HD] result held transposed (lane & 31 = row, registers = HD columns in NT C tiles) through a wave-private LDS
// tile, so that global memory sees whole rows: HD / 4 lanes x 16 B per row.
// ptr_of_row(r) -> destination of tile row r (HD floats), or nullptr for a padded row.
template <int HD, typename PtrFn>
__device__ __forceinline__ void store_rows(float* stg, const f32x16 (&acc)[Head<HD>::NT], float mul, int lane, PtrFn ptr_of_row) {
  typedef Head<HD> G;
#pragma unroll
  for (int n = 0; n < G::NT; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(stg + (lane & 31) * G::LD + n * 32 + 8 * g + 4 * (lane >> 5)) =
          make_float4(acc[n][4 * g] * mul, acc[n][4 * g + 1] * mul, acc[n][4 * g + 2] * mul, acc[n][4 * g + 3] * mul);
  wave_lds_sync();
#pragma unroll
  for (int i = 0; i < 32 * G::PR / 64; ++i) {
    const int id = i * 64 + lane;
    const int r = id / G::PR, c = id - r * G::PR;
    const float4 v = *reinterpret_cast<const float4*>(stg + r * G::LD + c * 4);
    float* dst = ptr_of_row(r);
    if (dst) *reinterpret_cast<float4*>(dst + c * 4) = v;
  }
  wave_lds_sync();
}

// ------------------------------------------------------------------------------------------------ forward
template <int HD>
__global__ __launch_bounds__(THREADS, occ_of(HD, FWD)) void fwd_kernel(AttnP p, const float* __restrict__ qkv, float* __restrict__ out,
                                                                       float* __restrict__ lse) {
  typedef Geo<HD, FWD> G;
  constexpr int CHUNK = G::CHUNK, KC = G::KC;
  float* sm = lds_base();
  const Who w = who<HD>(p);
  const int lane = w.lane, h = w.h;
  const float* kb = qkv + w.D + h * HD;
  const float* vb = qkv + 2 * w.D + h * HD;
  Frag<HD> qf;
  load_frag<HD>(qf, qkv, p.ld_qkv, h * HD, w.li, w.row, p.L, lane);
  Pre<HD, FWD> pre;
  chunk_load<HD, FWD>(pre, kb, p.ld_qkv, w.li, vb, p.ld_qkv, w.li, 0, p.L);
  chunk_store<HD, FWD>(pre, sm, sm + G::TILE);
  __syncthreads();
  const Lane ln = make_lane<HD>(lane);
  const float c2 = p.scale * LOG2E;
  f32x16 acc[G::NT];
#pragma unroll
  for (int n = 0; n < G::NT; ++n) zero16(acc[n]);
  float m = -1e30f, l = 0.f;                       // running max of the RAW scores (scale > 0)
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const float* Ks = sm + (c & 1) * G::STAGE;
    const float* Vs = Ks + G::TILE;
    chunk_load<HD, FWD>(pre, kb, p.ld_qkv, w.li, vb, p.ld_qkv, w.li, (c + 1) * CHUNK, p.L);
    if (w.active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
      f32x16 st[KC];                               // (tiles beyond nt stay undefined: every use below is guarded)
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) st[t] = scores<HD>(Ks, t * 32, qf, ln);
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
        if (t < nt) accum<HD>(acc, Vs, t * 32, st[t], ln);
    }
    if (c + 1 < nch) {
      float* nx = sm + ((c + 1) & 1) * G::STAGE;   // last read in iteration c - 1, behind that iteration's barrier
      chunk_store<HD, FWD>(pre, nx, nx + G::TILE);
    }
    __syncthreads();
  }
  if (!w.active) return;
  float* stg = sm + w.wave * G::STG;               // every wave is past the last chunk: the stages are free
  store_rows<HD>(stg, acc, 1.0f / l, lane, [&](int r) -> float* {
    const int qq = w.row0 + r;
    return qq < p.L ? out + lin_row(w.lo, qq) * p.ld_out + h * HD : nullptr;
  });
  if (w.row < p.L && lane < 32) lse[((long)w.s * p.H + h) * p.L + w.row] = (m * c2) * LN2 + __logf(l);
}

// ------------------------------------------------------------------------------------------------ backward: dq (+ delta)
template <int HD>
__global__ __launch_bounds__(THREADS, occ_of(HD, DQ)) void bwd_dq_kernel(AttnP p, const float* __restrict__ qkv, const float* __restrict__ o,
                                                                         const float* __restrict__ dout, const float* __restrict__ lse,
                                                                         float* __restrict__ delta, float* __restrict__ dqkv,
                                                                         float* __restrict__ dqkv_cls) {
  typedef Geo<HD, DQ> G;
  constexpr int CHUNK = G::CHUNK, KC = G::KC;
  float* sm = lds_base();
  const Who w = who<HD>(p);
  const int lane = w.lane, h = w.h;
  const float* kb = qkv + w.D + h * HD;
  const float* vb = qkv + 2 * w.D + h * HD;
  Frag<HD> qf, df;
  float dl;                                        // delta = rowsum(dO * O): this lane's half of the row's columns
  {
    Frag<HD> of;
    load_frag<HD>(qf, qkv, p.ld_qkv, h * HD, w.li, w.row, p.L, lane);
    load_frag<HD>(df, dout, p.ld_dout, h * HD, w.lo, w.row, p.L, lane);
    load_frag<HD>(of, o, p.ld_out, h * HD, w.lo, w.row, p.L, lane);
    dl = frag_dot<HD>(df, of);
  }
  dl += __shfl_xor(dl, 32, 64);
  float l2 = 0.f;
  if (w.row < p.L) {
    const long lidx = ((long)w.s * p.H + h) * p.L + w.row;
    l2 = lse[lidx] * LOG2E;
    if (lane < 32) delta[lidx] = dl;
  }
  Pre<HD, DQ> pre;
  chunk_load<HD, DQ>(pre, kb, p.ld_qkv, w.li, vb, p.ld_qkv, w.li, 0, p.L);
  chunk_store<HD, DQ>(pre, sm, sm + G::TILE);
  __syncthreads();
  const Lane ln = make_lane<HD>(lane);
  const float c2 = p.scale * LOG2E;
  f32x16 acc[G::NT];
#pragma unroll
  for (int n = 0; n < G::NT; ++n) zero16(acc[n]);
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const float* Ks = sm + (c & 1) * G::STAGE;
    const float* Vs = Ks + G::TILE;
    chunk_load<HD, DQ>(pre, kb, p.ld_qkv, w.li, vb, p.ld_qkv, w.li, (c + 1) * CHUNK, p.L);
    if (w.active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < nt) {
          const f32x16 st = scores<HD>(Ks, t * 32, qf, ln);
          f32x16 ds = scores<HD>(Vs, t * 32, df, ln);
          // dS = P (dP - delta); the softmax scale is applied once to dq at the store.  A padded key has zero K and V rows:
          // its dS is finite and multiplies zeros.
#pragma unroll
          for (int r = 0; r < 16; ++r) ds[r] = __builtin_amdgcn_exp2f(fmaf(st[r], c2, -l2)) * (ds[r] - dl);
          accum<HD>(acc, Ks, t * 32, ds, ln);
        }
    }
    if (c + 1 < nch) {
      float* nx = sm + ((c + 1) & 1) * G::STAGE;
      chunk_store<HD, DQ>(pre, nx, nx + G::TILE);
    }
    __syncthreads();
  }
  if (!w.active) return;
  float* stg = sm + w.wave * G::STG;
  store_rows<HD>(stg, acc, p.scale, lane, [&](int r) -> float* {
    const int qq = w.row0 + r;
    if (qq >= p.L) return nullptr;
    return attn_cls_row(p, qq) ? dqkv_cls + (long)w.s * p.ld_dqkv + h * HD : dqkv + lin_row(w.li, qq) * p.ld_dqkv + h * HD;
  });
}

// ------------------------------------------------------------------------------------------------ backward: dk, dv
// Lanes = keys: wave w of the workgroup of key block kb owns the key tile kb * 4 + w and walks ALL queries of the sequence.
template <int HD>
__global__ __launch_bounds__(THREADS, occ_of(HD, DKV)) void bwd_dkv_kernel(AttnP p, const float* __restrict__ qkv,
                                                                           const float* __restrict__ dout, const float* __restrict__ lse,
                                                                           const float* __restrict__ delta, float* __restrict__ dqkv,
                                                                           float* __restrict__ dqkv_cls) {
  typedef Geo<HD, DKV> G;
  constexpr int CHUNK = G::CHUNK, QC = G::KC;
  float* sm = lds_base();
  float* stats = sm + 2 * G::STAGE;                // [stage][lse * log2(e) | delta][CHUNK]
  const Who w = who<HD>(p);
  const int lane = w.lane, h = w.h, D = w.D;
  const float* qb = qkv + h * HD;
  const float* ob = dout + h * HD;
  const float* lb = lse + ((long)w.s * p.H + h) * p.L;
  const float* db = delta + ((long)w.s * p.H + h) * p.L;
  Frag<HD> kf, vf;
  load_frag<HD>(kf, qkv, p.ld_qkv, D + h * HD, w.li, w.row, p.L, lane);
  load_frag<HD>(vf, qkv, p.ld_qkv, 2 * D + h * HD, w.li, w.row, p.L, lane);
  // thread t < CHUNK: lse of chunk row t (scaled; +huge on padded rows -> P = 0); CHUNK <= t < 2 CHUNK: delta of chunk row t - CHUNK
  const int srow = threadIdx.x & (CHUNK - 1);
  const bool is_lse = threadIdx.x < CHUNK, has_stat = threadIdx.x < 2 * CHUNK;
  auto stat_load = [&](int row0) -> float {
    const int r = row0 + srow;
    if (!has_stat || r >= p.L) return is_lse ? 1e30f : 0.f;
    return is_lse ? lb[r] * LOG2E : db[r];
  };
  Pre<HD, DKV> pre;
  chunk_load<HD, DKV>(pre, qb, p.ld_qkv, w.li, ob, p.ld_dout, w.lo, 0, p.L);
  float sv = stat_load(0);
  chunk_store<HD, DKV>(pre, sm, sm + G::TILE);
  if (has_stat) stats[threadIdx.x] = sv;
  __syncthreads();
  const Lane ln = make_lane<HD>(lane);
  const float c2 = p.scale * LOG2E;
  f32x16 dk[G::NT], dv[G::NT];
#pragma unroll
  for (int n = 0; n < G::NT; ++n) { zero16(dk[n]); zero16(dv[n]); }
  const int nch = (p.L + CHUNK - 1) / CHUNK;
  for (int c = 0; c < nch; ++c) {
    const float* Qs = sm + (c & 1) * G::STAGE;
    const float* Os = Qs + G::TILE;
    const float* Ls = stats + (c & 1) * 2 * CHUNK;
    const float* Ds = Ls + CHUNK;
    chunk_load<HD, DKV>(pre, qb, p.ld_qkv, w.li, ob, p.ld_dout, w.lo, (c + 1) * CHUNK, p.L);
    sv = stat_load((c + 1) * CHUNK);
    if (w.active) {
      const int nrows = min(CHUNK, p.L - c * CHUNK);
      const int nt = (nrows + 31) >> 5;
#pragma unroll
      for (int t = 0; t < QC; ++t)
        // padded query rows: Ls = +huge -> P = 0, zero Q / dO rows; padded keys only feed dk / dv rows that are never stored
        if (t < nt) dkv_tile<HD>(dk, dv, Qs, Os, Ls, Ds, t * 32, kf, vf, c2, ln, lane);
    }
    if (c + 1 < nch) {
      float* nx = sm + ((c + 1) & 1) * G::STAGE;
      chunk_store<HD, DKV>(pre, nx, nx + G::TILE);
      if (has_stat) stats[((c + 1) & 1) * 2 * CHUNK + threadIdx.x] = sv;
    }
    __syncthreads();
  }
  if (!w.active) return;
  float* stg = sm + w.wave * G::STG;
  auto base_of = [&](int r) -> float* {
    const int kk = w.row0 + r;
    if (kk >= p.L) return nullptr;
    return attn_cls_row(p, kk) ? dqkv_cls + (long)w.s * p.ld_dqkv : dqkv + lin_row(w.li, kk) * p.ld_dqkv;
  };
  store_rows<HD>(stg, dk, p.scale, lane, [&](int r) -> float* { float* b = base_of(r); return b ? b + D + h * HD : nullptr; });
  store_rows<HD>(stg, dv, 1.0f, lane, [&](int r) -> float* { float* b = base_of(r); return b ? b + 2 * D + h * HD : nullptr; });
}

// host side ---------------------------------------------------------------------------------------
static dim3 grid_of(const AttnP& p) { return dim3((unsigned)p.S * (unsigned)cdiv(p.L, ROWS), p.H); }

template <int HD>
static int fwd_launch(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st) {
  constexpr size_t lds = Geo<HD, FWD>::LDS;
  allow_lds<fwd_kernel<HD>>(lds);
  hipLaunchKernelGGL(fwd_kernel<HD>, grid_of(p), dim3(THREADS), lds, st, p, (const float*)qkv, (float*)out, lse);
  return check_launch("attn_fwd_hd_f32");
}
template <int HD>
static int bwd_launch(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                      void* dqkv_cls, hipStream_t st) {
  constexpr size_t lds_dq = Geo<HD, DQ>::LDS, lds_dkv = Geo<HD, DKV>::LDS;
  allow_lds<bwd_dq_kernel<HD>>(lds_dq);
  hipLaunchKernelGGL(bwd_dq_kernel<HD>, grid_of(p), dim3(THREADS), lds_dq, st, p, (const float*)qkv, (const float*)o,
                     (const float*)dout, lse, delta, (float*)dqkv, (float*)dqkv_cls);
  const int rc = check_launch("attn_bwd_dq_hd_f32");
  if (rc) return rc;
  allow_lds<bwd_dkv_kernel<HD>>(lds_dkv);
  hipLaunchKernelGGL(bwd_dkv_kernel<HD>, grid_of(p), dim3(THREADS), lds_dkv, st, p, (const float*)qkv, (const float*)dout, lse,
                     (const float*)delta, (float*)dqkv, (float*)dqkv_cls);
  return check_launch("attn_bwd_dkv_hd_f32");
}

}  // namespace hdf32

bool attn_hd_f32_eligible(int dtype, int L, int hd) { return dtype == VTX_F32 && (hd == 32 || hd == 96 || hd == 128) && L > 32; }

int attn_fwd_hd_f32_launch(const AttnP& p, int hd, const void* qkv, void* out, float* lse, hipStream_t st) {
  switch (hd) {
    case 32: return hdf32::fwd_launch<32>(p, qkv, out, lse, st);
    case 96: return hdf32::fwd_launch<96>(p, qkv, out, lse, st);
    case 128: return hdf32::fwd_launch<128>(p, qkv, out, lse, st);
  }
  VTX_REQUIRE(false, VTX_EINVAL, "attn_fwd_hd_f32: head_dim %d", hd);
}

int attn_bwd_hd_f32_launch(const AttnP& p, int hd, const void* qkv, const void* o, const void* dout, const float* lse, float* delta,
                           void* dqkv, void* dqkv_cls, hipStream_t st) {
  switch (hd) {
    case 32: return hdf32::bwd_launch<32>(p, qkv, o, dout, lse, delta, dqkv, dqkv_cls, st);
    case 96: return hdf32::bwd_launch<96>(p, qkv, o, dout, lse, delta, dqkv, dqkv_cls, st);
    case 128: return hdf32::bwd_launch<128>(p, qkv, o, dout, lse, delta, dqkv, dqkv_cls, st);
  }
  VTX_REQUIRE(false, VTX_EINVAL, "attn_bwd_hd_f32: head_dim %d", hd);
}

}  // namespace vtx
