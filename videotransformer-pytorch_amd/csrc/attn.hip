// attn.hip -- softmax(q k^T * scale) v per (sequence, head): forward, materialised
// probabilities, and backward.  fp32-exact VALU formulation (one thread per
// query row, keys/values staged through LDS in tiles, chunked online softmax).
//
// Reference: Attention.forward transformer.py:165-177 and the regrouping around
// it: '(b p) t d' :250 (temporal, contiguous T-token sequences), '(b t) p d' +
// per-frame cls replication :352-356 and the scatter back :375 (spatial).  The
// regrouping is done here by row arithmetic (in_row/out_row); no tensor is
// rearranged in memory.
//
// Small sequences (temporal attention, L = T = 8) pack G = 256/L sequences per
// workgroup; long ones use one sequence per workgroup and 64-key tiles.  bf16 with
// head_dim 64 never gets here by default: up to 32 tokens run the packed kernels of attn_hd.hip,
// 33..256 (L = 197 spatial) the MFMA kernels of attn_mfma.hip, more than 256 (785 spatial at 448^2, 1569
// joint) those of attn_long.hip; fp32 with head_dim 64 and more than 32 tokens runs the exact-fp32 MFMA kernels of
// attn_f32.hip.  These kernels are the fp32 path of up to 32 tokens, the `probs` pass (and the forward in front of it)
// and what attn_valu=1 / attn_long=0 / attn_f32=valu select.  At head_dim 32, 96 and 128 the same holds: bf16 runs the MFMA
// kernels of attn_hd.hip (attn_hd=valu sends it back here), fp32 above 32 tokens the exact-fp32 MFMA kernels of attn_hd_f32.hip
// (attn_f32=valu), and what stays here is fp32 of up to 32 tokens, bf16 SPACE / SPACE_NOCLS of up to 32 tokens and the `probs`
// pass.  Algorithmic bytes per (sequence, head):
// read 3*L*hd, write L*hd elements (+ L fp32 lse).
#include <stdlib.h>
#include "attn_common.h"

namespace vtx {

constexpr int AT_THREADS = 256;    // long sequences: one sequence per workgroup
constexpr int AT_PACK_THREADS = 128;  // short sequences: G = 128/L sequences per workgroup (64 KB of LDS tiles)
constexpr int AT_KT = 64;      // keys (or queries, in the dk/dv pass) per LDS tile
constexpr int AT_CH = 8;       // online-softmax chunk

template <int HD> struct Tile {           // one [rows][HD] fp32 tile per packed sequence, padded
  static constexpr int SEQ_PAD = 4;       // floats between packed sequences (bank spread for broadcast reads)
};

// Cooperative load of `n` rows x HD elements (type T, global) into fp32 LDS rows.
// 8 (bf16) or 16 (fp32) threads per row; rows addressed through rowfn(r).
template <typename T, int HD, typename RowFn>
__device__ inline void load_rows(float* lds, int lds_ld, int n, const T* base, long ld, int col0, RowFn rowfn) {
  constexpr int CH = HD / 8;              // 8-element chunks per row
  for (int id = threadIdx.x; id < n * CH; id += blockDim.x) {
    const int r = id / CH, c = id - r * CH;
    float v[8];
    load8(base + rowfn(r) * ld + col0 + c * 8, v);
    float* d = lds + r * lds_ld + c * 8;
    *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
}

template <int HD> __device__ inline float dot_lds(const float (&q)[HD], const float* k) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int e = 0; e < HD; e += 4) {
    const float4 kv = *reinterpret_cast<const float4*>(k + e);
    s0 += q[e] * kv.x; s1 += q[e + 1] * kv.y; s2 += q[e + 2] * kv.z; s3 += q[e + 3] * kv.w;
  }
  return (s0 + s1) + (s2 + s3);
}
template <int HD> __device__ inline void axpy_lds(float (&acc)[HD], float a, const float* v) {
#pragma unroll
  for (int e = 0; e < HD; e += 4) {
    const float4 x = *reinterpret_cast<const float4*>(v + e);
    acc[e] += a * x.x; acc[e + 1] += a * x.y; acc[e + 2] += a * x.z; acc[e + 3] += a * x.w;
  }
}
template <typename T, int HD> __device__ inline void load_vec(const T* p, float (&v)[HD]) {
#pragma unroll
  for (int c = 0; c < HD / 8; ++c) {
    float t8[8];
    load8(p + c * 8, t8);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[c * 8 + j] = t8[j];
  }
}
template <typename T, int HD> __device__ inline void store_vec(T* p, const float (&v)[HD]) {
#pragma unroll
  for (int c = 0; c < HD / 8; ++c) {
    float t8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t8[j] = v[c * 8 + j];
    store8(p + c * 8, t8);
  }
}

// Work decomposition shared by all passes: blockIdx.x -> (sequence group, row block), blockIdx.y -> head.
// Thread -> (g, i): packed sequence g of the group and row i (query or key) of that sequence.
struct Who { int s0, g, i, nseq, rows_blk; bool active; };
__device__ inline Who who_am_i(const AttnP& p) {
  Who w;
  if (p.G > 1) {
    w.s0 = blockIdx.x * p.G;
    w.nseq = min(p.G, p.S - w.s0);
    w.g = threadIdx.x / p.L; w.i = threadIdx.x - w.g * p.L;
    w.active = w.g < w.nseq;
    w.rows_blk = 0;
  } else {
    const int nblk = (p.L + blockDim.x - 1) / blockDim.x;
    w.s0 = blockIdx.x / nblk; w.nseq = 1; w.g = 0;
    w.rows_blk = (blockIdx.x - w.s0 * nblk) * blockDim.x;
    w.i = w.rows_blk + threadIdx.x;
    w.active = w.i < p.L;
  }
  return w;
}

// PASS 0: forward (out, lse).  PASS 1: probabilities from a saved lse.
template <typename T, int HD, int PASS>
__global__ __launch_bounds__(AT_THREADS) void attn_fwd_kernel(AttnP p, const T* __restrict__ qkv, T* __restrict__ out,
                                                              float* __restrict__ lse, float* __restrict__ probs) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int h = blockIdx.y, D = p.H * HD;
  const Who w = who_am_i(p);
  const int KT = p.G > 1 ? p.L : AT_KT;
  const int seq_ld = KT * HD + Tile<HD>::SEQ_PAD;
  float* Ks = sm;
  float* Vs = sm + p.G * seq_ld;
  const int s = w.s0 + w.g;

  float q[HD];
  if (w.active) {
    load_vec<T, HD>(qkv + in_row(p, s, w.i) * p.ld_qkv + h * HD, q);
#pragma unroll
    for (int e = 0; e < HD; ++e) q[e] *= p.scale;
  }
  float acc[HD];
#pragma unroll
  for (int e = 0; e < HD; ++e) acc[e] = 0.f;
  float m = -INFINITY, l = 0.f;
  float my_lse = 0.f;
  if (PASS == 1 && w.active) my_lse = lse[((long)s * p.H + h) * p.L + w.i];

  for (int k0 = 0; k0 < p.L; k0 += KT) {
    const int nk = min(KT, p.L - k0);
    __syncthreads();
    for (int g = 0; g < w.nseq; ++g) {
      const int sg = w.s0 + g;
      load_rows<T, HD>(Ks + g * seq_ld, HD, nk, qkv, p.ld_qkv, D + h * HD, [&](int r) { return in_row(p, sg, k0 + r); });
      if (PASS == 0)
        load_rows<T, HD>(Vs + g * seq_ld, HD, nk, qkv, p.ld_qkv, 2 * D + h * HD, [&](int r) { return in_row(p, sg, k0 + r); });
    }
    __syncthreads();
    if (!w.active) continue;
    const float* Kg = Ks + w.g * seq_ld;
    const float* Vg = Vs + w.g * seq_ld;
    if (PASS == 1) {
      float* pr = probs + (((long)s * p.H + h) * p.L + w.i) * p.L + k0;
      for (int j = 0; j < nk; ++j) pr[j] = __expf(dot_lds<HD>(q, Kg + j * HD) - my_lse);
      continue;
    }
    for (int j0 = 0; j0 < nk; j0 += AT_CH) {
      float sc[AT_CH];
      float cmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < AT_CH; ++j) {
        if (j0 + j < nk) { sc[j] = dot_lds<HD>(q, Kg + (j0 + j) * HD); cmax = fmaxf(cmax, sc[j]); }
        else sc[j] = -INFINITY;
      }
      const float mn = fmaxf(m, cmax);
      const float alpha = __expf(m - mn);      // m = -inf on the first chunk -> 0
      l *= alpha;
#pragma unroll
      for (int e = 0; e < HD; ++e) acc[e] *= alpha;
      m = mn;
#pragma unroll
      for (int j = 0; j < AT_CH; ++j) {
        if (j0 + j < nk) {
          const float pj = __expf(sc[j] - m);
          l += pj;
          axpy_lds<HD>(acc, pj, Vg + (j0 + j) * HD);
        }
      }
    }
  }
  if (PASS == 0 && w.active) {
    const float inv = 1.0f / l;
#pragma unroll
    for (int e = 0; e < HD; ++e) acc[e] *= inv;
    store_vec<T, HD>(out + out_row(p, s, w.i) * p.ld_out + h * HD, acc);
    lse[((long)s * p.H + h) * p.L + w.i] = m + __logf(l);
  }
}

// Backward pass A: thread per query.  dq_i = scale * sum_j p_ij (dO_i.v_j - delta_i) k_j; also writes delta.
// NP > 1 (head_dim 96 and 128): blockIdx.z picks one of NP column parts of dq, so that a thread accumulates HD / NP columns
// (q, dO and all of dq are 3 HD floats a thread: more than the 256 vector registers from HD = 96 on); the parts repeat the scores.  The one-part form of <bf16, 96> spilled to scratch
// and returned wrong dq on the device, for a reason that was not found (profiles/attn_hd_bench.txt, 1); NP = 1 is the kernel as it was.
template <typename T, int HD, int NP>
__global__ __launch_bounds__(AT_THREADS) void attn_bwd_dq_kernel(AttnP p, const T* __restrict__ qkv, const T* __restrict__ o,
                                                                 const T* __restrict__ dout, const float* __restrict__ lse,
                                                                 float* __restrict__ delta, T* __restrict__ dqkv,
                                                                 T* __restrict__ dqkv_cls) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int HP = HD / NP;
  const int h = blockIdx.y, D = p.H * HD, part = NP > 1 ? blockIdx.z : 0;
  const Who w = who_am_i(p);
  const int KT = p.G > 1 ? p.L : AT_KT;
  const int seq_ld = KT * HD + Tile<HD>::SEQ_PAD;
  float* Ks = sm;
  float* Vs = sm + p.G * seq_ld;
  const int s = w.s0 + w.g;

  float q[HD], dO[HD], dq[HP];
  float my_lse = 0.f, my_delta = 0.f;
#pragma unroll
  for (int e = 0; e < HP; ++e) dq[e] = 0.f;
  if (w.active) {
    load_vec<T, HD>(qkv + in_row(p, s, w.i) * p.ld_qkv + h * HD, q);
    const long orow = out_row(p, s, w.i);
    load_vec<T, HD>(dout + orow * p.ld_dout + h * HD, dO);
    {
      float ov[HD];
      load_vec<T, HD>(o + orow * p.ld_out + h * HD, ov);
#pragma unroll
      for (int e = 0; e < HD; ++e) my_delta += ov[e] * dO[e];
    }
#pragma unroll
    for (int e = 0; e < HD; ++e) q[e] *= p.scale;
    const long li = ((long)s * p.H + h) * p.L + w.i;
    my_lse = lse[li];
    if (part == 0) delta[li] = my_delta;
  }
  for (int k0 = 0; k0 < p.L; k0 += KT) {
    const int nk = min(KT, p.L - k0);
    __syncthreads();
    for (int g = 0; g < w.nseq; ++g) {
      const int sg = w.s0 + g;
      load_rows<T, HD>(Ks + g * seq_ld, HD, nk, qkv, p.ld_qkv, D + h * HD, [&](int r) { return in_row(p, sg, k0 + r); });
      load_rows<T, HD>(Vs + g * seq_ld, HD, nk, qkv, p.ld_qkv, 2 * D + h * HD, [&](int r) { return in_row(p, sg, k0 + r); });
    }
    __syncthreads();
    if (!w.active) continue;
    const float* Kg = Ks + w.g * seq_ld;
    const float* Vg = Vs + w.g * seq_ld;
    for (int j = 0; j < nk; ++j) {
      const float pij = __expf(dot_lds<HD>(q, Kg + j * HD) - my_lse);
      const float dp = dot_lds<HD>(dO, Vg + j * HD);
      axpy_lds<HP>(dq, pij * (dp - my_delta), Kg + j * HD + part * HP);
    }
  }
  if (w.active) {
#pragma unroll
    for (int e = 0; e < HP; ++e) dq[e] *= p.scale;
    T* dst = attn_cls_row(p, w.i) ? dqkv_cls + (long)s * p.ld_dqkv + h * HD
                                                    : dqkv + in_row(p, s, w.i) * p.ld_dqkv + h * HD;
    store_vec<T, HP>(dst + part * HP, dq);
  }
}

// Backward pass B: thread per key.  dv_j = sum_i p_ij dO_i;  dk_j = scale * sum_i p_ij (dO_i.v_j - delta_i) q_i.
template <typename T, int HD>
__global__ __launch_bounds__(AT_THREADS, 1) void attn_bwd_dkv_kernel(AttnP p, const T* __restrict__ qkv,
                                                                     const T* __restrict__ dout, const float* __restrict__ lse,
                                                                     const float* __restrict__ delta, T* __restrict__ dqkv,
                                                                     T* __restrict__ dqkv_cls) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int h = blockIdx.y, D = p.H * HD;
  const Who w = who_am_i(p);
  const int QT = p.G > 1 ? p.L : AT_KT;
  const int seq_ld = QT * HD + Tile<HD>::SEQ_PAD;
  float* Qs = sm;
  float* Os = sm + p.G * seq_ld;
  float* Ls = Os + p.G * seq_ld;            // [G][QT] lse
  float* Ds = Ls + p.G * QT;                // [G][QT] delta
  const int s = w.s0 + w.g;

  float k[HD], v[HD], dk[HD], dv[HD];
#pragma unroll
  for (int e = 0; e < HD; ++e) { dk[e] = 0.f; dv[e] = 0.f; }
  if (w.active) {
    const long r = in_row(p, s, w.i);
    load_vec<T, HD>(qkv + r * p.ld_qkv + D + h * HD, k);
    load_vec<T, HD>(qkv + r * p.ld_qkv + 2 * D + h * HD, v);
#pragma unroll
    for (int e = 0; e < HD; ++e) k[e] *= p.scale;      // s_ij = q_i . (scale k_j)
  }
  for (int q0 = 0; q0 < p.L; q0 += QT) {
    const int nq = min(QT, p.L - q0);
    __syncthreads();
    for (int g = 0; g < w.nseq; ++g) {
      const int sg = w.s0 + g;
      load_rows<T, HD>(Qs + g * seq_ld, HD, nq, qkv, p.ld_qkv, h * HD, [&](int r) { return in_row(p, sg, q0 + r); });
      load_rows<T, HD>(Os + g * seq_ld, HD, nq, dout, p.ld_dout, h * HD, [&](int r) { return out_row(p, sg, q0 + r); });
      for (int r = threadIdx.x; r < nq; r += blockDim.x) {
        const long li = ((long)sg * p.H + h) * p.L + q0 + r;
        Ls[g * QT + r] = lse[li];
        Ds[g * QT + r] = delta[li];
      }
    }
    __syncthreads();
    if (!w.active) continue;
    const float* Qg = Qs + w.g * seq_ld;
    const float* Og = Os + w.g * seq_ld;
    for (int i = 0; i < nq; ++i) {
      const float pij = __expf(dot_lds<HD>(k, Qg + i * HD) - Ls[w.g * QT + i]);
      const float dp = dot_lds<HD>(v, Og + i * HD);
      axpy_lds<HD>(dv, pij, Og + i * HD);
      axpy_lds<HD>(dk, pij * (dp - Ds[w.g * QT + i]), Qg + i * HD);
    }
  }
  if (w.active) {
#pragma unroll
    for (int e = 0; e < HD; ++e) dk[e] *= p.scale;
    T* base = attn_cls_row(p, w.i) ? dqkv_cls + (long)s * p.ld_dqkv
                                                     : dqkv + in_row(p, s, w.i) * p.ld_dqkv;
    store_vec<T, HD>(base + D + h * HD, dk);
    store_vec<T, HD>(base + 2 * D + h * HD, dv);
  }
}

// Which kernel family serves (dtype, mode, L, head_dim).  The whole precedence is here; the first match wins.  The mode matters
// up to 32 tokens only: CONTIG and TIME_CLS are packed, SPACE_NOCLS runs the one-workgroup kernels at one tile, SPACE (no model
// has P < 32) the VALU kernels as before.
enum Route { SMALL, MFMA, LONG, F32, F32HD, VALU, HDIM };
static Route attn_route(int dtype, int mode, int L, int hd, bool probs) {
  // VTX_ATTN_VALU=1 forces the VALU path.
  if (options().attn_valu) return VALU;
  // bf16, up to 32 tokens, CONTIG or TIME_CLS, every head dim -> packed MFMA kernels (attn_hd.hip); at head_dim 32 / 96 / 128
  // VTX_ATTN_HD=valu sends them to the VALU kernels.  Everything else of up to 32 tokens at those head dims (fp32; SPACE and
  // SPACE_NOCLS, which no model reaches) has no other kernel.
  if ((hd == 64 || options().attn_hd) && attn_small_eligible(dtype, mode, L, hd)) return SMALL;
  // bf16, head_dim 64, 33..256 tokens (SPACE_NOCLS: 1..256) -> MFMA kernels (attn_mfma.hip).
  if (attn_mfma_eligible(dtype, mode, L, hd)) return MFMA;
  // bf16, head_dim 64, more than 256 tokens -> chunk-streaming MFMA kernels (attn_long.hip); VTX_ATTN_LONG=0 sends them back here.
  if (options().attn_long && attn_long_eligible(dtype, L, hd)) return LONG;
  // fp32, head_dim 64, more than 32 tokens -> exact-fp32 MFMA kernels (attn_f32.hip); VTX_ATTN_F32=valu sends them back here, and
  // so does a `probs` request: the probabilities are then recomputed from the lse of the kernel they always followed.
  if (options().attn_f32 && !probs && attn_f32_eligible(dtype, L, hd)) return F32;
  // fp32, head_dim 32 / 96 / 128, more than 32 tokens -> exact-fp32 MFMA kernels (attn_hd_f32.hip), under the same switch and with
  // the same `probs` rule.
  if (options().attn_f32 && !probs && attn_hd_f32_eligible(dtype, L, hd)) return F32HD;
  // bf16, head_dim 32 / 96 / 128, more than 32 tokens -> chunk-streaming MFMA kernels (attn_hd.hip); VTX_ATTN_HD=valu sends them
  // back here.
  if (options().attn_hd && attn_hd_eligible(dtype, L, hd)) return HDIM;
  return VALU;
}

static int make_params(const vtx_attn_desc* d, AttnP& p, const char* who) {
  VTX_REQUIRE(d->S > 0 && d->L > 0 && d->H > 0, VTX_EINVAL, "%s: bad shape S=%d L=%d H=%d", who, d->S, d->L, d->H);
  VTX_REQUIRE(d->hd == 32 || d->hd == 64 || d->hd == 96 || d->hd == 128, VTX_EINVAL, "%s: head_dim %d unsupported (32, 64, 96, 128)", who,
              d->hd);
  VTX_REQUIRE(d->mode == VTX_ATTN_CONTIG || d->mode == VTX_ATTN_SPACE || d->mode == VTX_ATTN_TIME_CLS ||
                  d->mode == VTX_ATTN_SPACE_NOCLS,
              VTX_EINVAL, "%s: bad mode", who);
  VTX_REQUIRE(d->dtype == VTX_F32 || d->dtype == VTX_BF16, VTX_EINVAL, "%s: bad dtype", who);
  const bool btp = d->B > 0 && d->T > 0 && d->P > 0;
  if (d->mode == VTX_ATTN_SPACE)
    VTX_REQUIRE(btp && d->S == d->B * d->T && d->L == d->P + 1, VTX_EINVAL, "%s: SPACE mode needs S == B*T and L == P+1", who);
  if (d->mode == VTX_ATTN_TIME_CLS)
    VTX_REQUIRE(btp && d->S == d->B * d->P && d->L == d->T + 1, VTX_EINVAL, "%s: TIME_CLS mode needs S == B*P and L == T+1", who);
  if (d->mode == VTX_ATTN_SPACE_NOCLS)
    VTX_REQUIRE(btp && d->S == d->B * d->T && d->L == d->P, VTX_EINVAL, "%s: SPACE_NOCLS mode needs S == B*T and L == P", who);
  const long vec = d->dtype == VTX_BF16 ? 8 : 4;
  VTX_REQUIRE(d->qkv && aligned16(d->qkv) && d->ld_qkv % vec == 0, VTX_EALIGN, "%s: qkv alignment", who);
  p.mode = d->mode; p.S = d->S; p.L = d->L; p.H = d->H; p.B = d->B; p.T = d->T; p.P = d->P;
  p.ld_qkv = d->ld_qkv; p.ld_out = d->ld_out; p.ld_dout = 0; p.ld_dqkv = 0; p.scale = d->scale;
  p.G = d->L <= AT_KT ? AT_PACK_THREADS / d->L : 1;
  return VTX_OK;
}
static dim3 attn_grid(const AttnP& p) {
  if (p.G > 1) return dim3(cdiv(p.S, p.G), p.H);
  return dim3(p.S * cdiv(p.L, AT_THREADS), p.H);
}
static dim3 attn_block(const AttnP& p) { return dim3(p.G > 1 ? AT_PACK_THREADS : AT_THREADS); }
static size_t attn_lds(const AttnP& p, int hd, bool with_stats) {
  const int KT = p.G > 1 ? p.L : AT_KT;
  size_t b = (size_t)2 * p.G * (KT * hd + 4) * sizeof(float);
  if (with_stats) b += (size_t)2 * p.G * KT * sizeof(float);
  return b;
}

// The VALU launches, once per element type and head dim.  PROBS = 1 recomputes the probabilities from the lse that a forward left.
// At head_dim 128 the tiles pass 64 KB (one sequence: 2 (64 * 128 + 4) * 4 B = 65568; packed, G * L <= 128: 132160 B at L = 64 and up
// to 136192 B at L = 1, where the pad of 4 floats counts G = 128 times, with the lse / delta rows of the dk / dv pass), hence the
// opt-in; 160 KB is the CU's.
template <typename T, int HD, int PROBS>
static int valu_fwd_launch_hd(const AttnP& p, const vtx_attn_desc* d, hipStream_t st) {
  const size_t lds = attn_lds(p, HD, false);
  allow_lds<attn_fwd_kernel<T, HD, PROBS>>(lds);
  hipLaunchKernelGGL((attn_fwd_kernel<T, HD, PROBS>), attn_grid(p), attn_block(p), lds, st, p, (const T*)d->qkv,
                     (T*)d->out, d->lse, PROBS ? d->probs : nullptr);
  return check_launch(PROBS ? "attn_probs" : "attn_fwd");
}
template <typename T, int PROBS>
static int valu_fwd_launch(const AttnP& p, const vtx_attn_desc* d, hipStream_t st) {
  switch (d->hd) {                                   // make_params admits no other
    case 32: return valu_fwd_launch_hd<T, 32, PROBS>(p, d, st);
    case 96: return valu_fwd_launch_hd<T, 96, PROBS>(p, d, st);
    case 128: return valu_fwd_launch_hd<T, 128, PROBS>(p, d, st);
    default: return valu_fwd_launch_hd<T, 64, PROBS>(p, d, st);
  }
}
template <typename T, int HD>
static int valu_bwd_launch_hd(const AttnP& p, const vtx_attn_bwd_desc* d, hipStream_t st) {
  const dim3 grid = attn_grid(p), block = attn_block(p);
  const size_t lds = attn_lds(p, HD, false), lds_dkv = attn_lds(p, HD, true);
  constexpr int NP = HD > 64 ? 2 : 1;                // column parts of dq (attn_bwd_dq_kernel)
  allow_lds<attn_bwd_dq_kernel<T, HD, NP>>(lds);
  hipLaunchKernelGGL((attn_bwd_dq_kernel<T, HD, NP>), dim3(grid.x, grid.y, NP), block, lds, st, p, (const T*)d->f.qkv, (const T*)d->f.out,
                     (const T*)d->dout, d->f.lse, d->delta, (T*)d->dqkv, (T*)d->dqkv_cls);
  const int rc = check_launch("attn_bwd_dq");
  if (rc) return rc;
  allow_lds<attn_bwd_dkv_kernel<T, HD>>(lds_dkv);
  hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, HD>), grid, block, lds_dkv, st, p, (const T*)d->f.qkv, (const T*)d->dout,
                     d->f.lse, d->delta, (T*)d->dqkv, (T*)d->dqkv_cls);
  return check_launch("attn_bwd_dkv");
}
template <typename T>
static int valu_bwd_launch(const AttnP& p, const vtx_attn_bwd_desc* d, hipStream_t st) {
  switch (d->f.hd) {
    case 32: return valu_bwd_launch_hd<T, 32>(p, d, st);
    case 96: return valu_bwd_launch_hd<T, 96>(p, d, st);
    case 128: return valu_bwd_launch_hd<T, 128>(p, d, st);
    default: return valu_bwd_launch_hd<T, 64>(p, d, st);
  }
}

}  // namespace vtx

using namespace vtx;

extern "C" int vtx_attn_fwd(const vtx_attn_desc* d, void* stream) {
  VTX_REQUIRE(d != nullptr, VTX_EINVAL, "attn_fwd: null descriptor");
  AttnP p;
  int rc = make_params(d, p, "attn_fwd");
  if (rc) return rc;
  VTX_REQUIRE(d->out && d->lse && aligned16(d->out), VTX_EINVAL, "attn_fwd: out/lse required");
  hipStream_t st = as_stream(stream);
  const bool f32 = d->dtype == VTX_F32;
  switch (attn_route(d->dtype, d->mode, d->L, d->hd, d->probs != nullptr)) {
    case SMALL: rc = attn_fwd_small_launch(p, d->hd, d->qkv, d->out, d->lse, st); break;
    case MFMA: rc = attn_fwd_mfma_launch(p, d->qkv, d->out, d->lse, st); break;
    case LONG: rc = attn_fwd_long_launch(p, d->qkv, d->out, d->lse, st); break;
    case F32: rc = attn_fwd_f32_launch(p, d->qkv, d->out, d->lse, st); break;
    case F32HD: rc = attn_fwd_hd_f32_launch(p, d->hd, d->qkv, d->out, d->lse, st); break;
    case HDIM: rc = attn_fwd_hd_launch(p, d->hd, d->qkv, d->out, d->lse, st); break;
    case VALU: rc = f32 ? valu_fwd_launch<float, 0>(p, d, st) : valu_fwd_launch<bf16raw, 0>(p, d, st); break;
  }
  if (rc || !d->probs) return rc;
  return f32 ? valu_fwd_launch<float, 1>(p, d, st) : valu_fwd_launch<bf16raw, 1>(p, d, st);
}

extern "C" int vtx_attn_bwd(const vtx_attn_bwd_desc* d, void* stream) {
  VTX_REQUIRE(d != nullptr, VTX_EINVAL, "attn_bwd: null descriptor");
  AttnP p;
  int rc = make_params(&d->f, p, "attn_bwd");
  if (rc) return rc;
  VTX_REQUIRE(d->f.out && d->f.lse && d->dout && d->dqkv && d->delta, VTX_EINVAL, "attn_bwd: null pointer");
  VTX_REQUIRE(d->f.mode != VTX_ATTN_SPACE || d->dqkv_cls, VTX_EINVAL, "attn_bwd: SPACE mode needs dqkv_cls");
  VTX_REQUIRE(d->f.mode != VTX_ATTN_TIME_CLS || d->dqkv_cls, VTX_EINVAL, "attn_bwd: TIME_CLS mode needs dqkv_cls");
  VTX_REQUIRE(aligned16(d->dout) && aligned16(d->dqkv), VTX_EALIGN, "attn_bwd: alignment");
  p.ld_dout = d->ld_dout; p.ld_dqkv = d->ld_dqkv;
  hipStream_t st = as_stream(stream);
  if (d->f.mode == VTX_ATTN_SPACE_NOCLS) {           // no sequence holds the cls rows: their gradient is zero
    const size_t es = d->f.dtype == VTX_F32 ? 4 : 2;
    const hipError_t e = hipMemset2DAsync(d->dqkv, (size_t)(1 + (long)d->f.P * d->f.T) * d->ld_dqkv * es, 0,
                                          (size_t)3 * d->f.H * d->f.hd * es, (size_t)d->f.B, st);
    VTX_REQUIRE(e == hipSuccess, VTX_EINVAL, "attn_bwd: zeroing the cls rows of dqkv: %s", hipGetErrorString(e));
  }
  switch (attn_route(d->f.dtype, d->f.mode, d->f.L, d->f.hd, false)) {
    case SMALL: return attn_bwd_small_launch(p, d->f.hd, d->f.qkv, d->f.out, d->dout, d->f.lse, d->dqkv, d->dqkv_cls, st);
    case MFMA: return attn_bwd_mfma_launch(p, d->f.qkv, d->f.out, d->dout, d->f.lse, d->delta, d->dqkv, d->dqkv_cls, st);
    case LONG: return attn_bwd_long_launch(p, d->f.qkv, d->f.out, d->dout, d->f.lse, d->delta, d->dqkv, d->dqkv_cls, st);
    case F32: return attn_bwd_f32_launch(p, d->f.qkv, d->f.out, d->dout, d->f.lse, d->delta, d->dqkv, d->dqkv_cls, st);
    case F32HD: return attn_bwd_hd_f32_launch(p, d->f.hd, d->f.qkv, d->f.out, d->dout, d->f.lse, d->delta, d->dqkv, d->dqkv_cls, st);
    case HDIM: return attn_bwd_hd_launch(p, d->f.hd, d->f.qkv, d->f.out, d->dout, d->f.lse, d->delta, d->dqkv, d->dqkv_cls, st);
    case VALU: break;
  }
  return d->f.dtype == VTX_F32 ? valu_bwd_launch<float>(p, d, st) : valu_bwd_launch<bf16raw>(p, d, st);
}
