// attn_common.h -- launch parameters and row addressing shared by attn.hip (VALU), attn_mfma.hip and the chunk-streaming kernels
// (attn_stream.h with its two tile policies, attn_tiles_bf16.h and attn_tiles_f32.h, instantiated by attn_long.hip, attn_f32.hip
// and attn_hd_f32.hip; attn_hd.hip with the bf16 policy under bodies of its own), and the swizzled-LDS / MFMA fragment helpers of the two bf16 MFMA
// families.
#pragma once
#include "common.h"

namespace vtx {

struct AttnP {
  int mode, S, L, H, B, T, P;
  long ld_qkv, ld_out, ld_dout, ld_dqkv;
  float scale;
  int G;                        // sequences per workgroup
};

// Row addressing of the four layouts (include/vtx.h).  Every layout but CONTIG reads qkv in the natural token order
// [B, 1 + P*T, 3D], tokens in (p t) order:
//   SPACE        s = (b, t), i = 0 the clip's cls row, i >= 1 token row 1 + (i-1)*T + t;   out: tokens, then a cls row per s
//   TIME_CLS     s = (b, p), i = 0 the clip's cls row, i >= 1 token row 1 + p*T + (i-1);   out: tokens, then a cls row per s
//   SPACE_NOCLS  s = (b, t), token row 1 + i*T + t for every i (no cls row);               out: tokens
__device__ inline bool attn_has_cls(int mode) { return mode == VTX_ATTN_SPACE || mode == VTX_ATTN_TIME_CLS; }
// the gradient of row i of sequence s goes to dqkv_cls[s] (one row per sequence, summed by vtx_cls_qkv_reduce), not to dqkv
__device__ inline bool attn_cls_row(const AttnP& p, int i) { return i == 0 && attn_has_cls(p.mode); }
__device__ inline long in_row(const AttnP& p, int s, int i) {
  if (p.mode == VTX_ATTN_CONTIG) return (long)s * p.L + i;
  if (p.mode == VTX_ATTN_TIME_CLS) {
    const int b = s / p.P;                          // token rows of (b, p): b * (1 + P*T) + 1 + p*T + (i-1) = s*T + b + i
    return i == 0 ? (long)b * (1 + (long)p.P * p.T) : (long)s * p.T + b + i;
  }
  const int b = s / p.T, t = s - b * p.T;
  if (p.mode == VTX_ATTN_SPACE_NOCLS) return (long)b * (1 + (long)p.P * p.T) + 1 + (long)i * p.T + t;
  return (long)b * (1 + (long)p.P * p.T) + (i == 0 ? 0 : 1 + (long)(i - 1) * p.T + t);
}
__device__ inline long out_row(const AttnP& p, int s, int i) {
  if (p.mode == VTX_ATTN_CONTIG) return (long)s * p.L + i;
  if (p.mode == VTX_ATTN_TIME_CLS) return i == 0 ? (long)p.B * p.P * p.T + s : (long)s * p.T + (i - 1);
  const int b = s / p.T, t = s - b * p.T;
  if (p.mode == VTX_ATTN_SPACE_NOCLS) return (long)b * p.P * p.T + (long)i * p.T + t;
  return i == 0 ? (long)p.B * p.P * p.T + s : (long)b * p.P * p.T + (long)(i - 1) * p.T + t;
}


// ---- bf16 MFMA building blocks shared by attn_mfma.hip (33..256 tokens), attn_long.hip (> 256) and attn_hd.hip (its packed kernels: <= 32) ----
constexpr int MA_THREADS = 256;
constexpr int MA_MAXT = 8;            // up to 8 tiles of 32 rows (Lp <= 256)
constexpr int MA_KB = 4;              // key tiles per online-softmax block in the forward kernel
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

__device__ inline int sw_of(int row) {
  const int x = (row >> 1) & 7;
  return ((x & 1) << 2) | (x & 2) | ((x >> 2) & 1);
}
// element offset of (row, col) in a swizzled [rows][64] bf16 tile
__device__ inline int sw_off(int row, int col) { return row * 64 + ((((col >> 3) ^ sw_of(row))) << 3) + (col & 7); }

// Fill TWO swizzled LDS tiles (rows gathered through rowfn0 / rowfn1, zero rows beyond nvalid, up to
// Lp <= 256).  All global loads of both tiles are issued before the first LDS store: a load->store
// loop serialises one memory latency per iteration (measured: ~25 us of a 50 us workgroup).
template <int NTHR = 256, typename RowFn0, typename RowFn1>
__device__ inline void fill_tiles2(bf16raw* lds0, bf16raw* lds1, int Lp, int nvalid, const bf16raw* base0, long ld0, int col0,
                                   RowFn0 rowfn0, const bf16raw* base1, long ld1, int col1, RowFn1 rowfn1) {
  constexpr int NI = 2048 / NTHR;
  uint4 v0[NI], v1[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int id = threadIdx.x + i * NTHR;
    const int r = id >> 3, c = id & 7;
    v0[i] = make_uint4(0, 0, 0, 0);
    v1[i] = make_uint4(0, 0, 0, 0);
    if (id < Lp * 8 && r < nvalid) {
      v0[i] = *reinterpret_cast<const uint4*>(base0 + rowfn0(r) * ld0 + col0 + c * 8);
      v1[i] = *reinterpret_cast<const uint4*>(base1 + rowfn1(r) * ld1 + col1 + c * 8);
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int id = threadIdx.x + i * NTHR;
    const int r = id >> 3, c = id & 7;
    if (id < Lp * 8) {
      const int off = r * 64 + ((c ^ sw_of(r)) << 3);
      *reinterpret_cast<uint4*>(lds0 + off) = v0[i];
      *reinterpret_cast<uint4*>(lds1 + off) = v1[i];
    }
  }
}

// Row-wise operand fragment from LDS: lane (l&31) -> row, 8 consecutive columns ks*16 + 8*(l>>5)..
__device__ inline bf16x8 frag_rows(const bf16raw* lds, int row0, int ks, int lane) {
  const int row = row0 + (lane & 31);
  const int c = ks * 2 + (lane >> 5);
  return *reinterpret_cast<const bf16x8*>(lds + row * 64 + ((c ^ sw_of(row)) << 3));
}

// Transposed operand fragment: A[i = column col0 + (l&31)][k] with k running over the 16 rows
// row0..row0+15 in the permuted order {0-3, 8-11 | 4-7, 12-15} (lower | upper half-wave).
__device__ inline bf16x8 frag_cols(const bf16raw* lds, int row0, int col0, int lane) {
  const int r = row0 + 4 * (lane >> 5) + ((lane & 15) >> 2);
  const int c = col0 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  union { bf16x8 v; s16x4 h[2]; } u;
  u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(lds + sw_off(r, c)));
  u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(lds + sw_off(r + 8, c)));
  return u.v;
}

// The same two readers with their per-lane part precomputed.  For a row0 that is a multiple of 16 the swizzle term only
// depends on the lane, so a fragment address is (lane constant) + row0 * 128 B: the kernels keep the lane constants in
// registers (FragOff) and the compiler turns row0 into an immediate / one scalar add -- the generic readers above cost
// 3 (rows) to 6 (columns) vector instructions of index arithmetic per LDS read, in kernels bound by vector-ALU issue.
struct FragOff {
  int rows[4];        // frag_rows: element offset of (row = lane&31, ks)
  int cols[2][2];     // frag_cols: element offset of (n2, half = rows r / r + 8), col0 = n2 * 32
};
__device__ inline FragOff make_frag_off(int lane) {
  FragOff f;
  const int row = lane & 31;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) f.rows[ks] = row * 64 + (((ks * 2 + (lane >> 5)) ^ sw_of(row)) << 3);
  const int r = 4 * (lane >> 5) + ((lane & 15) >> 2);
#pragma unroll
  for (int n2 = 0; n2 < 2; ++n2) {
    const int c = n2 * 32 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    f.cols[n2][0] = sw_off(r, c);
    f.cols[n2][1] = sw_off(r + 8, c);
  }
  return f;
}
__device__ inline bf16x8 frag_rows_o(const bf16raw* lds, int row0, int ks, const FragOff& f) {     // row0 % 32 == 0
  return *reinterpret_cast<const bf16x8*>(lds + row0 * 64 + f.rows[ks]);
}
__device__ inline bf16x8 frag_cols_o(const bf16raw* lds, int row0, int n2, const FragOff& f) {     // row0 % 16 == 0
  union { bf16x8 v; s16x4 h[2]; } u;
  u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(lds + row0 * 64 + f.cols[n2][0]));
  u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(lds + row0 * 64 + f.cols[n2][1]));
  return u.v;
}

// Row addressing of one sequence in closed form: row(i) = i == 0 ? row0 : base + i * stride (contiguous sequences:
// row0 = base, stride 1; divided spatial attention: row 0 is the clip's cls row / its per-frame copy, token i >= 1 sits
// i * T rows further; temporal attention over the cls token: the same row 0, tokens on consecutive rows; spatial attention
// without the cls token: every row on the line, T rows apart).  in_row / out_row (attn_common.h) compute the same rows with
// a division per call; per lane and row that was ~40 vector instructions around every fragment load and row store of
// kernels bound by vector-ALU issue.
struct RowLin { long row0, base, stride; };
__device__ inline RowLin lin_in(const AttnP& p, int s) {
  RowLin r;
  if (p.mode == VTX_ATTN_CONTIG) { r.base = (long)s * p.L; r.stride = 1; r.row0 = r.base; return r; }
  if (p.mode == VTX_ATTN_TIME_CLS) {
    const int b = s / p.P;
    r.row0 = (long)b * (1 + (long)p.P * p.T);
    r.stride = 1;
    r.base = (long)s * p.T + b;                 // row(i) = b * (1 + P*T) + 1 + p*T + (i - 1)
    return r;
  }
  const int b = s / p.T, t = s - b * p.T;
  r.row0 = (long)b * (1 + (long)p.P * p.T);
  r.stride = p.T;
  if (p.mode == VTX_ATTN_SPACE_NOCLS) { r.base = r.row0 + 1 + t; r.row0 = r.base; return r; }
  r.base = r.row0 + 1 + t - r.stride;           // row(i) = row0 + 1 + (i - 1) * T + t
  return r;
}
__device__ inline RowLin lin_out(const AttnP& p, int s) {
  RowLin r;
  if (p.mode == VTX_ATTN_CONTIG) { r.base = (long)s * p.L; r.stride = 1; r.row0 = r.base; return r; }
  if (p.mode == VTX_ATTN_TIME_CLS) {
    r.row0 = (long)p.B * p.P * p.T + s;
    r.stride = 1;
    r.base = (long)s * p.T - 1;                 // row(i) = (b*P + p) * T + (i - 1)
    return r;
  }
  const int b = s / p.T, t = s - b * p.T;
  r.stride = p.T;
  if (p.mode == VTX_ATTN_SPACE_NOCLS) { r.base = (long)b * p.P * p.T + t; r.row0 = r.base; return r; }
  r.row0 = (long)p.B * p.P * p.T + s;
  r.base = (long)b * p.P * p.T + t - r.stride;  // row(i) = b * P * T + (i - 1) * T + t
  return r;
}
__device__ inline long lin_row(const RowLin& r, int i) { return i == 0 ? r.row0 : r.base + (long)i * r.stride; }

// The four row-wise fragments (64 columns) of row `row` of a [.., ld] matrix, column origin col0; rows beyond nvalid read
// row nvalid - 1 instead (no branch, one address per row): every kernel below keeps a padded query / key in its own lane
// and never stores its results, so its operands only have to be finite.
__device__ inline void load_row_frags(bf16x8 (&f)[4], const bf16raw* base, long ld, int col0, const RowLin& rl, int row, int nvalid,
                                      int lane) {
  const int rc = row < nvalid ? row : nvalid - 1;
  const bf16raw* src = base + lin_row(rl, rc) * ld + col0 + 8 * (lane >> 5);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    union { bf16x8 v; uint4 u; } x;
    x.u = *reinterpret_cast<const uint4*>(src + ks * 16);
    f[ks] = x.v;
  }
}
// sum_j a[j] * b[j] over the 8 bf16 pairs of two fragments, accumulated into acc (v_dot2c_f32_bf16: exact products, fp32 sum)
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_;
__device__ inline float frag_dot2(const bf16x8& a, const bf16x8& b, float acc) {
  union { bf16x8 v; bf16x2_ h[4]; } ua, ub;
  ua.v = a; ub.v = b;
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_fdot2_f32_bf16(ua.h[j], ub.h[j], acc, false);
  return acc;
}

// Row-wise operand fragment straight from global memory (rows beyond nvalid read as zero).
template <typename RowFn>
__device__ inline bf16x8 frag_global(const bf16raw* base, long ld, int col0, int row, int nvalid, int ks, int lane, RowFn rowfn) {
  union { bf16x8 v; uint4 u; } x;
  x.u = make_uint4(0, 0, 0, 0);
  if (row < nvalid) x.u = *reinterpret_cast<const uint4*>(base + rowfn(row) * ld + col0 + ks * 16 + 8 * (lane >> 5));
  return x.v;
}

__device__ inline bf16x8 pack8(const float* f) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (__bf16)f[j];
  return v;
}
__device__ inline float frag_dot(const bf16x8& a, const bf16x8& b) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += (float)a[j] * (float)b[j];
  return s;
}
__device__ inline void zero16(f32x16& a) {
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
}
// row index (within a 32-row tile) that accumulator register r of this lane holds
__device__ inline int crow(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

constexpr int MA_STAGE_ELEMS = 32 * 64;   // per-wave [32][64] bf16 staging tile for row stores (4 KB)

__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
}

// Store a [32 x 64] result held transposed (lane&31 = row, registers = 64 columns in two C tiles).
// The accumulator layout gives each lane 8-byte pieces of 32 different rows -- stored directly that
// is 16 B per row per instruction (measured: 47 us of a 153 us forward).  Stage through a wave-private
// swizzled LDS tile instead and write whole 128-B rows: 8 lanes x 16 B, 8 rows per instruction.
// ptr_of_row(r) -> destination of tile row r (64 bf16), or nullptr for a padded row.
template <typename PtrFn>
__device__ inline void store_rows_T(bf16raw* stg, const f32x16 (&acc)[2], float mul, int lane, PtrFn ptr_of_row) {
  const int row = lane & 31;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int col = nt * 32 + 8 * g + 4 * (lane >> 5);
      union { bf16x4 v; uint2 u; } w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w.v[j] = (__bf16)(acc[nt][4 * g + j] * mul);
      *reinterpret_cast<uint2*>(stg + sw_off(row, col)) = w.u;
    }
  wave_lds_sync();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = i * 8 + (lane >> 3), c = lane & 7;
    const uint4 v = *reinterpret_cast<const uint4*>(stg + r * 64 + ((c ^ sw_of(r)) << 3));
    bf16raw* dst = ptr_of_row(r);
    if (dst) *reinterpret_cast<uint4*>(dst + c * 8) = v;
  }
  wave_lds_sync();
}


// attn_mfma.hip
bool attn_mfma_eligible(int dtype, int mode, int L, int hd);
int attn_fwd_mfma_launch(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st);
int attn_bwd_mfma_launch(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse,
                         float* delta, void* dqkv, void* dqkv_cls, hipStream_t st);
// attn_long.hip
bool attn_long_eligible(int dtype, int L, int hd);
int attn_fwd_long_launch(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st);
int attn_bwd_long_launch(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse,
                         float* delta, void* dqkv, void* dqkv_cls, hipStream_t st);
// attn_f32.hip
bool attn_f32_eligible(int dtype, int L, int hd);
int attn_fwd_f32_launch(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st);
int attn_bwd_f32_launch(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse,
                        float* delta, void* dqkv, void* dqkv_cls, hipStream_t st);
// attn_hd.hip (head_dim 32, 96, 128, more than 32 tokens)
bool attn_hd_eligible(int dtype, int L, int hd);
int attn_fwd_hd_launch(const AttnP& p, int hd, const void* qkv, void* out, float* lse, hipStream_t st);
int attn_bwd_hd_launch(const AttnP& p, int hd, const void* qkv, const void* o, const void* dout, const float* lse, float* delta,
                       void* dqkv, void* dqkv_cls, hipStream_t st);
// attn_hd.hip, up to 32 tokens (bf16, CONTIG and TIME_CLS, head_dim 32, 64, 96, 128): the packed kernels
bool attn_small_eligible(int dtype, int mode, int L, int hd);
int attn_fwd_small_launch(const AttnP& p, int hd, const void* qkv, void* out, float* lse, hipStream_t st);
int attn_bwd_small_launch(const AttnP& p, int hd, const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv,
                          void* dqkv_cls, hipStream_t st);
// attn_hd_f32.hip (fp32, head_dim 32, 96, 128, more than 32 tokens)
bool attn_hd_f32_eligible(int dtype, int L, int hd);
int attn_fwd_hd_f32_launch(const AttnP& p, int hd, const void* qkv, void* out, float* lse, hipStream_t st);
int attn_bwd_hd_f32_launch(const AttnP& p, int hd, const void* qkv, const void* o, const void* dout, const float* lse, float* delta,
                           void* dqkv, void* dqkv_cls, hipStream_t st);

}  // namespace vtx
