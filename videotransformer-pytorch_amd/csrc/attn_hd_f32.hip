// attn_hd_f32.hip -- exact-fp32 MFMA attention core for fp32 inputs, head_dim 32, 96 and 128, more than 32 tokens per sequence,
// all four layouts, forward and backward.  Every product runs on v_mfma_f32_32x32x2_f32: fp32 operands, an fma chain with fp32
// rounding after every step -- the arithmetic of the VALU kernels of attn.hip in another summation order.  Scores, probabilities
// and accumulators stay fp32 registers from the first product to the store: no value is ever rounded to bf16.
//
// The three kernels are the chunk-streaming bodies of attn_stream.h (read its header first: transposed scores, a workgroup of 4
// waves owns 128 queries -- 128 keys in the dk / dv kernel --, the other operands stream through two LDS stages, one barrier per
// chunk, dk / dv with one workgroup per key block walking all queries: fixed summation order, no atomics, no workspace, the
// masking) over the fp32 tile policy of attn_tiles_f32.h (read its header for the operand layouts of the 32x32x2 MFMA and for
// what a head of HD columns is) -- the bodies and the policy of attn_f32.hip at head_dim 64.  This file holds what is its own:
// the chunk rows and the workgroups per CU of each (head dim, kernel), the kernels' names and the launchers.
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
#include "attn_tiles_f32.h"

namespace vtx {
namespace hdf32 {

// rows per chunk and workgroups per CU of (head dim, kernel): see Resources above
enum Kern { FWD, DQ, DKV };
constexpr int occ_of(int hd, Kern k) { return hd == 32 ? 3 : hd == 96 ? (k == DKV ? 1 : 2) : (k == FWD ? 2 : 1); }
constexpr int chunk_of(int hd, Kern k) { return hd == 32 || occ_of(hd, k) == 1 ? 64 : 32; }    // alone on its CU: half the barriers

template <int HD, Kern K> using Tiles = F32Tiles<HD, chunk_of(HD, K)>;

// dynamic LDS of a launch: forward, dq, dk / dv
template <int HD> constexpr bool lds_is(size_t fwd, size_t dq, size_t dkv) {
  return stream_lds_kv<Tiles<HD, FWD>>() == fwd && stream_lds_kv<Tiles<HD, DQ>>() == dq && stream_lds_dkv<Tiles<HD, DKV>>() == dkv;
}
static_assert(lds_is<32>(36864, 36864, 37888) && lds_is<96>(51200, 51200, 103424) && lds_is<128>(67584, 135168, 136192),
              "dynamic LDS of a launch");

template <int HD>
__global__ __launch_bounds__(AS_THREADS, occ_of(HD, FWD)) void fwd_kernel(AttnP p, const float* __restrict__ qkv, float* __restrict__ out,
                                                                          float* __restrict__ lse) {
  stream_fwd<Tiles<HD, FWD>>(p, qkv, out, lse);
}
template <int HD>
__global__ __launch_bounds__(AS_THREADS, occ_of(HD, DQ)) void bwd_dq_kernel(AttnP p, const float* __restrict__ qkv, const float* __restrict__ o,
                                                                            const float* __restrict__ dout, const float* __restrict__ lse,
                                                                            float* __restrict__ delta, float* __restrict__ dqkv,
                                                                            float* __restrict__ dqkv_cls) {
  stream_bwd_dq<Tiles<HD, DQ>>(p, qkv, o, dout, lse, delta, dqkv, dqkv_cls);
}
template <int HD>
__global__ __launch_bounds__(AS_THREADS, occ_of(HD, DKV)) void bwd_dkv_kernel(AttnP p, const float* __restrict__ qkv,
                                                                              const float* __restrict__ dout, const float* __restrict__ lse,
                                                                              const float* __restrict__ delta, float* __restrict__ dqkv,
                                                                              float* __restrict__ dqkv_cls) {
  stream_bwd_dkv<Tiles<HD, DKV>>(p, qkv, dout, lse, delta, dqkv, dqkv_cls);
}

// host side ---------------------------------------------------------------------------------------
template <int HD>
static int fwd_launch(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st) {
  return stream_fwd_launch<Tiles<HD, FWD>, fwd_kernel<HD>>("attn_fwd_hd_f32", p, qkv, out, lse, st);
}
template <int HD>
static int bwd_launch(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                      void* dqkv_cls, hipStream_t st) {
  return stream_bwd_launch<Tiles<HD, DQ>, bwd_dq_kernel<HD>, Tiles<HD, DKV>, bwd_dkv_kernel<HD>>(
      "attn_bwd_dq_hd_f32", "attn_bwd_dkv_hd_f32", p, qkv, o, dout, lse, delta, dqkv, dqkv_cls, st);
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
