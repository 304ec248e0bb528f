// attn_long.hip -- bf16 MFMA attention core for sequences of more than 256 tokens, head_dim 64
// (joint space-time attention of TimeSformer / ViViT: L = 1 + 196 * 8 = 1569; the divided spatial attention of a
// 448^2 model: L = 785).  Both VTX_ATTN_CONTIG and VTX_ATTN_SPACE, forward and backward.
//
// The three kernels are the chunk-streaming bodies of attn_stream.h over the bf16 tile policy of attn_tiles_bf16.h; this file
// chooses the policy's parameters and holds the kernels' names, launch bounds and launchers.  K and V (Q and dO in the dk / dv
// kernel) stream in chunks of 128 rows: 2 stages x 2 tiles x 16 KiB = 64 KiB (+ 2 KiB of lse / delta in the dk / dv kernel),
// two workgroups a CU.
#include "attn_tiles_bf16.h"

namespace vtx {

typedef Bf16Tiles<64, 128> LongTiles;
static_assert(stream_lds_kv<LongTiles>() == 65536 && stream_lds_dkv<LongTiles>() == 67584, "dynamic LDS of a launch");

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
  return stream_bwd_launch<LongTiles, attn_bwd_dq_long_kernel, LongTiles, attn_bwd_dkv_long_kernel>(
      "attn_bwd_dq_long", "attn_bwd_dkv_long", p, qkv, o, dout, lse, delta, dqkv, dqkv_cls, st);
}

}  // namespace vtx
