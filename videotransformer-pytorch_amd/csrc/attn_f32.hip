// attn_f32.hip -- exact-fp32 MFMA attention core for fp32 inputs, head_dim 64, more than 32 tokens per sequence
// (joint space-time: 1569; spatial: 197 at 224^2, 785 at 448^2; ViViT encoders).  VTX_ATTN_CONTIG and VTX_ATTN_SPACE,
// forward and backward.  Every product runs on v_mfma_f32_32x32x2_f32: fp32 operands, an fma chain with fp32 rounding after
// every step -- the same arithmetic as the VALU kernels of attn.hip in another summation order.  Scores, probabilities and
// accumulators stay fp32 registers from the first product to the store: no value is ever rounded to bf16.
//
// The three kernels are the chunk-streaming bodies of attn_stream.h (the masking and the launchers live there) over the fp32
// tile policy of attn_tiles_f32.h (read its header for the operand layouts of the 32x32x2 MFMA); this file chooses the
// policy's parameters and holds the kernels' names, launch bounds and launchers.  Chunks of 64 rows: a stage is two [64][68]
// fp32 tiles (34 KiB); two stages = 68 KiB (+ 1 KiB of lse / delta in the dk / dv kernel), two workgroups a CU.  In the dq
// kernel a padded key's dS multiplies a zero K row and is not masked.
#include "attn_tiles_f32.h"

namespace vtx {

typedef F32Tiles<64, 64> F32Tiles64;
static_assert(stream_lds_kv<F32Tiles64>() == 69632 && stream_lds_dkv<F32Tiles64>() == 70656, "dynamic LDS of a launch");

__global__ __launch_bounds__(AS_THREADS, 2) void attn_fwd_f32_kernel(AttnP p, const float* __restrict__ qkv, float* __restrict__ out,
                                                                     float* __restrict__ lse) {
  stream_fwd<F32Tiles64>(p, qkv, out, lse);
}
__global__ __launch_bounds__(AS_THREADS, 2) void attn_bwd_dq_f32_kernel(AttnP p, const float* __restrict__ qkv, const float* __restrict__ o,
                                                                        const float* __restrict__ dout, const float* __restrict__ lse,
                                                                        float* __restrict__ delta, float* __restrict__ dqkv,
                                                                        float* __restrict__ dqkv_cls) {
  stream_bwd_dq<F32Tiles64>(p, qkv, o, dout, lse, delta, dqkv, dqkv_cls);
}
__global__ __launch_bounds__(AS_THREADS, 2) void attn_bwd_dkv_f32_kernel(AttnP p, const float* __restrict__ qkv,
                                                                         const float* __restrict__ dout, const float* __restrict__ lse,
                                                                         const float* __restrict__ delta, float* __restrict__ dqkv,
                                                                         float* __restrict__ dqkv_cls) {
  stream_bwd_dkv<F32Tiles64>(p, qkv, dout, lse, delta, dqkv, dqkv_cls);
}

// host-side launchers used by attn.hip's entry points --------------------------------------
bool attn_f32_eligible(int dtype, int L, int hd) { return dtype == VTX_F32 && hd == 64 && L > 32; }

int attn_fwd_f32_launch(const AttnP& p, const void* qkv, void* out, float* lse, hipStream_t st) {
  return stream_fwd_launch<F32Tiles64, attn_fwd_f32_kernel>("attn_fwd_f32", p, qkv, out, lse, st);
}

int attn_bwd_f32_launch(const AttnP& p, const void* qkv, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                        void* dqkv_cls, hipStream_t st) {
  return stream_bwd_launch<F32Tiles64, attn_bwd_dq_f32_kernel, F32Tiles64, attn_bwd_dkv_f32_kernel>(
      "attn_bwd_dq_f32", "attn_bwd_dkv_f32", p, qkv, o, dout, lse, delta, dqkv, dqkv_cls, st);
}

}  // namespace vtx
