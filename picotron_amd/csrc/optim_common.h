// Shared by the whole-parameter-list kernels (adamw.hip, grad_clip.hip): the chunk size of their device
// tables and the gradient load.
//
// tensors: [n_tensors][5] = (param, grad, exp_avg, exp_avg_sq pointers, grad_is_f32) as int64; sizes:
// [n_tensors] numel; chunks: [n_chunks][2] (tensor index, first element).
#pragma once
#include "common.h"

constexpr int OPT_CHUNK = 65536;  // elements per workgroup

// grad_is_f32 = 1: the gradient is DataParallelBucket's averaged fp32 main_grad (its bf16 .grad cast
// deferred, ref picotron/data_parallel/data_parallel.py:165): each element is rounded to bf16 in register
// exactly as pico_cast_f32_bf16 would store it, so the step is bit-identical to cast-then-step, without the
// bf16 .grad write and re-read.
template <bool GF32>
PICO_DEV void load_grad8(const void* g, int64_t i, float (&out)[8]) {
  if constexpr (GF32) {
    const f32x4 a = reinterpret_cast<const f32x4*>((const float*)g + i)[0];
    const f32x4 b = reinterpret_cast<const f32x4*>((const float*)g + i)[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      out[j] = bf2f(f2bf(a[j]));
      out[4 + j] = bf2f(f2bf(b[j]));
    }
  } else {
    const u16x8 gv = *reinterpret_cast<const u16x8*>((const bf16_t*)g + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = bf2f(gv[j]);
  }
}

// the scalar load of the same value (unaligned pointers, n % 8 != 0)
template <bool GF32>
PICO_DEV float load_grad1(const void* g, int64_t i) {
  return GF32 ? bf2f(f2bf(((const float*)g)[i])) : bf2f(((const bf16_t*)g)[i]);
}

// 16-byte vector access to a gradient tensor of n elements (32-byte for fp32: two f32x4 per 8 elements)
template <bool GF32>
PICO_DEV bool grad_vec_ok(const void* g, int64_t n) {
  return (((uintptr_t)g & (GF32 ? 31 : 15)) == 0) && (n % 8 == 0);
}
