// Shared by the whole-parameter-list kernels (adamw.hip, grad_clip.hip, muon.hip): their device tables and
// a workgroup's row of them, the gradient load, the workgroup sum and the stochastic rounding.
//
// tensors: [n_tensors][5] = (param, grad, exp_avg, exp_avg_sq pointers, grad_is_f32) as int64 (muon.hip: param,
// grad, momentum_buffer, work, grad_is_f32); sizes: [n_tensors] numel; chunks: [n_chunks][2] (tensor index, first
// element).
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int OPT_CHUNK = 65536;  // elements per workgroup

// The chunk of workgroup blockIdx.x: tensor index, first element, the tensor's row of `tensors` and its numel.
struct OptChunk {
  int64_t ti, c0;
  const int64_t* t;
  int64_t n;
};

PICO_DEV OptChunk opt_chunk(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks) {
  const int64_t ti = chunks[2 * blockIdx.x], c0 = chunks[2 * blockIdx.x + 1];
  return {ti, c0, tensors + 5 * ti, sizes[ti]};
}

// *out = the sum of s over a workgroup of 256 lanes (all of them call), in the fixed order that pico_grad_sqnorm
// documents (grad_clip.hip): wave_sum_dpp over the 64 lanes, then the four waves' sums pairwise through LDS.
PICO_DEV void block_sum_store(float s, float* out) {
  __shared__ float wave_part[4];
  s = wave_sum_dpp(s);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

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

// ---- stochastic rounding fp32 -> bf16 from a counter-based generator (pico_adamw_bf16_sr, pico_sr_round_bf16) ----
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"; Random123's known answers are
// restated in tests/test_adamw_sr_host.py), in registers: no generator state in memory. One 32 x 32 -> 64
// product per v_mad_u64_u32.
PICO_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                            uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t a = (uint64_t)0xD2511F53u * c0, b = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(b >> 32) ^ c1 ^ k0, n2 = (uint32_t)(a >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)b;
    c3 = (uint32_t)a;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// key = the 64-bit seed (low, high word); counter = (element index >> 3, tensor id, step, quantity), quantity
// 0 = parameter, 1 = exp_avg, 2 = exp_avg_sq. A step's bits are a pure function of these.
struct SrKey {
  uint32_t k0, k1, step;
};

// The four words of one call are the 16-bit values of the eight elements i & ~7 .. i | 7.
PICO_DEV void sr_words(const SrKey& k, uint32_t id, int64_t i, uint32_t quantity, uint32_t (&w)[4]) {
  philox4x32_10((uint32_t)(i >> 3), id, k.step, quantity, k.k0, k.k1, w);
}

PICO_DEV uint32_t sr_lane(const uint32_t (&w)[4], int j) { return (w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu; }

// u: the fp32 bit pattern, r: 16 random bits. Adding r below the kept bits rounds the magnitude up with
// probability (u & 0xFFFF) / 65536: the expectation is the fp32 value, a value exact in bf16 never changes.
// inf / NaN take f2bf; a finite value is never carried to inf (it keeps its truncation, the largest finite bf16).
// (A select-only form with v_cmp_class_f32 tests measured 2 % faster without the clip and the same with it, at 82
// instead of 72 VGPRs: DESIGN.md §4i.)
PICO_DEV unsigned short f2bf_sr(uint32_t u, uint32_t r) {
  if ((u & 0x7F800000u) == 0x7F800000u) return f2bf(__uint_as_float(u));
  uint32_t t = u + r;
  if ((t & 0x7F800000u) == 0x7F800000u) t = u;
  return (unsigned short)(t >> 16);
}
