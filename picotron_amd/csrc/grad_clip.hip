// Global L2 gradient norm and clip over every parameter of a model (HBM-bound), on the AdamW step's device
// tables (optim_common.h; only the gradient pointer and grad_is_f32 columns are read).
//
// Replaces torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm): ATen computes one norm per tensor in
// multi_tensor_apply launches (~60 per SmolLM-1.7B step), then a norm of norms, then writes the scaled
// gradients back. Here:
//   pico_grad_sqnorm    one workgroup per 64 Ki-element chunk writes one fp32 partial sum of squares; a second
//                       launch (one workgroup) adds the partials in index order in double -> sumsq (device double).
//                       No atomics: the same tables give the same bits on every run.
//   pico_grad_clip_coef (norm, coef) = (sqrt(sumsq), min(1, max_norm / (norm + 1e-6))), torch's formula, on the
//                       device; its own launch because the model-parallel path all-reduces sumsq before it.
//   pico_grad_scale     g = bf16(g * coef) in place (the standalone clip; pico_adamw_bf16_clip folds the same
//                       product into the optimizer's gradient load instead).
// Bytes per element: sqnorm reads 2 (4 for an fp32 main_grad); scale reads 2 and writes 2 (4 + 4).
// Summation order of one chunk (fixed): lane t takes 8-element vectors t, t + 256, ... (32 per full chunk) into 8
// fp32 accumulators, one per vector slot, adds them pairwise, then wave_sum_dpp over the 64 lanes, then the four
// waves' sums pairwise through LDS. The scalar path (unaligned pointer or numel % 8 != 0) gives lane t elements
// t, t + 256, ... (256 per full chunk) in one accumulator.
#include "optim_common.h"

namespace {

template <bool GF32>
PICO_DEV float sqnorm_chunk(const void* g, int64_t n, int64_t c0) {
  const int64_t end = min(n, c0 + OPT_CHUNK);
  float s;
  if (grad_vec_ok<GF32>(g, n)) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int64_t i0 = c0 + 8 * (int64_t)threadIdx.x;
    if (end - c0 == OPT_CHUNK) {  // a full chunk: fixed trip count, so the loads of several iterations are in flight
#pragma unroll 8
      for (int it = 0; it < OPT_CHUNK / (8 * 256); ++it) {
        float gf[8];
        load_grad8<GF32>(g, i0 + (int64_t)it * (8 * 256), gf);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += gf[j] * gf[j];
      }
    } else {
      for (int64_t i = i0; i < end; i += 8 * 256) {
        float gf[8];
        load_grad8<GF32>(g, i, gf);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += gf[j] * gf[j];
      }
    }
    s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  } else {
    s = 0.f;
    for (int64_t i = c0 + threadIdx.x; i < end; i += 256) {
      const float gf = load_grad1<GF32>(g, i);
      s += gf * gf;
    }
  }
  return s;
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const int64_t* __restrict__ tensors,
                                                          const int64_t* __restrict__ sizes,
                                                          const int64_t* __restrict__ chunks,
                                                          float* __restrict__ partial) {
  const OptChunk c = opt_chunk(tensors, sizes, chunks);
  const void* g = (const void*)c.t[1];
  const float s = c.t[4] ? sqnorm_chunk<true>(g, c.n, c.c0) : sqnorm_chunk<false>(g, c.n, c.c0);
  block_sum_store(s, partial + blockIdx.x);
}

// One workgroup: lane t adds partials t, t + 256, ... in double, then a fixed LDS tree over the 256 lanes.
__global__ __launch_bounds__(256) void grad_sqnorm_final_kernel(const float* __restrict__ partial, int64_t n,
                                                                double* __restrict__ sumsq) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) a += (double)partial[i];
  sh[threadIdx.x] = a;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) sumsq[0] = sh[0];
}

__global__ __launch_bounds__(64) void grad_clip_coef_kernel(const double* __restrict__ sumsq, float max_norm,
                                                            float* __restrict__ norm_coef) {
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(sumsq[0]);
  norm_coef[0] = norm;
  norm_coef[1] = fminf(1.0f, max_norm / (norm + 1e-6f));
}

// bf16: g = bf16(float(g) * coef). fp32 main_grad: g32 = float(bf16(float(bf16(g32)) * coef)), the value the bf16
// form would hold, so a later deferred-cast step rounds it to the same bits.
template <bool GF32>
PICO_DEV void scale_chunk(void* g, int64_t n, int64_t c0, float coef) {
  const int64_t end = min(n, c0 + OPT_CHUNK);
  if (grad_vec_ok<GF32>(g, n)) {
    for (int64_t i = c0 + 8 * (int64_t)threadIdx.x; i < end; i += 8 * 256) {
      float gf[8];
      load_grad8<GF32>(g, i, gf);
      if constexpr (GF32) {
        f32x4 a, b;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] = bf2f(f2bf(gf[j] * coef));
          b[j] = bf2f(f2bf(gf[4 + j] * coef));
        }
        reinterpret_cast<f32x4*>((float*)g + i)[0] = a;
        reinterpret_cast<f32x4*>((float*)g + i)[1] = b;
      } else {
        u16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f2bf(gf[j] * coef);
        *reinterpret_cast<u16x8*>((bf16_t*)g + i) = o;
      }
    }
  } else {
    for (int64_t i = c0 + threadIdx.x; i < end; i += 256) {
      const unsigned short o = f2bf(load_grad1<GF32>(g, i) * coef);
      if constexpr (GF32) ((float*)g)[i] = bf2f(o);
      else ((bf16_t*)g)[i] = o;
    }
  }
}

// Nothing is written when coef == 1 (the product would store the same bf16 bits) or when the norm is not finite
// (the rule of pico_adamw_bf16_clip: an inf / NaN gradient leaves everything as it was).
__global__ __launch_bounds__(256) void grad_scale_kernel(const int64_t* __restrict__ tensors,
                                                         const int64_t* __restrict__ sizes,
                                                         const int64_t* __restrict__ chunks,
                                                         const float* __restrict__ norm_coef) {
  const float norm = norm_coef[0], coef = norm_coef[1];
  if (!isfinite(norm) || coef == 1.0f) return;
  const OptChunk c = opt_chunk(tensors, sizes, chunks);
  void* g = (void*)c.t[1];
  if (c.t[4]) scale_chunk<true>(g, c.n, c.c0, coef);
  else scale_chunk<false>(g, c.n, c.c0, coef);
}

}  // namespace

extern "C" int64_t pico_grad_sqnorm_workspace_bytes(int64_t n_chunks) {
  return n_chunks > 0 ? n_chunks * (int64_t)sizeof(float) : 0;
}

extern "C" int pico_grad_sqnorm(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks, int64_t n_chunks,
                                void* workspace, double* sumsq, void* stream) {
  PICO_REQUIRE(n_chunks >= 0 && n_chunks < (1ll << 31), "pico_grad_sqnorm: bad chunk count");
  PICO_REQUIRE(sumsq, "pico_grad_sqnorm: null sumsq");
  PICO_REQUIRE(n_chunks == 0 || (tensors && sizes && chunks), "pico_grad_sqnorm: null table");
  PICO_REQUIRE(n_chunks == 0 || workspace, "pico_grad_sqnorm: null workspace");
  hipStream_t s = (hipStream_t)stream;
  if (n_chunks > 0)
    PICO_TRY(pico_launch(PICO_K_GRAD_SQNORM, "grad_sqnorm", grad_sqnorm_kernel, dim3((int)n_chunks), dim3(256), 0, s,
                         tensors, sizes, chunks, (float*)workspace));
  // not timed: one workgroup over n_chunks floats (an empty list: sumsq = 0)
  PICO_TRY(pico_launch(0, "grad_sqnorm_final", grad_sqnorm_final_kernel, dim3(1), dim3(256), 0, s,
                       (const float*)workspace, n_chunks, sumsq));
  return 0;
}

extern "C" int pico_grad_clip_coef(const double* sumsq, double max_norm, float* norm_coef, void* stream) {
  PICO_REQUIRE(max_norm >= 0.0, "pico_grad_clip_coef: max_norm must be >= 0 (got %g)", max_norm);  // NaN fails too
  PICO_REQUIRE(sumsq && norm_coef, "pico_grad_clip_coef: null sumsq / norm_coef");
  PICO_TRY(pico_launch(0, "grad_clip_coef", grad_clip_coef_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sumsq,
                       (float)max_norm, norm_coef));
  return 0;
}

extern "C" int pico_grad_scale(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks, int64_t n_chunks,
                               const float* norm_coef, void* stream) {
  PICO_REQUIRE(n_chunks >= 0 && n_chunks < (1ll << 31), "pico_grad_scale: bad chunk count");
  PICO_REQUIRE(norm_coef, "pico_grad_scale: null norm_coef");
  if (n_chunks == 0) return 0;
  PICO_REQUIRE(tensors && sizes && chunks, "pico_grad_scale: null table");
  PICO_TRY(pico_launch(PICO_K_GRAD_SCALE, "grad_scale", grad_scale_kernel, dim3((int)n_chunks), dim3(256), 0,
                       (hipStream_t)stream, tensors, sizes, chunks, norm_coef));
  return 0;
}
