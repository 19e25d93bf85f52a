// Muon's HBM passes for gfx950 over every matrix of a parameter list (HBM-bound), on the AdamW step's device
// tables (optim_common.h). The Newton-Schulz GEMMs between them stay on hipBLASLt (picotron_amd/optim.py).
//
// Replaces the elementwise half of torch.optim.Muon's single-tensor step (two lerps, a norm, a clamp, a div, a mul
// and an add per matrix, each with its own temporary) with whole-list launches that keep torch's rounding points:
// fp32 arithmetic, every named result rounded once to bf16 (round to nearest even).
// tensors: [n][5] = (param, grad, momentum_buffer, work, grad_is_f32); work is the tensor's slice of the
// Newton-Schulz input buffer. One workgroup of 256 lanes per 64 Ki-element chunk, 8 elements per lane with 16-byte
// accesses (32-byte for an fp32 main_grad) when the pointers and numel % 8 allow, one element per lane otherwise:
// the same values either way. No atomics: the same inputs give the same bits on every run.
//   pico_muon_momentum   m' = bf16(lerp(m, g, 1 - momentum)); u = nesterov ? bf16(lerp(g, m', momentum)) : m';
//                        m' -> momentum_buffer, u -> work, one fp32 sum of squares of the bf16 u per chunk in
//                        pico_grad_sqnorm's summation order (grad_clip.hip). 8 B per element (10 with fp32 main_grad).
//   pico_muon_normalize  norms[t] = max(float(bf16(sqrt(sum of the tensor's chunk partials, index order, double))),
//                        (float)eps), then work = bf16(work / norms[t]) (a true division). 4 B per element.
//   pico_muon_update     p = bf16(p * (float)(1 - lr wd)); p = bf16(p + (float)(-(lr ratio[t])) * O): torch's mul_
//                        then add_(O, alpha), two roundings. 6 B per element.
// lerp(a, b, w) is ATen's: |w| < 0.5 ? a + w (b - a) : b - (b - a)(1 - w), w cast to fp32.
#include "optim_common.h"

namespace {

PICO_DEV float lerp_aten(float a, float b, float w) {
  const float d = b - a;
  return fabsf(w) < 0.5f ? a + w * d : b - d * (1.0f - w);
}

struct MuonMom {
  float w_grad, momentum;  // (float)(1 - momentum), (float)momentum
  int nesterov;
};

PICO_DEV float momentum_elem(float g, unsigned short& m, unsigned short& u, const MuonMom& h) {
  m = f2bf(lerp_aten(bf2f(m), g, h.w_grad));
  u = h.nesterov ? f2bf(lerp_aten(g, bf2f(m), h.momentum)) : m;
  return bf2f(u);
}

// Returns the lane's share of the chunk's sum of squares of u, accumulated as sqnorm_chunk (grad_clip.hip) does.
template <bool GF32>
PICO_DEV float momentum_chunk(const void* g, bf16_t* m, bf16_t* u, int64_t n, int64_t c0, const MuonMom& h) {
  const int64_t end = min(n, c0 + OPT_CHUNK);
  const bool vec = ((((uintptr_t)m | (uintptr_t)u) & 15) == 0) && grad_vec_ok<GF32>(g, n);
  float s;
  if (vec) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t i = c0 + 8 * (int64_t)threadIdx.x; i < end; i += 8 * 256) {
      u16x8 mv = *reinterpret_cast<const u16x8*>(m + i), uv;
      float gf[8];
      load_grad8<GF32>(g, i, gf);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        unsigned short mb = mv[j], ub;
        const float uf = momentum_elem(gf[j], mb, ub, h);
        mv[j] = mb;
        uv[j] = ub;
        acc[j] += uf * uf;
      }
      *reinterpret_cast<u16x8*>(m + i) = mv;
      *reinterpret_cast<u16x8*>(u + i) = uv;
    }
    s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  } else {
    s = 0.f;
    for (int64_t i = c0 + threadIdx.x; i < end; i += 256) {
      unsigned short mb = m[i], ub;
      const float uf = momentum_elem(load_grad1<GF32>(g, i), mb, ub, h);
      m[i] = mb;
      u[i] = ub;
      s += uf * uf;
    }
  }
  return s;
}

__global__ __launch_bounds__(256) void muon_momentum_kernel(const int64_t* __restrict__ tensors,
                                                            const int64_t* __restrict__ sizes,
                                                            const int64_t* __restrict__ chunks, MuonMom h,
                                                            float* __restrict__ partial) {
  const OptChunk c = opt_chunk(tensors, sizes, chunks);
  const void* g = (const void*)c.t[1];
  bf16_t* m = (bf16_t*)c.t[2];
  bf16_t* u = (bf16_t*)c.t[3];
  const float s = c.t[4] ? momentum_chunk<true>(g, m, u, c.n, c.c0, h) : momentum_chunk<false>(g, m, u, c.n, c.c0, h);
  block_sum_store(s, partial + blockIdx.x);
}

// One workgroup per tensor: its chunk partials go through LDS 256 at a time (coalesced loads) and lane 0 adds them
// in index order in double. norms[t] is torch's bf16 norm() scalar after clamp(min=eps), held as fp32.
__global__ __launch_bounds__(256) void muon_norm_kernel(const float* __restrict__ partial,
                                                        const int64_t* __restrict__ chunk_start, float eps,
                                                        float* __restrict__ norms) {
  __shared__ float sh[256];
  const int64_t b = chunk_start[blockIdx.x], e = chunk_start[blockIdx.x + 1];
  double a = 0.0;
  for (int64_t base = b; base < e; base += 256) {
    const int64_t i = base + threadIdx.x;
    sh[threadIdx.x] = i < e ? partial[i] : 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int cnt = (int)min((int64_t)256, e - base);
      for (int k = 0; k < cnt; ++k) a += (double)sh[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) norms[blockIdx.x] = fmaxf(bf2f(f2bf((float)sqrt(a))), eps);
}

PICO_DEV void normalize_chunk(bf16_t* u, int64_t n, int64_t c0, float nrm) {
  const int64_t end = min(n, c0 + OPT_CHUNK);
  if ((((uintptr_t)u & 15) == 0) && (n % 8 == 0)) {
    for (int64_t i = c0 + 8 * (int64_t)threadIdx.x; i < end; i += 8 * 256) {
      u16x8 v = *reinterpret_cast<const u16x8*>(u + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = f2bf(bf2f(v[j]) / nrm);
      *reinterpret_cast<u16x8*>(u + i) = v;
    }
  } else {
    for (int64_t i = c0 + threadIdx.x; i < end; i += 256) u[i] = f2bf(bf2f(u[i]) / nrm);
  }
}

__global__ __launch_bounds__(256) void muon_normalize_kernel(const int64_t* __restrict__ tensors,
                                                             const int64_t* __restrict__ sizes,
                                                             const int64_t* __restrict__ chunks,
                                                             const float* __restrict__ norms) {
  const OptChunk c = opt_chunk(tensors, sizes, chunks);
  normalize_chunk((bf16_t*)c.t[3], c.n, c.c0, norms[c.ti]);
}

PICO_DEV unsigned short update_elem(unsigned short p, unsigned short o, float decay, float alpha) {
  const float pf = bf2f(f2bf(bf2f(p) * decay));  // mul_: its own rounding
  return f2bf(pf + alpha * bf2f(o));
}

PICO_DEV void update_chunk(bf16_t* p, const bf16_t* o, int64_t n, int64_t c0, float decay, float alpha) {
  const int64_t end = min(n, c0 + OPT_CHUNK);
  if (((((uintptr_t)p | (uintptr_t)o) & 15) == 0) && (n % 8 == 0)) {
    for (int64_t i = c0 + 8 * (int64_t)threadIdx.x; i < end; i += 8 * 256) {
      u16x8 pv = *reinterpret_cast<const u16x8*>(p + i);
      const u16x8 ov = *reinterpret_cast<const u16x8*>(o + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) pv[j] = update_elem(pv[j], ov[j], decay, alpha);
      *reinterpret_cast<u16x8*>(p + i) = pv;
    }
  } else {
    for (int64_t i = c0 + threadIdx.x; i < end; i += 256) p[i] = update_elem(p[i], o[i], decay, alpha);
  }
}

// out_ptrs: [n_tensors], the address of each tensor's orthogonalised update O (contiguous, the parameter's shape);
// ratios: [n_tensors] double, torch's _adjust_lr ratio. alpha = (float)(-(lr * ratio)), formed in double.
__global__ __launch_bounds__(256) void muon_update_kernel(const int64_t* __restrict__ tensors,
                                                          const int64_t* __restrict__ out_ptrs,
                                                          const int64_t* __restrict__ sizes,
                                                          const int64_t* __restrict__ chunks, double lr, float decay,
                                                          const double* __restrict__ ratios) {
  const OptChunk c = opt_chunk(tensors, sizes, chunks);
  const float alpha = (float)(-(lr * ratios[c.ti]));
  update_chunk((bf16_t*)c.t[0], (const bf16_t*)out_ptrs[c.ti], c.n, c.c0, decay, alpha);
}

}  // namespace

extern "C" int pico_muon_momentum(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks,
                                  int64_t n_chunks, double momentum, int nesterov, float* partials, void* stream) {
  PICO_REQUIRE(n_chunks >= 0 && n_chunks < (1ll << 31), "pico_muon_momentum: bad chunk count");
  PICO_REQUIRE(momentum >= 0.0, "pico_muon_momentum: momentum must be >= 0 (got %g)", momentum);  // NaN fails too
  if (n_chunks == 0) return 0;
  PICO_REQUIRE(tensors && sizes && chunks, "pico_muon_momentum: null table");
  PICO_REQUIRE(partials, "pico_muon_momentum: null partials");
  const MuonMom h{(float)(1.0 - momentum), (float)momentum, nesterov ? 1 : 0};
  PICO_TRY(pico_launch(PICO_K_ADAMW, "muon_momentum", muon_momentum_kernel, dim3((int)n_chunks), dim3(256), 0,
                       (hipStream_t)stream, tensors, sizes, chunks, h, partials));
  return 0;
}

extern "C" int pico_muon_normalize(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks,
                                   int64_t n_chunks, const int64_t* chunk_start, int64_t n_tensors,
                                   const float* partials, double eps, float* norms, void* stream) {
  PICO_REQUIRE(n_chunks >= 0 && n_chunks < (1ll << 31), "pico_muon_normalize: bad chunk count");
  PICO_REQUIRE(eps >= 0.0, "pico_muon_normalize: eps must be >= 0 (got %g)", eps);
  if (n_chunks == 0) return 0;
  PICO_REQUIRE(n_tensors >= 1 && n_tensors < (1ll << 31), "pico_muon_normalize: bad tensor count");
  PICO_REQUIRE(tensors && sizes && chunks && chunk_start, "pico_muon_normalize: null table");
  PICO_REQUIRE(partials && norms, "pico_muon_normalize: null partials / norms");
  hipStream_t s = (hipStream_t)stream;
  // not timed: one small workgroup per tensor over its chunk partials
  PICO_TRY(pico_launch(0, "muon_norm", muon_norm_kernel, dim3((int)n_tensors), dim3(256), 0, s, partials, chunk_start,
                       (float)eps, norms));
  PICO_TRY(pico_launch(PICO_K_ADAMW, "muon_normalize", muon_normalize_kernel, dim3((int)n_chunks), dim3(256), 0, s,
                       tensors, sizes, chunks, (const float*)norms));
  return 0;
}

extern "C" int pico_muon_update(const int64_t* tensors, const int64_t* out_ptrs, const int64_t* sizes,
                                const int64_t* chunks, int64_t n_chunks, double lr, double weight_decay,
                                const double* ratios, void* stream) {
  PICO_REQUIRE(n_chunks >= 0 && n_chunks < (1ll << 31), "pico_muon_update: bad chunk count");
  PICO_REQUIRE(lr >= 0.0 && weight_decay >= 0.0, "pico_muon_update: lr and weight_decay must be >= 0 (got %g, %g)", lr,
               weight_decay);
  if (n_chunks == 0) return 0;
  PICO_REQUIRE(tensors && sizes && chunks, "pico_muon_update: null table");
  PICO_REQUIRE(out_ptrs && ratios, "pico_muon_update: null out_ptrs / ratios");
  PICO_TRY(pico_launch(PICO_K_ADAMW, "muon_update", muon_update_kernel, dim3((int)n_chunks), dim3(256), 0,
                       (hipStream_t)stream, tensors, out_ptrs, sizes, chunks, lr, (float)(1.0 - lr * weight_decay),
                       ratios));
  return 0;
}
