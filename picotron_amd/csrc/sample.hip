// Fused next-token sampler for generation: temperature, top-k, top-p and the draw in one launch per decode step.
//
// One workgroup of 1024 lanes per row of logits [rows, vocab] (fp32 or bf16, row stride free, no alignment
// assumption). Everything a step needs lives on the device, so a captured launch replays with identical arguments:
// the settings are read from `params` at run time, the row's draw counter from `draws`, the EOS latch from `done`.
//
// Semantics per row, all in fp32, HF's warper order (temperature, top-k, top-p). A NaN logit counts as -inf, +inf as
// FLT_MAX, -0 as +0.
//   temperature <= 0 : tok = index of the maximum (lowest index on ties), kept = 1.
//   else z_i = (x_i - max x) / T, mass w_i = exp(z_i);
//     top-k : K = {i : x_i >= the k-th largest value} (ties at the threshold are all kept);
//     top-p : t = the largest value with mass{i in K : x_i >= t} >= p mass(K); kept = {i in K : x_i >= t};
//     draw  : w = philox4x32_10(row, n, 0, 0; seed), u = ((w[1] << 32) | w[0]) / 2^64; tok = the first kept index in
//             vocabulary order whose inclusive cumulative mass exceeds u mass(kept).
//   A row with no finite logit (all -inf / NaN) gives tok = 0, kept = 0. A row whose `done` flag is set gives
//   tok = pad, kept = 0. Either way the counter advances.
//
// The bits depend on the inputs only. Both thresholds come from a 4 x 8-bit radix select on the order-preserving
// integer image of the fp32 logit, with integer LDS bins: counts for top-k, and for top-p the masses as fixed point
// round(w_i 2^40) in uint64 (vocab <= 2^20 cannot overflow). Integer adds commute, so the order in which lanes reach a
// bin does not matter. The draw is an exact integer prefix scan in index order against mulhi64(r, total). No float
// reduction anywhere.
//
// The row is re-read from L2 by every pass (max; 4 per active threshold; kept mass per tile; the draw's tile). A lane
// owns groups of 4 consecutive elements, aligned to the vector load by a per-row offset; the groups at the two ends
// of a row are read element by element.
#include <float.h>

#include "optim_common.h"

namespace {

constexpr int SMP_THREADS = 1024;
constexpr int SMP_WAVES = SMP_THREADS / 64;
constexpr int SMP_E = 4;         // elements per group
constexpr int SMP_COPIES = 8;    // bin copies, by lane & 7: an 8-way instead of a 64-way collision on a hot bin
constexpr int SMP_MAX_TILES = 260;  // (2^20 + 3) / 4 groups in tiles of 1024, rounded up
constexpr int64_t SMP_MAX_VOCAB = 1 << 20;
constexpr uint32_t SMP_KEY_NINF = 0x007FFFFFu;  // smp_key(-inf): the smallest key there is

struct SampleParams {  // the `params` buffer: 8 words
  float temperature, top_p;
  int32_t top_k, eos, pad;
  uint32_t seed_lo, seed_hi, reserved;
};

PICO_DEV float smp_canon(float x) {
  if (x != x) return -INFINITY;
  if (x == 0.f) return 0.f;
  return fminf(x, FLT_MAX);
}

// order-preserving image of a canonical fp32 value
PICO_DEV uint32_t smp_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

PICO_DEV uint64_t smp_mass(float x, float xmax, float temperature) {
  const float w = expf(__fdiv_rn(x - xmax, temperature));
  return __float2ull_rn(w * 0x1p40f);
}

template <typename T>
struct SmpRow {
  const T* p;   // element 0 of the row
  int off;      // group g holds elements g * 4 - off .. + 3: (p - off) is aligned to a 4-element vector
  int vocab;
  int groups;
};

template <typename T>
PICO_DEV SmpRow<T> smp_row(const T* p, int vocab) {
  const int off = (int)(((uintptr_t)p / sizeof(T)) & (SMP_E - 1));
  return {p, off, vocab, (vocab + off + SMP_E - 1) / SMP_E};
}

// canonical values of group g; an element outside the row reads -inf with its bit clear in the returned mask
template <typename T>
PICO_DEV unsigned smp_load(const SmpRow<T>& r, int g, float (&x)[SMP_E]) {
  const int i0 = g * SMP_E - r.off;
  if (g >= r.groups) {
#pragma unroll
    for (int e = 0; e < SMP_E; ++e) x[e] = -INFINITY;
    return 0u;
  }
  if (i0 >= 0 && i0 + SMP_E <= r.vocab) {
    if constexpr (sizeof(T) == 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(r.p + i0);
#pragma unroll
      for (int e = 0; e < SMP_E; ++e) x[e] = smp_canon(v[e]);
    } else {
      const u16x4 v = *reinterpret_cast<const u16x4*>(r.p + i0);
#pragma unroll
      for (int e = 0; e < SMP_E; ++e) x[e] = smp_canon(bf2f(v[e]));
    }
    return 0xFu;
  }
  unsigned m = 0;
#pragma unroll
  for (int e = 0; e < SMP_E; ++e) {
    const int i = i0 + e;
    const bool ok = i >= 0 && i < r.vocab;
    float v = -INFINITY;
    if (ok) {
      if constexpr (sizeof(T) == 4) v = smp_canon(r.p[i]);
      else v = smp_canon(bf2f(r.p[i]));
      m |= 1u << e;
    }
    x[e] = v;
  }
  return m;
}

struct SmpShared {
  unsigned long long bins[SMP_COPIES * 256];
  unsigned long long tile[SMP_MAX_TILES];
  unsigned long long wave[SMP_WAVES];
  unsigned long long pick[3];  // a selection's winner, broadcast
};

PICO_DEV uint64_t smp_shfl_up(uint64_t v, int d) { return (uint64_t)__shfl_up((unsigned long long)v, d, 64); }
PICO_DEV uint64_t smp_shfl_xor(uint64_t v, int d) { return (uint64_t)__shfl_xor((unsigned long long)v, d, 64); }

PICO_DEV uint64_t smp_wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += smp_shfl_xor(v, d);
  return v;
}

// inclusive prefix sum over the 1024 lanes in lane order, *total = the sum of all; every lane calls
PICO_DEV uint64_t smp_block_scan(uint64_t v, SmpShared& sh, uint64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = smp_shfl_up(v, d);
    if (lane >= d) v += o;
  }
  __syncthreads();  // the previous readers of sh.wave are through
  if (lane == 63) sh.wave[wave] = v;
  __syncthreads();
  uint64_t base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < SMP_WAVES; ++i) {
    const uint64_t s = sh.wave[i];
    if (i < wave) base += s;
    tot += s;
  }
  *total = tot;
  return v + base;
}

// the maximum over the 1024 lanes, in every lane
PICO_DEV uint64_t smp_block_max(uint64_t v, SmpShared& sh) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint64_t o = smp_shfl_xor(v, d);
    v = o > v ? o : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh.wave[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t m = 0;
#pragma unroll
  for (int i = 0; i < SMP_WAVES; ++i) {
    const uint64_t s = sh.wave[i];
    m = s > m ? s : m;
  }
  return m;
}

// Radix select: the largest key t with weight{key >= t, key >= floor_key} >= target, where an element weighs 1
// (MASS false; target = `count`) or its fixed-point mass (MASS true; target = ceil(frac * the weight of all keys >=
// floor_key)). Needs 1 <= target <= the total weight, which the caller guarantees.
template <bool MASS, typename T>
PICO_DEV uint32_t smp_select(const SmpRow<T>& row, int tiles, SmpShared& sh, uint32_t floor_key, uint64_t count,
                             float frac, float xmax, float temperature) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
  uint64_t above = 0, target = count;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < SMP_COPIES * 256; i += SMP_THREADS) sh.bins[i] = 0;
    __syncthreads();
    unsigned long long* mine = sh.bins + (tid & (SMP_COPIES - 1)) * 256;
    for (int j = 0; j < tiles; ++j) {
      float x[SMP_E];
      const unsigned ok = smp_load(row, j * SMP_THREADS + tid, x);
#pragma unroll
      for (int e = 0; e < SMP_E; ++e) {
        const uint32_t key = smp_key(x[e]);
        const bool in = ((ok >> e) & 1u) && key >= floor_key && (pass == 0 || (key >> (shift + 8)) == prefix);
        if (in) {
          const unsigned long long w = MASS ? smp_mass(x[e], xmax, temperature) : 1ull;
          if (w) atomicAdd(mine + ((key >> shift) & 255u), w);
        }
      }
    }
    __syncthreads();
    // lane j < 256 owns digit 255 - j: the scan runs from the largest digit down
    uint64_t h = 0;
    if (tid < 256) {
#pragma unroll
      for (int c = 0; c < SMP_COPIES; ++c) h += sh.bins[c * 256 + 255 - tid];
    }
    uint64_t tot;
    const uint64_t inc = above + smp_block_scan(h, sh, &tot);
    if (MASS && pass == 0) {
      // the one place that leaves integers: tot (up to 2^60) and the product round in double, a relative 2^-52,
      // far below the fixed-point quantum's share; the same inputs still give the same target
      const double want = ceil((double)frac * (double)tot);
      target = want < 1.0 ? 1ull : (uint64_t)want;
    }
    if (pass == 0 && target > tot) target = tot;
    if (tid < 256 && inc >= target && inc - h < target) {
      sh.pick[0] = 255 - tid;
      sh.pick[1] = inc - h;
    }
    __syncthreads();
    prefix = (prefix << 8) | (uint32_t)sh.pick[0];
    above = sh.pick[1];
  }
  return prefix;
}

template <typename T>
__global__ __launch_bounds__(SMP_THREADS) void sample_kernel(const T* __restrict__ logits, int64_t row_stride,
                                                              int vocab, const SampleParams* __restrict__ params,
                                                              int* __restrict__ draws, uint8_t* __restrict__ done,
                                                              int64_t* __restrict__ tokens, int64_t* __restrict__ out,
                                                              int64_t out_stride, int64_t out_cols,
                                                              int* __restrict__ kept) {
  __shared__ SmpShared sh;
  const int b = blockIdx.x, tid = threadIdx.x;
  const SampleParams prm = *params;
  const int n = draws[b];
  const bool was_done = done != nullptr && done[b] != 0;
  int64_t tok = 0;
  int nkept = 0;

  if (was_done) {
    tok = prm.pad;
  } else {
    const SmpRow<T> row = smp_row(logits + (int64_t)b * row_stride, vocab);
    const int tiles = (row.groups + SMP_THREADS - 1) / SMP_THREADS;
    // ---- maximum and its lowest index: one integer maximum of (key, ~index)
    uint64_t best = 0;
    for (int j = 0; j < tiles; ++j) {
      float x[SMP_E];
      const int g = j * SMP_THREADS + tid;
      const unsigned ok = smp_load(row, g, x);
#pragma unroll
      for (int e = 0; e < SMP_E; ++e) {
        const uint32_t idx = (uint32_t)(g * SMP_E - row.off + e);
        const uint64_t c = ((uint64_t)smp_key(x[e]) << 32) | (uint32_t)~idx;
        if (((ok >> e) & 1u) && c > best) best = c;
      }
    }
    best = smp_block_max(best, sh);
    const uint32_t kmax = (uint32_t)(best >> 32);
    if (kmax <= SMP_KEY_NINF) {  // no finite logit
      tok = 0;
      nkept = 0;
    } else if (!(prm.temperature > 0.f)) {
      tok = (int64_t)(~(uint32_t)best);
      nkept = 1;
    } else {
      const float xmax = __uint_as_float(kmax & 0x80000000u ? kmax & 0x7FFFFFFFu : ~kmax);
      const float temp = prm.temperature;
      uint32_t thr = 0;
      if (prm.top_k > 0 && prm.top_k < vocab)
        thr = smp_select<false>(row, tiles, sh, 0u, (uint64_t)prm.top_k, 0.f, xmax, temp);
      if (prm.top_p > 0.f && prm.top_p < 1.f)
        thr = smp_select<true>(row, tiles, sh, thr, 0ull, prm.top_p, xmax, temp);
      // ---- mass of the kept set per tile of 1024 groups (index order), and its size
      for (int i = tid; i < SMP_MAX_TILES; i += SMP_THREADS) sh.tile[i] = 0;
      __syncthreads();
      uint64_t cnt = 0;
      for (int j = 0; j < tiles; ++j) {
        float x[SMP_E];
        const unsigned ok = smp_load(row, j * SMP_THREADS + tid, x);
        uint64_t m = 0;
#pragma unroll
        for (int e = 0; e < SMP_E; ++e) {
          if (((ok >> e) & 1u) && smp_key(x[e]) >= thr) {
            m += smp_mass(x[e], xmax, temp);
            ++cnt;
          }
        }
        m = smp_wave_sum(m);
        if ((tid & 63) == 0 && m) atomicAdd(&sh.tile[j], (unsigned long long)m);
      }
      __syncthreads();
      uint64_t total;
      smp_block_scan(cnt, sh, &total);
      nkept = (int)total;
      // ---- the draw: tile, then lane, then element
      uint32_t w[4];
      philox4x32_10((uint32_t)b, (uint32_t)n, 0u, 0u, prm.seed_lo, prm.seed_hi, w);
      const uint64_t r = ((uint64_t)w[1] << 32) | w[0];
      const uint64_t ht = tid < tiles ? (uint64_t)sh.tile[tid] : 0ull;
      const uint64_t it = smp_block_scan(ht, sh, &total);
      const uint64_t u = __umul64hi(r, total);  // floor(u * total) < total: the kept set holds the maximum, mass 2^40
      if (it > u && it - ht <= u) {
        sh.pick[0] = (unsigned long long)tid;
        sh.pick[1] = u - (it - ht);
      }
      __syncthreads();
      const int jt = (int)sh.pick[0];
      const uint64_t ut = sh.pick[1];
      float x[SMP_E];
      const int g = jt * SMP_THREADS + tid;
      const unsigned ok = smp_load(row, g, x);
      uint64_t m[SMP_E], s = 0;
#pragma unroll
      for (int e = 0; e < SMP_E; ++e) {
        m[e] = (((ok >> e) & 1u) && smp_key(x[e]) >= thr) ? smp_mass(x[e], xmax, temp) : 0ull;
        s += m[e];
      }
      const uint64_t il = smp_block_scan(s, sh, &total);
      if (il > ut && il - s <= ut) {
        uint64_t c = il - s;
        int pick = -1;
#pragma unroll
        for (int e = 0; e < SMP_E; ++e) {
          c += m[e];
          if (pick < 0 && c > ut) pick = e;
        }
        sh.pick[2] = (unsigned long long)(g * SMP_E - row.off + pick);
      }
      __syncthreads();
      tok = (int64_t)sh.pick[2];
    }
  }

  __syncthreads();  // every lane has read draws[b] and done[b]
  if (tid == 0) {
    tokens[b] = tok;
    if (out != nullptr && n >= 0 && n < out_cols) out[(int64_t)b * out_stride + n] = tok;
    if (done != nullptr && prm.eos >= 0 && tok == (int64_t)prm.eos) done[b] = 1;
    if (kept != nullptr) kept[b] = nkept;
    draws[b] = n + 1;
  }
}

}  // namespace

extern "C" int pico_sample(const void* logits, int dtype, int64_t row_stride, int64_t rows, int64_t vocab,
                           const void* params, int32_t* draws, uint8_t* done, int64_t* tokens, int64_t* out,
                           int64_t out_stride, int64_t out_cols, int32_t* kept, void* stream) {
  PICO_REQUIRE(dtype == PICO_SAMPLE_F32 || dtype == PICO_SAMPLE_BF16,
               "pico_sample: dtype code %d unsupported (0 fp32, 1 bf16)", dtype);
  PICO_REQUIRE(vocab >= 1 && vocab <= SMP_MAX_VOCAB, "pico_sample: vocab=%lld outside [1, 2^20]", (long long)vocab);
  PICO_REQUIRE(rows >= 0 && rows < (1 << 24), "pico_sample: bad rows=%lld", (long long)rows);
  PICO_REQUIRE(logits && params && draws && tokens, "pico_sample: null pointer (logits, params, draws, tokens)");
  PICO_REQUIRE(out == nullptr || out_cols >= 0, "pico_sample: bad out_cols=%lld", (long long)out_cols);
  PICO_REQUIRE(((uintptr_t)logits % (dtype == PICO_SAMPLE_F32 ? 4 : 2)) == 0 && (uintptr_t)params % 4 == 0,
               "pico_sample: logits / params must be aligned to their element size");
  if (rows == 0) return 0;
  const dim3 grid((unsigned)rows), block(SMP_THREADS);
  if (dtype == PICO_SAMPLE_F32) {
    PICO_TRY(pico_launch(PICO_K_CE_FWD, "sample", sample_kernel<float>, grid, block, 0, (hipStream_t)stream,
                         (const float*)logits, row_stride, (int)vocab, (const SampleParams*)params, draws, done,
                         tokens, out, out_stride, out_cols, kept));
  } else {
    PICO_TRY(pico_launch(PICO_K_CE_FWD, "sample", sample_kernel<bf16_t>, grid, block, 0, (hipStream_t)stream,
                         (const bf16_t*)logits, row_stride, (int)vocab, (const SampleParams*)params, draws, done,
                         tokens, out, out_stride, out_cols, kept));
  }
  return 0;
}
