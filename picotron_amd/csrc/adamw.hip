// AdamW step for gfx950 over every parameter of a model in ONE launch (HBM-bound).
//
// Replaces torch.optim.AdamW(model.parameters(), lr, fused=True).step() (ref train.py:13,204-209,235):
// ATen's fused AdamW walks the parameter list in multi_tensor_apply chunks (~60 launches per
// SmolLM-1.7B step at ~3.4 TB/s). Here a device table describes the tensors once (param, grad,
// exp_avg, exp_avg_sq pointers and sizes, all in the parameter dtype as torch keeps them), a chunk
// table maps workgroups to 64 Ki-element ranges, and each lane streams 8-element vectors.
// Per element, with ATen's fused AdamW expression types and order (fp32 values, double hyper-parameters,
// so the weight-decay and moment updates evaluate in double and round once to fp32; decoupled decay first):
//   p -= lr * wd * p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;
//   p -= (float)(lr / bc1) * m / (float)(sqrt(v) / sqrt(bc2) + eps),  bc_i = 1 - b_i^step (host, double).
// Bytes per element: 8 read (p, g, m, v) + 6 written (p, m, v) for bf16 (10 read with an fp32 main_grad).
// pico_adamw_master keeps an fp32 master copy of each parameter and fp32 moments: 28 bytes per element.
//
// One kernel template covers the six forms: where p, m, v live is a state policy (Bf16State<SR>, MasterState),
// everything else (chunk bounds, vector / scalar choice, gradient load, clip, adam_elem) is adamw_chunk's.
#include "optim_common.h"

#include <type_traits>

namespace {

constexpr int CHUNK = OPT_CHUNK;  // elements per workgroup

struct AdamHyper {
  double lr_wd, b1, b2, eps, bc2_sqrt;
  float step_size;
};

PICO_DEV void adam_elem(float& p, float g, float& m, float& v, const AdamHyper& h) {
  p -= h.lr_wd * p;
  m = h.b1 * m + (1 - h.b1) * g;
  v = h.b2 * v + (1 - h.b2) * g * g;
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  p -= h.step_size * m / denom;
}

// A state policy holds the pointers of one tensor and gives adamw_chunk: vec_ok() (may 8 elements move with
// 16-byte accesses), load8 / store8 of a lane's 8 elements through its own register type Vec8 with get / put of
// element j in place, and load1 / store1 of one element. Each keeps the registers in the layout they are loaded in
// (handing the walker float[8] copies instead costs the master kernel its 6th wave: DESIGN.md §4k).
//
// p, m, v in bf16, as torch keeps the states of a bf16 parameter. SR: the three stores round stochastically
// (f2bf_sr, optim_common.h) instead of to nearest even; quantity 0, 1, 2 = parameter, exp_avg, exp_avg_sq. The
// vector path draws the 8 elements' bits with one Philox call per quantity; the scalar path evaluates the same
// calls and takes its lane, so both paths store the same bits. id: the generator's tensor id.
template <bool SR>
struct Bf16State {
  bf16_t *p, *m, *v;
  SrKey sr;
  uint32_t id;
  typedef uint32_t Words[4];  // SR only: the random bits of the 8 elements around an index, for one quantity
  struct Vec8 {
    u16x8 p, m, v;
    Words wp, wm, wv;
  };

  PICO_DEV Bf16State(const int64_t* t, const int64_t* ids, int64_t ti, const SrKey& key)
      : p((bf16_t*)t[0]), m((bf16_t*)t[2]), v((bf16_t*)t[3]), sr(key), id(SR ? (uint32_t)ids[ti] : 0) {}

  PICO_DEV bool vec_ok() const { return (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0; }

  PICO_DEV void draw(int64_t i, Words& wp, Words& wm, Words& wv) const {
    if constexpr (SR) {
      sr_words(sr, id, i, 0, wp);
      sr_words(sr, id, i, 1, wm);
      sr_words(sr, id, i, 2, wv);
    }
  }
  PICO_DEV static unsigned short round(float x, const Words& w, int j) {
    if constexpr (SR) return f2bf_sr(__float_as_uint(x), sr_lane(w, j));
    else return f2bf(x);
  }
  PICO_DEV void load8(int64_t i, Vec8& r) const {
    r.p = *reinterpret_cast<const u16x8*>(p + i);
    r.m = *reinterpret_cast<const u16x8*>(m + i);
    r.v = *reinterpret_cast<const u16x8*>(v + i);
    draw(i, r.wp, r.wm, r.wv);
  }
  PICO_DEV void get(const Vec8& r, int j, float& pf, float& mf, float& vf) const {
    pf = bf2f(r.p[j]);
    mf = bf2f(r.m[j]);
    vf = bf2f(r.v[j]);
  }
  PICO_DEV void put(Vec8& r, int j, float pf, float mf, float vf) const {
    r.p[j] = round(pf, r.wp, j);
    r.m[j] = round(mf, r.wm, j);
    r.v[j] = round(vf, r.wv, j);
  }
  PICO_DEV void store8(int64_t i, const Vec8& r) const {
    *reinterpret_cast<u16x8*>(p + i) = r.p;
    *reinterpret_cast<u16x8*>(m + i) = r.m;
    *reinterpret_cast<u16x8*>(v + i) = r.v;
  }
  PICO_DEV void load1(int64_t i, float& pf, float& mf, float& vf) const {
    pf = bf2f(p[i]);
    mf = bf2f(m[i]);
    vf = bf2f(v[i]);
  }
  PICO_DEV void store1(int64_t i, float pf, float mf, float vf) const {
    Words wp, wm, wv;
    draw(i, wp, wm, wv);
    const int j = (int)(i & 7);
    p[i] = round(pf, wp, j);
    m[i] = round(mf, wm, j);
    v[i] = round(vf, wv, j);
  }
};

// fp32 master weights and fp32 moments under the bf16 model parameter (pico_adamw_master): adam_elem runs on the
// fp32 master p32 and the fp32 m, v, which are stored as fp32: ATen's fused AdamW on fp32 tensors. The bf16 model
// parameter is bf16(p32), written and never read. Bytes per element: 14 read (p32, g, m, v) + 14 written (p32, m,
// v, p), 16 read with an fp32 main_grad. Vector path: two 16-byte accesses per fp32 operand and one per bf16
// operand (fp32 pointers 32-byte aligned, the rule of grad_vec_ok<true>).
struct MasterState {
  bf16_t* p;
  float *p32, *m, *v;
  struct Vec8 {
    f32x4 p[2], m[2], v[2];
    u16x8 pb;
  };

  PICO_DEV MasterState(const int64_t* t, const int64_t* masters, int64_t ti, const SrKey&)
      : p((bf16_t*)t[0]), p32((float*)masters[ti]), m((float*)t[2]), v((float*)t[3]) {}

  PICO_DEV bool vec_ok() const {
    return (((uintptr_t)p & 15) == 0) && ((((uintptr_t)p32 | (uintptr_t)m | (uintptr_t)v) & 31) == 0);
  }
  PICO_DEV void load8(int64_t i, Vec8& r) const {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      r.p[k] = reinterpret_cast<const f32x4*>(p32 + i)[k];
      r.m[k] = reinterpret_cast<const f32x4*>(m + i)[k];
      r.v[k] = reinterpret_cast<const f32x4*>(v + i)[k];
    }
  }
  PICO_DEV void get(const Vec8& r, int j, float& pf, float& mf, float& vf) const {
    pf = r.p[j / 4][j % 4];
    mf = r.m[j / 4][j % 4];
    vf = r.v[j / 4][j % 4];
  }
  PICO_DEV void put(Vec8& r, int j, float pf, float mf, float vf) const {
    r.p[j / 4][j % 4] = pf;
    r.m[j / 4][j % 4] = mf;
    r.v[j / 4][j % 4] = vf;
    r.pb[j] = f2bf(pf);
  }
  PICO_DEV void store8(int64_t i, const Vec8& r) const {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      reinterpret_cast<f32x4*>(p32 + i)[k] = r.p[k];
      reinterpret_cast<f32x4*>(m + i)[k] = r.m[k];
      reinterpret_cast<f32x4*>(v + i)[k] = r.v[k];
    }
    *reinterpret_cast<u16x8*>(p + i) = r.pb;
  }
  PICO_DEV void load1(int64_t i, float& pf, float& mf, float& vf) const {
    pf = p32[i];
    mf = m[i];
    vf = v[i];
  }
  PICO_DEV void store1(int64_t i, float pf, float mf, float vf) const {
    p32[i] = pf;
    m[i] = mf;
    v[i] = vf;
    p[i] = f2bf(pf);
  }
};

// One workgroup's chunk of one tensor. The gradient value is load_grad8 / load_grad1's (optim_common.h; the fp32
// main_grad form is grad_is_f32 = 1). CLIP: it is first scaled by the clip coefficient and rounded to bf16,
// g = bf16(g * coef): the value pico_grad_scale would have stored, so the step is bit-identical to scale-then-step
// without the gradient write and re-read (coef = 1: g unchanged, bit-identical to the plain step).
template <bool GF32, bool CLIP, class State>
PICO_DEV void adamw_chunk(const State& st, const void* g, int64_t n, int64_t c0, const AdamHyper& h, float coef) {
  const int64_t end = min(n, c0 + CHUNK);
  if (st.vec_ok() && grad_vec_ok<GF32>(g, n)) {
    for (int64_t i = c0 + 8 * (int64_t)threadIdx.x; i < end; i += 8 * 256) {
      typename State::Vec8 r;
      st.load8(i, r);
      float gf[8];
      load_grad8<GF32>(g, i, gf);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float pf, mf, vf;
        st.get(r, j, pf, mf, vf);
        if constexpr (CLIP) gf[j] = bf2f(f2bf(gf[j] * coef));
        adam_elem(pf, gf[j], mf, vf, h);
        st.put(r, j, pf, mf, vf);
      }
      st.store8(i, r);
    }
  } else {
    for (int64_t i = c0 + threadIdx.x; i < end; i += 256) {
      float pf, mf, vf;
      st.load1(i, pf, mf, vf);
      float gf = load_grad1<GF32>(g, i);
      if constexpr (CLIP) gf = bf2f(f2bf(gf * coef));
      adam_elem(pf, gf, mf, vf, h);
      st.store1(i, pf, mf, vf);
    }
  }
}

enum { FORM_BF16, FORM_SR, FORM_MASTER };

// sixth: the masters table (FORM_MASTER) or the generator's tensor ids (FORM_SR), [n_tensors]; unused, as sr is,
// by the other forms. CLIP: norm_coef is the device (gradient norm, clip coefficient) pair as pico_grad_clip_coef
// leaves it; a non-finite norm (an inf / NaN gradient somewhere in the list) skips the update: nothing is written.
template <int FORM, bool CLIP>
__global__ __launch_bounds__(256) void adamw_kernel(const int64_t* __restrict__ tensors,
                                                    const int64_t* __restrict__ sixth,
                                                    const int64_t* __restrict__ sizes,
                                                    const int64_t* __restrict__ chunks, AdamHyper h, SrKey sr,
                                                    const float* __restrict__ norm_coef) {
  float coef = 1.0f;
  if constexpr (CLIP) {
    const float norm = norm_coef[0];
    coef = norm_coef[1];
    if (!isfinite(norm)) return;
  }
  using State = std::conditional_t<FORM == FORM_MASTER, MasterState, Bf16State<FORM == FORM_SR>>;
  const OptChunk c = opt_chunk(tensors, sizes, chunks);
  const State st(c.t, sixth, c.ti, sr);
  const void* g = (const void*)c.t[1];
  if (c.t[4]) adamw_chunk<true, CLIP>(st, g, c.n, c.c0, h, coef);
  else adamw_chunk<false, CLIP>(st, g, c.n, c.c0, h, coef);
}

// pico_sr_round_bf16: the rounding alone. Aligned pointers: 8 elements per lane with one Philox call, then a scalar
// tail of n % 8 elements; otherwise every element on the scalar form of the same function.
__global__ __launch_bounds__(256) void sr_round_bf16_kernel(const uint32_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                            int64_t n, SrKey sr, uint32_t id, uint32_t quantity) {
  const bool vec = (((uintptr_t)src & 31) == 0) && (((uintptr_t)dst & 15) == 0);
  const int64_t n8 = vec ? (n & ~(int64_t)7) : 0;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
  for (int64_t i = 8 * tid; i < n8; i += 8 * nthr) {
    const u32x4 a = reinterpret_cast<const u32x4*>(src + i)[0], b = reinterpret_cast<const u32x4*>(src + i)[1];
    uint32_t w[4];
    sr_words(sr, id, i, quantity, w);
    u16x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = f2bf_sr(a[j], sr_lane(w, j));
      o[4 + j] = f2bf_sr(b[j], sr_lane(w, 4 + j));
    }
    *reinterpret_cast<u16x8*>(dst + i) = o;
  }
  for (int64_t i = n8 + tid; i < n; i += nthr) {
    uint32_t w[4];
    sr_words(sr, id, i, quantity, w);
    dst[i] = f2bf_sr(src[i], sr_lane(w, (int)(i & 7)));
  }
}

// The checks every step entry point opens with, then the host-side hyper-parameters: the bias corrections on the
// host in double, as ATen's fused AdamW takes them (then fp32 in the kernel). sr: the step is also a word of the
// generator's counter.
int adamw_prepare(const char* fn, bool sr, int64_t n_chunks, int64_t step, double lr, double beta1, double beta2,
                  double eps, double weight_decay, AdamHyper* h) {
  PICO_REQUIRE(n_chunks >= 0 && n_chunks < (1ll << 31), "%s: bad chunk count", fn);
  PICO_REQUIRE(step >= 1, "%s: step must be >= 1", fn);
  PICO_REQUIRE(!sr || step < (1ll << 32), "%s: step must be < 2^32 (the generator's counter word)", fn);
  PICO_REQUIRE(lr >= 0.0 && eps >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
               "%s: invalid hyper-parameters", fn);
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  h->lr_wd = (double)lr * (double)weight_decay;
  h->b1 = beta1;
  h->b2 = beta2;
  h->eps = eps;
  h->bc2_sqrt = sqrt(bc2);
  h->step_size = (float)((double)lr / bc1);
  return 0;
}

// One launch of a form, with the clip when norm_coef is not null. Timed under PICO_K_ADAMW.
template <int FORM>
int adamw_launch(const char* op, const char* op_clip, const int64_t* tensors, const int64_t* sixth,
                 const int64_t* sizes, const int64_t* chunks, int64_t n_chunks, const AdamHyper& h, const SrKey& sr,
                 const float* norm_coef, void* stream) {
  return pico_launch(PICO_K_ADAMW, norm_coef ? op_clip : op,
                     norm_coef ? adamw_kernel<FORM, true> : adamw_kernel<FORM, false>, dim3((int)n_chunks), dim3(256), 0,
                     (hipStream_t)stream, tensors, sixth, sizes, chunks, h, sr, norm_coef);
}

}  // namespace

extern "C" int64_t pico_adamw_chunk_elems(void) { return CHUNK; }

extern "C" int pico_adamw_bf16(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks, int64_t n_chunks,
                               double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                               void* stream) {
  AdamHyper h;
  PICO_TRY(adamw_prepare("pico_adamw_bf16", false, n_chunks, step, lr, beta1, beta2, eps, weight_decay, &h));
  if (n_chunks == 0) return 0;
  PICO_REQUIRE(tensors && sizes && chunks, "pico_adamw_bf16: null table");
  return adamw_launch<FORM_BF16>("adamw", "adamw_clip", tensors, nullptr, sizes, chunks, n_chunks, h, SrKey{}, nullptr,
                                 stream);
}

// pico_adamw_bf16 with the gradient clip folded in: plus the device (norm, coefficient) pair.
extern "C" int pico_adamw_bf16_clip(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks,
                                    int64_t n_chunks, double lr, double beta1, double beta2, double eps,
                                    double weight_decay, int64_t step, const float* norm_coef, void* stream) {
  AdamHyper h;
  PICO_TRY(adamw_prepare("pico_adamw_bf16_clip", false, n_chunks, step, lr, beta1, beta2, eps, weight_decay, &h));
  PICO_REQUIRE(norm_coef, "pico_adamw_bf16_clip: null norm_coef");
  if (n_chunks == 0) return 0;
  PICO_REQUIRE(tensors && sizes && chunks, "pico_adamw_bf16_clip: null table");
  return adamw_launch<FORM_BF16>("adamw", "adamw_clip", tensors, nullptr, sizes, chunks, n_chunks, h, SrKey{},
                                 norm_coef, stream);
}

// The step on fp32 master weights and fp32 moments: plus the masters table; norm_coef NULL: no clip.
extern "C" int pico_adamw_master(const int64_t* tensors, const int64_t* masters, const int64_t* sizes,
                                 const int64_t* chunks, int64_t n_chunks, double lr, double beta1, double beta2,
                                 double eps, double weight_decay, int64_t step, const float* norm_coef, void* stream) {
  AdamHyper h;
  PICO_TRY(adamw_prepare("pico_adamw_master", false, n_chunks, step, lr, beta1, beta2, eps, weight_decay, &h));
  if (n_chunks == 0) return 0;
  PICO_REQUIRE(tensors && sizes && chunks, "pico_adamw_master: null table");
  PICO_REQUIRE(masters, "pico_adamw_master: null masters table");
  return adamw_launch<FORM_MASTER>("adamw_master", "adamw_master_clip", tensors, masters, sizes, chunks, n_chunks, h,
                                   SrKey{}, norm_coef, stream);
}

// The bf16 step with stochastic rounding of the parameter and both moments: plus the ids table and the seed;
// norm_coef NULL: no clip.
extern "C" int pico_adamw_bf16_sr(const int64_t* tensors, const int64_t* ids, const int64_t* sizes,
                                  const int64_t* chunks, int64_t n_chunks, double lr, double beta1, double beta2,
                                  double eps, double weight_decay, int64_t step, const float* norm_coef, uint64_t seed,
                                  void* stream) {
  AdamHyper h;
  PICO_TRY(adamw_prepare("pico_adamw_bf16_sr", true, n_chunks, step, lr, beta1, beta2, eps, weight_decay, &h));
  if (n_chunks == 0) return 0;
  PICO_REQUIRE(tensors && sizes && chunks, "pico_adamw_bf16_sr: null table");
  PICO_REQUIRE(ids, "pico_adamw_bf16_sr: null ids table");
  const SrKey sr{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step};
  return adamw_launch<FORM_SR>("adamw_sr", "adamw_sr_clip", tensors, ids, sizes, chunks, n_chunks, h, sr, norm_coef,
                               stream);
}

extern "C" int pico_sr_round_bf16(const float* src, void* dst, int64_t n, uint64_t seed, int64_t step, int64_t id,
                                  int quantity, void* stream) {
  PICO_REQUIRE(n >= 0 && n < (1ll << 35), "pico_sr_round_bf16: n must be in [0, 2^35)");
  PICO_REQUIRE(step >= 0 && step < (1ll << 32), "pico_sr_round_bf16: step must be in [0, 2^32)");
  PICO_REQUIRE(id >= 0 && id < (1ll << 32), "pico_sr_round_bf16: id must be in [0, 2^32)");
  PICO_REQUIRE(quantity >= 0 && quantity <= 2, "pico_sr_round_bf16: quantity must be 0, 1 or 2");
  if (n == 0) return 0;
  PICO_REQUIRE(src && dst, "pico_sr_round_bf16: null pointer");
  PICO_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 1) == 0, "pico_sr_round_bf16: misaligned pointer");
  const SrKey sr{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step};
  const int64_t blocks = (n + 2047) / 2048;  // 8 elements per lane; a grid-stride loop beyond 64 Ki workgroups
  hipStream_t s = (hipStream_t)stream;
  PICO_TRY(pico_launch(PICO_K_CAST, "sr_round_bf16", sr_round_bf16_kernel, dim3((int)(blocks < 65536 ? blocks : 65536)),
                       dim3(256), 0, s, (const uint32_t*)src, (bf16_t*)dst, n, sr, (uint32_t)id, (uint32_t)quantity));
  return 0;
}
