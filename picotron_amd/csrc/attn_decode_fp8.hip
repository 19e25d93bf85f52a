// Split-KV decode attention against an FP8 (OCP e4m3) KV cache.
//
// pico_attn_decode's contract (attn_decode.hip) with another cache format: k_cache / v_cache [B, Hkv, S_max, D] hold
// one e4m3 code per element (head-major, so one (row, kv head) is one contiguous stream of len * D bytes) and
// k_scale / v_scale [B, Hkv, S_max] one fp32 scale per cached head vector; element (.., s, d) has the value
// scale[.., s] * e4m3(code[.., s, d]). Both scales fold into the softmax exactly: the score of key s is
// (q . codes_k[s]) * (k_scale[s] * scale log2 e), the V scale multiplies p before the PV accumulation, and l sums
// the unscaled p.
//
// What is the bf16 kernel's: one workgroup of 4 waves serves all G = Hq / Hkv (<= 8) query heads of a kv head over
// one chunk of split_keys keys (the same DecodePlan: the grid is the bf16 kernel's and each workgroup streams half
// the bytes); a lane group keeps its own online softmax (m, l, O slice) per head in fp32; the groups are merged
// across a wave with lane shuffles and across the waves through LDS; an fp32 partial per chunk, combined in chunk
// order by a second kernel; no atomics, no waiting. A lane whose row is past the chunk's live end loads the last
// live row AND THAT ROW'S SCALES and its score becomes -inf, so stale codes (0x7f / 0xff are NaN) and stale or NaN
// scales beyond the length never reach the result, and no address leaves [0, S_max).
//
// What is new is how K / V reach the registers. The lane decomposition stays LPK = D / 8 lanes per key row, 8 dims
// per lane, so q and the G x 8 accumulators cost the registers they cost there; a lane's piece of a row is 8 bytes,
// a wave load covers 512 contiguous bytes = 64 / LPK rows, and the row's two scales are 4-byte loads of one address
// per lane group. A trip issues U rows of K, V and both scales per lane before the first use (U = 8: 128 bytes of
// codes in flight per lane, the bf16 kernel's amount; dec8_unroll gives the U of each G), then consumes them four
// rows at a time (two at G = 5), each an online-softmax update of the bf16 kernel's shape, so the score and V
// registers live are those of one update whatever U is. v_cvt_pk_f32_fp8 converts two codes to fp32 exactly; every
// product q x code and p' x code is a plain fp32 FMA.
#include "attn_decode_plan.h"
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr float NEG_INF = -__builtin_huge_valf();
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
// Per G: the rows of K and of V in flight per lane group (U), the rows per online-softmax update, and the waves per
// SIMD the instance is held to, which is the bf16 instance's occupancy. U = 8 wherever that bound leaves no scratch;
// G = 2 and G = 5 spill there and take U = 4, G = 5 with updates of two rows (DESIGN.md 4v lists the registers).
constexpr int dec8_unroll(int g) { return g == 2 || g == 5 ? 4 : 8; }
constexpr int dec8_step(int g) { return g == 5 ? 2 : 4; }
constexpr int dec8_waves(int g) { return g == 1 ? 7 : g == 2 ? 5 : g == 3 ? 4 : g <= 5 ? 3 : 2; }

// sum over the LPK (8 or 16) adjacent lanes that hold one key row, result in each of them (DPP: xor 1, xor 2,
// row_half_mirror, row_mirror)
template <int LPK>
PICO_DEV float row_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));
  if constexpr (LPK == 16)
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));
  return v;
}

PICO_DEV float ex2(float x) { return __builtin_amdgcn_exp2f(x); }  // exp2(-inf) = 0
PICO_DEV float finite_or_zero(float m) { return m == NEG_INF ? 0.f : m; }

// 8 e4m3 codes (two dwords, ascending) -> fp32, exactly
PICO_DEV void cvt8(const u32x2& c, float* f) {
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[d], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[d], true);
    f[4 * d] = lo[0], f[4 * d + 1] = lo[1], f[4 * d + 2] = hi[0], f[4 * d + 3] = hi[1];
  }
}

struct Dec8Params {
  const bf16_t* q;
  const uint8_t* kc;
  const uint8_t* vc;
  const float* ksc;
  const float* vsc;
  const int* seqlens;
  float* pm;
  float* pl;
  float* po;
  int64_t qs0, qs1;
  int64_t ks[3], vs[3], kss[3], vss[3];
  int s_max, split_keys, nsplit;
  float scale_log2;
};

template <int D, int G>
__global__ __launch_bounds__(DEC_THREADS, dec8_waves(G)) void attn_decode_fp8_kernel(const Dec8Params a) {
  constexpr int LPK = D / 8;     // lanes per key row
  constexpr int KPW = 64 / LPK;  // key rows per wave load
  constexpr int NG = 4 * KPW;    // lane groups per workgroup
  constexpr int U = dec8_unroll(G), STEP = dec8_step(G);
  static_assert(U % STEP == 0, "a trip is whole updates");
  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int dl = (lane % LPK) * 8;         // this lane's 8 dims of the row
  const int gi = wave * KPW + lane / LPK;  // this lane's group among the NG
  const int nsplit = a.nsplit;
  const int hq_total = gridDim.y * G;
  const int64_t pbase = ((int64_t)b * hq_total + (int64_t)hk * G) * nsplit + split;  // + g * nsplit for head g

  int len = a.seqlens[b];
  len = len < 0 ? 0 : (len > a.s_max ? a.s_max : len);
  const int c0 = split * a.split_keys;  // < s_max (the grid has ceil(s_max / split_keys) chunks)
  const int end = min(c0 + a.split_keys, len);
  if (c0 >= end) {  // nothing of this chunk is live (uniform over the workgroup)
    if (tid < G) {
      a.pm[pbase + (int64_t)tid * nsplit] = NEG_INF;
      a.pl[pbase + (int64_t)tid * nsplit] = 0.f;
    }
    return;
  }

  float qf[G][8], m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const u16x8 qv = *reinterpret_cast<const u16x8*>(a.q + (int64_t)b * a.qs0 + (int64_t)(hk * G + g) * a.qs1 + dl);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      qf[g][i] = bf2f(qv[i]);
      acc[g][i] = 0.f;
    }
    m[g] = NEG_INF;
    l[g] = 0.f;
  }
  const uint8_t* kb = a.kc + (int64_t)b * a.ks[0] + (int64_t)hk * a.ks[1] + dl;
  const uint8_t* vb = a.vc + (int64_t)b * a.vs[0] + (int64_t)hk * a.vs[1] + dl;
  const float* ksb = a.ksc + (int64_t)b * a.kss[0] + (int64_t)hk * a.kss[1];
  const float* vsb = a.vsc + (int64_t)b * a.vss[0] + (int64_t)hk * a.vss[1];
  const int64_t ks2 = a.ks[2], vs2 = a.vs[2], kss2 = a.kss[2], vss2 = a.vss[2];
  const float scale_log2 = a.scale_log2;

  for (int base = c0; base < end; base += NG * U) {
    u32x2 kr[U], vr[U];
    float ksr[U], vsr[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int key = base + j * NG + gi;
      const int row = key < end ? key : end - 1;  // c0 <= row < end <= s_max: codes and scales of a live row
      kr[j] = *reinterpret_cast<const u32x2*>(kb + (int64_t)row * ks2);
      vr[j] = *reinterpret_cast<const u32x2*>(vb + (int64_t)row * vs2);
      ksr[j] = ksb[(int64_t)row * kss2];
      vsr[j] = vsb[(int64_t)row * vss2];
    }
#pragma unroll
    for (int h = 0; h < U; h += STEP) {
      if (h && base + h * NG >= end) break;  // no lane group has a live row in this update (uniform)
      float s[STEP][G];
#pragma unroll
      for (int j = 0; j < STEP; ++j) {
        float kf[8];
        cvt8(kr[h + j], kf);
        const bool live = base + (h + j) * NG + gi < end;
        const float ksl = ksr[h + j] * scale_log2;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          float d = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) d = fmaf(qf[g][i], kf[i], d);
          d = row_sum<LPK>(d);
          s[j][g] = live ? d * ksl : NEG_INF;
        }
      }
      float vf[STEP][8];
#pragma unroll
      for (int j = 0; j < STEP; ++j) cvt8(vr[h + j], vf[j]);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float mn = m[g];
#pragma unroll
        for (int j = 0; j < STEP; ++j) mn = fmaxf(mn, s[j][g]);
        const float ms = finite_or_zero(mn);
        const float alpha = ex2(m[g] - ms);
        float p[STEP], ps = 0.f;
#pragma unroll
        for (int j = 0; j < STEP; ++j) {
          const float e = ex2(s[j][g] - ms);
          ps += e;
          p[j] = e * vsr[h + j];  // 0 * a live row's finite scale for a lane past the end
        }
        l[g] = l[g] * alpha + ps;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float o = acc[g][i] * alpha;
#pragma unroll
          for (int j = 0; j < STEP; ++j) o = fmaf(p[j], vf[j][i], o);
          acc[g][i] = o;
        }
        m[g] = mn;
      }
    }
  }

  // merge the KPW groups of a wave (lanes that differ in the bits above the row's)
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float mw = m[g];
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1) mw = fmaxf(mw, __shfl_xor(mw, off));
    const float sc = ex2(m[g] - finite_or_zero(mw));
    float lw = l[g] * sc;
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1) lw += __shfl_xor(lw, off);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float o = acc[g][i] * sc;
#pragma unroll
      for (int off = LPK; off < 64; off <<= 1) o += __shfl_xor(o, off);
      acc[g][i] = o;
    }
    m[g] = mw;
    l[g] = lw;
  }

  // merge the four waves through LDS and write the partial
  __shared__ float sm_m[4][G], sm_l[4][G];
  __shared__ float sm_o[4][G][D];
  if (lane < LPK) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int i = 0; i < 8; ++i) sm_o[wave][g][dl + i] = acc[g][i];
      if (lane == 0) {
        sm_m[wave][g] = m[g];
        sm_l[wave][g] = l[g];
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < G * D; idx += DEC_THREADS) {
    const int g = idx / D, d = idx % D;
    float mt = sm_m[0][g];
#pragma unroll
    for (int w = 1; w < 4; ++w) mt = fmaxf(mt, sm_m[w][g]);
    const float ms = finite_or_zero(mt);
    float o = 0.f, lt = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float sc = ex2(sm_m[w][g] - ms);
      o = fmaf(sm_o[w][g][d], sc, o);
      lt = fmaf(sm_l[w][g], sc, lt);
    }
    const int64_t p = pbase + (int64_t)g * nsplit;
    a.po[p * D + d] = o;
    if (d == 0) {
      a.pm[p] = mt;
      a.pl[p] = lt;
    }
  }
}

// one workgroup of D threads per (b, query head): O = sum_c o_c 2^(m_c - M) / sum_c l_c 2^(m_c - M), in chunk order
// (the bf16 kernel's combine: the partials have its layout and meaning)
template <int D>
__global__ __launch_bounds__(D) void attn_decode_fp8_combine_kernel(const float* __restrict__ pm,
                                                                    const float* __restrict__ pl,
                                                                    const float* __restrict__ po,
                                                                    bf16_t* __restrict__ o, float* __restrict__ lse,
                                                                    int nsplit) {
  const int64_t row = blockIdx.x;
  const int d = threadIdx.x;
  const float* rm = pm + row * nsplit;
  const float* rl = pl + row * nsplit;
  float mt = NEG_INF;
#pragma unroll 8
  for (int c = 0; c < nsplit; ++c) mt = fmaxf(mt, rm[c]);
  float acc = 0.f, lt = 0.f;
  // branch-free: an empty chunk (m = -inf) never wrote its o; what the workspace holds there is selected away
#pragma unroll 8
  for (int c = 0; c < nsplit; ++c) {
    const float mc = rm[c];
    const bool empty = mc == NEG_INF;
    const float sc = empty ? 0.f : ex2(mc - mt);
    const float oc = po[(row * nsplit + c) * D + d];
    lt = fmaf(rl[c], sc, lt);
    acc = fmaf(empty ? 0.f : oc, sc, acc);
  }
  const bool any = lt > 0.f;
  o[row * D + d] = f2bf(any ? acc / lt : 0.f);
  if (d == 0) lse[row] = any ? fmaf(mt, LN2, __logf(lt)) : NEG_INF;
}

template <int D>
int launch_decode8(int group, dim3 grid, hipStream_t s, const Dec8Params& a) {
#define PICO_DEC8_CASE(GG)                                                                                          \
  case GG:                                                                                                          \
    return pico_launch(PICO_K_ATTN_FWD, "attn_decode_fp8", attn_decode_fp8_kernel<D, GG>, grid, dim3(DEC_THREADS), \
                       0, s, a)
  switch (group) {
    PICO_DEC8_CASE(1);
    PICO_DEC8_CASE(2);
    PICO_DEC8_CASE(3);
    PICO_DEC8_CASE(4);
    PICO_DEC8_CASE(5);
    PICO_DEC8_CASE(6);
    PICO_DEC8_CASE(7);
    PICO_DEC8_CASE(8);
  }
#undef PICO_DEC8_CASE
  return pico_set_error("pico_attn_decode_fp8: bad group %d", group);
}

}  // namespace

extern "C" int pico_attn_decode_fp8(const void* q, const int64_t* q_strides, const void* k_cache,
                                    const int64_t* k_strides, const float* k_scale, const int64_t* k_scale_strides,
                                    const void* v_cache, const int64_t* v_strides, const float* v_scale,
                                    const int64_t* v_scale_strides, const int32_t* seqlens, void* o, float* lse,
                                    void* workspace, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t s_max,
                                    int64_t head_dim, float softmax_scale, int64_t split_keys, void* stream) {
  PICO_REQUIRE(q && q_strides && k_cache && k_strides && k_scale && k_scale_strides && v_cache && v_strides &&
                   v_scale && v_scale_strides && seqlens && o && lse && workspace,
               "pico_attn_decode_fp8: null pointer");
  PICO_REQUIRE(head_dim == 64 || head_dim == 128, "pico_attn_decode_fp8: head_dim=%lld unsupported (64, 128)",
               (long long)head_dim);
  PICO_REQUIRE(batch >= 0 && batch <= 65535 && heads_kv > 0 && heads_kv <= 65535 && heads_q > 0,
               "pico_attn_decode_fp8: bad batch=%lld / heads_q=%lld / heads_kv=%lld", (long long)batch,
               (long long)heads_q, (long long)heads_kv);
  PICO_REQUIRE(heads_q % heads_kv == 0, "pico_attn_decode_fp8: heads_q=%lld is not a multiple of heads_kv=%lld",
               (long long)heads_q, (long long)heads_kv);
  PICO_REQUIRE(heads_q / heads_kv <= DEC_MAX_GROUP,
               "pico_attn_decode_fp8: %lld query heads per kv head; at most %d are supported",
               (long long)(heads_q / heads_kv), DEC_MAX_GROUP);
  PICO_REQUIRE(s_max > 0 && s_max <= (1 << 30), "pico_attn_decode_fp8: bad cache length %lld", (long long)s_max);
  PICO_REQUIRE(split_keys <= (1 << 30), "pico_attn_decode_fp8: bad split_keys %lld", (long long)split_keys);
  for (int d = 0; d < 3; ++d)
    PICO_REQUIRE(k_strides[d] % 8 == 0 && v_strides[d] % 8 == 0 && (d == 2 || q_strides[d] % 8 == 0),
                 "pico_attn_decode_fp8: q strides must be multiples of 8 elements, cache strides of 8 bytes");
  PICO_REQUIRE(((uintptr_t)q | (uintptr_t)o | (uintptr_t)workspace) % 16 == 0 &&
                   ((uintptr_t)k_cache | (uintptr_t)v_cache) % 8 == 0 &&
                   ((uintptr_t)k_scale | (uintptr_t)v_scale) % 4 == 0,
               "pico_attn_decode_fp8: q / o / workspace must be 16-byte, the caches 8-byte and the scales 4-byte "
               "aligned");
  if (batch == 0) return 0;
  const DecodePlan p = decode_plan(batch, heads_q, heads_kv, s_max, head_dim, split_keys, pico_num_cus());
  PICO_REQUIRE(p.nsplit <= 0x7fffffff / 2, "pico_attn_decode_fp8: too many chunks");
  char* ws = (char*)workspace;
  Dec8Params a{};
  a.q = (const bf16_t*)q, a.kc = (const uint8_t*)k_cache, a.vc = (const uint8_t*)v_cache;
  a.ksc = k_scale, a.vsc = v_scale, a.seqlens = seqlens;
  a.pm = (float*)(ws + p.m_off), a.pl = (float*)(ws + p.l_off), a.po = (float*)(ws + p.o_off);
  a.qs0 = q_strides[0], a.qs1 = q_strides[1];
  for (int d = 0; d < 3; ++d)
    a.ks[d] = k_strides[d], a.vs[d] = v_strides[d], a.kss[d] = k_scale_strides[d], a.vss[d] = v_scale_strides[d];
  a.s_max = (int)s_max, a.split_keys = (int)p.split_keys, a.nsplit = (int)p.nsplit;
  a.scale_log2 = softmax_scale * LOG2E;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)p.nsplit, (unsigned)heads_kv, (unsigned)batch);
  const int group = (int)(heads_q / heads_kv);
  if (head_dim == 64) {
    PICO_TRY(launch_decode8<64>(group, grid, s, a));
    PICO_TRY(pico_launch(PICO_K_ATTN_MERGE, "attn_decode_fp8_combine", attn_decode_fp8_combine_kernel<64>,
                         dim3((unsigned)(batch * heads_q)), dim3(64), 0, s, a.pm, a.pl, a.po, (bf16_t*)o, lse,
                         (int)p.nsplit));
  } else {
    PICO_TRY(launch_decode8<128>(group, grid, s, a));
    PICO_TRY(pico_launch(PICO_K_ATTN_MERGE, "attn_decode_fp8_combine", attn_decode_fp8_combine_kernel<128>,
                         dim3((unsigned)(batch * heads_q)), dim3(128), 0, s, a.pm, a.pl, a.po, (bf16_t*)o, lse,
                         (int)p.nsplit));
  }
  return 0;
}
