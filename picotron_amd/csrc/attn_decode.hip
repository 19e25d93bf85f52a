// Split-KV decode attention: one new query per sequence against a head-major KV cache.
//
// q [B, Hq, D] (strided rows), k_cache / v_cache [B, Hkv, S_max, D] (strided, unit last stride), seqlens int32 [B]
// on the device -> O [B, Hq, D] bf16, LSE [B, Hq] fp32 (natural log) of softmax(scale q K^T) V over keys
// [0, min(seqlens[b], S_max)).
//
// Memory-bound on the K / V read, so the shape of the kernel is the stream: a workgroup serves all G = Hq / Hkv
// (<= 8) query heads of one kv head over one chunk of split_keys keys, so K / V are read once per kv head. A key
// row is D / 8 lanes x 16 bytes; a wave load covers 64 / (D / 8) consecutive rows (1 KiB contiguous), straight to
// VGPRs, DEC_UNROLL rows of K and of V in flight per lane before the first use, no LDS on the way. Each lane group
// keeps its own online softmax (m, l, O slice) per head in fp32 over the rows it owns; the dot product's D / 8
// partial sums are added with DPP row operations (no LDS). The groups are merged once at the end: across a wave
// with lane shuffles, across the four waves through 16 KiB of LDS. The workgroup writes an fp32 partial (m, l, O)
// to the workspace and a second small kernel combines the chunks of a row. No workgroup waits for another one (no
// tickets, no atomics): the order of every sum is fixed by the shape and split_keys alone, so the result is
// deterministic and a row's result does not depend on the other rows of the batch.
//
// Rows at or beyond the length are never read: a lane whose row is past the end loads the chunk's last live row
// instead and its score is replaced by -inf (p = 0), so stale cache contents (NaN included) cannot reach the result
// and no address leaves [0, S_max). An empty chunk writes m = -inf, l = 0; every exp2(m - max) is taken against a
// maximum that is replaced by 0 when it is -inf, so no (-inf) - (-inf) is formed.
#include "attn_decode_plan.h"
#include "common.h"

namespace {

constexpr float NEG_INF = -__builtin_huge_valf();
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

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

template <int D, int G>
__global__ __launch_bounds__(DEC_THREADS) void attn_decode_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    const int* __restrict__ seqlens, float* __restrict__ pm, float* __restrict__ pl, float* __restrict__ po,
    int s_max, int split_keys, int nsplit, int64_t qs0, int64_t qs1, int64_t ks0, int64_t ks1, int64_t ks2,
    int64_t vs0, int64_t vs1, int64_t vs2, float scale_log2) {
  constexpr int LPK = D / 8;    // lanes per key row
  constexpr int KPW = 64 / LPK; // key rows per wave load
  constexpr int NG = 4 * KPW;   // lane groups per workgroup
  constexpr int U = DEC_UNROLL;
  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int dl = (lane % LPK) * 8;       // this lane's 8 dims of the row
  const int gi = wave * KPW + lane / LPK; // this lane's group among the NG
  const int hq_total = gridDim.y * G;
  const int64_t pbase = ((int64_t)b * hq_total + (int64_t)hk * G) * nsplit + split;  // + g * nsplit for head g

  int len = seqlens[b];
  len = len < 0 ? 0 : (len > s_max ? s_max : len);
  const int c0 = split * split_keys;  // < s_max (the grid has ceil(s_max / split_keys) chunks)
  const int end = min(c0 + split_keys, len);
  if (c0 >= end) {  // nothing of this chunk is live (uniform over the workgroup)
    if (tid < G) {
      pm[pbase + (int64_t)tid * nsplit] = NEG_INF;
      pl[pbase + (int64_t)tid * nsplit] = 0.f;
    }
    return;
  }

  float qf[G][8], m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const u16x8 qv = *reinterpret_cast<const u16x8*>(q + (int64_t)b * qs0 + (int64_t)(hk * G + g) * qs1 + dl);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      qf[g][i] = bf2f(qv[i]);
      acc[g][i] = 0.f;
    }
    m[g] = NEG_INF;
    l[g] = 0.f;
  }
  const bf16_t* kb = kc + (int64_t)b * ks0 + (int64_t)hk * ks1 + dl;
  const bf16_t* vb = vc + (int64_t)b * vs0 + (int64_t)hk * vs1 + dl;

  for (int base = c0; base < end; base += NG * U) {
    u16x8 kr[U], vr[U];
    bool live[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int key = base + j * NG + gi;
      live[j] = key < end;
      const int row = live[j] ? key : end - 1;  // c0 <= row < end <= s_max
      kr[j] = *reinterpret_cast<const u16x8*>(kb + (int64_t)row * ks2);
      vr[j] = *reinterpret_cast<const u16x8*>(vb + (int64_t)row * vs2);
    }
    float s[U][G];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      float kf[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) kf[i] = bf2f(kr[j][i]);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) d = fmaf(qf[g][i], kf[i], d);
        d = row_sum<LPK>(d);
        s[j][g] = live[j] ? d * scale_log2 : NEG_INF;
      }
    }
    float vf[U][8];
#pragma unroll
    for (int j = 0; j < U; ++j)
#pragma unroll
      for (int i = 0; i < 8; ++i) vf[j][i] = bf2f(vr[j][i]);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mn = m[g];
#pragma unroll
      for (int j = 0; j < U; ++j) mn = fmaxf(mn, s[j][g]);
      const float ms = finite_or_zero(mn);
      const float alpha = ex2(m[g] - ms);
      float p[U], ps = 0.f;
#pragma unroll
      for (int j = 0; j < U; ++j) {
        p[j] = ex2(s[j][g] - ms);
        ps += p[j];
      }
      l[g] = l[g] * alpha + ps;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float a = acc[g][i] * alpha;
#pragma unroll
        for (int j = 0; j < U; ++j) a = fmaf(p[j], vf[j][i], a);
        acc[g][i] = a;
      }
      m[g] = mn;
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
      float a = acc[g][i] * sc;
#pragma unroll
      for (int off = LPK; off < 64; off <<= 1) a += __shfl_xor(a, off);
      acc[g][i] = a;
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
    po[p * D + d] = o;
    if (d == 0) {
      pm[p] = mt;
      pl[p] = lt;
    }
  }
}

// one workgroup of D threads per (b, query head): O = sum_c o_c 2^(m_c - M) / sum_c l_c 2^(m_c - M), in chunk order
template <int D>
__global__ __launch_bounds__(D) void attn_decode_combine_kernel(const float* __restrict__ pm,
                                                                const float* __restrict__ pl,
                                                                const float* __restrict__ po, bf16_t* __restrict__ o,
                                                                float* __restrict__ lse, int nsplit) {
  const int64_t row = blockIdx.x;
  const int d = threadIdx.x;
  const float* rm = pm + row * nsplit;
  const float* rl = pl + row * nsplit;
  float mt = NEG_INF;
#pragma unroll 8
  for (int c = 0; c < nsplit; ++c) mt = fmaxf(mt, rm[c]);
  float acc = 0.f, lt = 0.f;
  // branch-free, so that the loads of several chunks are in flight together (the adds stay in chunk order). An
  // empty chunk (m = -inf) never wrote its o: whatever the workspace holds there is loaded and selected away,
  // with weight 0
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

int decode_check(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t s_max, int64_t head_dim,
                 int64_t split_keys) {
  PICO_REQUIRE(head_dim == 64 || head_dim == 128, "pico_attn_decode: head_dim=%lld unsupported (64, 128)",
               (long long)head_dim);
  PICO_REQUIRE(batch >= 0 && batch <= 65535 && heads_kv > 0 && heads_kv <= 65535 && heads_q > 0,
               "pico_attn_decode: bad batch=%lld / heads_q=%lld / heads_kv=%lld", (long long)batch, (long long)heads_q,
               (long long)heads_kv);
  PICO_REQUIRE(heads_q % heads_kv == 0, "pico_attn_decode: heads_q=%lld is not a multiple of heads_kv=%lld",
               (long long)heads_q, (long long)heads_kv);
  PICO_REQUIRE(heads_q / heads_kv <= DEC_MAX_GROUP,
               "pico_attn_decode: %lld query heads per kv head; at most %d are supported",
               (long long)(heads_q / heads_kv), DEC_MAX_GROUP);
  PICO_REQUIRE(s_max > 0 && s_max <= (1 << 30), "pico_attn_decode: bad cache length %lld", (long long)s_max);
  PICO_REQUIRE(split_keys <= (1 << 30), "pico_attn_decode: bad split_keys %lld", (long long)split_keys);
  return 0;
}

template <int D>
int launch_decode(int group, dim3 grid, hipStream_t s, const bf16_t* q, const bf16_t* kc, const bf16_t* vc,
                  const int* seqlens, float* pm, float* pl, float* po, int s_max, int split_keys, int nsplit,
                  const int64_t* qs, const int64_t* ks, const int64_t* vs, float scale_log2) {
#define PICO_DEC_CASE(GG)                                                                                             \
  case GG:                                                                                                            \
    return pico_launch(PICO_K_ATTN_FWD, "attn_decode", attn_decode_kernel<D, GG>, grid, dim3(DEC_THREADS), 0, s, q,   \
                       kc, vc, seqlens, pm, pl, po, s_max, split_keys, nsplit, qs[0], qs[1], ks[0], ks[1], ks[2],     \
                       vs[0], vs[1], vs[2], scale_log2)
  switch (group) {
    PICO_DEC_CASE(1);
    PICO_DEC_CASE(2);
    PICO_DEC_CASE(3);
    PICO_DEC_CASE(4);
    PICO_DEC_CASE(5);
    PICO_DEC_CASE(6);
    PICO_DEC_CASE(7);
    PICO_DEC_CASE(8);
  }
#undef PICO_DEC_CASE
  return pico_set_error("pico_attn_decode: bad group %d", group);
}

}  // namespace

extern "C" int64_t pico_attn_decode_split_keys(int64_t batch, int64_t heads_kv, int64_t s_max, int64_t head_dim) {
  if (head_dim != 64 && head_dim != 128) return -1;
  return decode_default_split(batch, heads_kv, s_max, head_dim, pico_num_cus());
}

extern "C" int64_t pico_attn_decode_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t s_max,
                                                    int64_t head_dim, int64_t split_keys) {
  if (decode_check(batch, heads_q, heads_kv, s_max, head_dim, split_keys)) return -1;
  return decode_plan(batch, heads_q, heads_kv, s_max, head_dim, split_keys, pico_num_cus()).bytes;
}

extern "C" int pico_attn_decode(const void* q, const int64_t* q_strides, const void* k_cache,
                                const int64_t* k_strides, const void* v_cache, const int64_t* v_strides,
                                const int32_t* seqlens, void* o, float* lse, void* workspace, int64_t batch,
                                int64_t heads_q, int64_t heads_kv, int64_t s_max, int64_t head_dim,
                                float softmax_scale, int64_t split_keys, void* stream) {
  PICO_REQUIRE(q && q_strides && k_cache && k_strides && v_cache && v_strides && seqlens && o && lse && workspace,
               "pico_attn_decode: null pointer");
  PICO_TRY(decode_check(batch, heads_q, heads_kv, s_max, head_dim, split_keys));
  for (int d = 0; d < 3; ++d)
    PICO_REQUIRE(k_strides[d] % 8 == 0 && v_strides[d] % 8 == 0 && (d == 2 || q_strides[d] % 8 == 0),
                 "pico_attn_decode: strides must be multiples of 8 elements");
  PICO_REQUIRE(((uintptr_t)q | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)o | (uintptr_t)workspace) % 16 == 0,
               "pico_attn_decode: pointers must be 16-byte aligned");
  if (batch == 0) return 0;
  const DecodePlan p = decode_plan(batch, heads_q, heads_kv, s_max, head_dim, split_keys, pico_num_cus());
  PICO_REQUIRE(p.nsplit <= 0x7fffffff / 2, "pico_attn_decode: too many chunks");
  char* ws = (char*)workspace;
  float* pm = (float*)(ws + p.m_off);
  float* pl = (float*)(ws + p.l_off);
  float* po = (float*)(ws + p.o_off);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)p.nsplit, (unsigned)heads_kv, (unsigned)batch);
  const int group = (int)(heads_q / heads_kv);
  const float scale_log2 = softmax_scale * LOG2E;
  if (head_dim == 64) {
    PICO_TRY(launch_decode<64>(group, grid, s, (const bf16_t*)q, (const bf16_t*)k_cache, (const bf16_t*)v_cache,
                               seqlens, pm, pl, po, (int)s_max, (int)p.split_keys, (int)p.nsplit, q_strides, k_strides,
                               v_strides, scale_log2));
    PICO_TRY(pico_launch(PICO_K_ATTN_MERGE, "attn_decode_combine", attn_decode_combine_kernel<64>,
                         dim3((unsigned)(batch * heads_q)), dim3(64), 0, s, pm, pl, po, (bf16_t*)o, lse,
                         (int)p.nsplit));
  } else {
    PICO_TRY(launch_decode<128>(group, grid, s, (const bf16_t*)q, (const bf16_t*)k_cache, (const bf16_t*)v_cache,
                                seqlens, pm, pl, po, (int)s_max, (int)p.split_keys, (int)p.nsplit, q_strides,
                                k_strides, v_strides, scale_log2));
    PICO_TRY(pico_launch(PICO_K_ATTN_MERGE, "attn_decode_combine", attn_decode_combine_kernel<128>,
                         dim3((unsigned)(batch * heads_q)), dim3(128), 0, s, pm, pl, po, (bf16_t*)o, lse,
                         (int)p.nsplit));
  }
  return 0;
}
