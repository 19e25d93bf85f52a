// Multi-token extend attention: T <= 16 new queries per sequence against a head-major KV cache, split over the keys,
// on the matrix unit.
//
// q [B, T, Hq, D] (strided rows), k_cache / v_cache [B, Hkv, S_max, D] (strided, unit last stride), seqlens int32 [B]
// on the device = the keys the LAST of the T queries sees -> O [B, T, Hq, D] bf16, LSE [B, T, Hq] fp32 (natural log).
// Query t of row b attends to keys [0, clamp(seqlens[b] - (T - 1 - t), 0, S_max)).
//
// Work split. The T * G (G = Hq / Hkv) query rows of a kv head, row r = (t = r / G, g = r % G), are the n extent of
// v_mfma_f32_16x16x32_bf16: a workgroup (4 waves) serves NB = 1 or 2 blocks of 16 rows over one chunk of split_keys
// keys; grid = (chunk x query block, kv head, batch). Each wave owns every fourth 32-key step of the chunk and runs
// the whole pipeline on it by itself, so the key loop has no workgroup barrier:
//   scores  S^T[key][row] = K Q^T. K is the A operand straight from global memory: lane (c = lane & 15, h = lane >> 4)
//           loads the 16 bytes K[key0 + c][32 ks + 8 h ..], which is the operand as it stands (no LDS for K). Q^T is
//           the B operand, loaded once per workgroup into registers the same way (padding rows are zeros). Two 16-key
//           tiles leave lane (c, h) with the eight scores of row c for keys 4h..4h+3 and 16+4h..16+4h+3 of the step.
//   softmax online per row in the log2 domain; the step maximum of a row crosses the four h groups with
//           v_permlane16_swap + v_permlane32_swap; l stays a per-lane partial sum until the end.
//   P V     O^T[d][row] += V^T P^T. The PV product's k index is DEFINED as kk = 8 h + j <-> key 4h + j (j < 4),
//           16 + 4h + j - 4 (j >= 4), so a lane's eight p, rounded to bf16 once, are the B operand as they lie. V^T
//           with that row permutation comes from a wave-private, double-buffered, swizzled LDS image of the step's
//           32 x D V tile (16-byte global loads, 16-byte LDS stores) through two ds_read_b64_tr_b16 per 16 d.
// The next step's K / V loads are issued before the current step's MFMAs. At the end the four waves' (m, l, O^T) are
// merged by wave 0 in wave order through LDS (which reuses the V images), the fp32 partial goes to the workspace and
// a second kernel combines a row's chunks in chunk order. No atomics, no workgroup waits for another: every sum's
// order is fixed by the shape and split_keys, and a batch row's bits do not depend on the other rows.
//
// Masking. K / V rows at or beyond the chunk's live end min(c0 + split_keys, clamp(seqlens[b])) never enter an
// operand: those loads are redirected to the last live row and their scores replaced by -inf, so stale cache contents
// (NaN included) cannot reach an MFMA and no address leaves [0, S_max). Keys between a query's own limit and the live
// end are the later new tokens: live and finite, masked by score -inf (p = 0) only. Every exp2(m - max) is taken
// against a maximum that is replaced by 0 when it is -inf.
#include "attn_common.h"
#include "attn_extend_plan.h"

namespace {

constexpr float NEG_INF = -__builtin_huge_valf();

PICO_DEV float finite_or_zero(float m) { return m == NEG_INF ? 0.f : m; }

// combine over the four 16-lane groups (lanes c, c + 16, c + 32, c + 48), result in each of them
template <class F>
PICO_DEV float cross_h(float v, F f) {
  const auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = f(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
  const auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return f(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
}

// One wave step's loads: K as the score product's A operands (2 tiles x D / 32 slices), V row-major for the LDS image.
// A row at or beyond `end` is replaced by row end - 1 (c0 <= end - 1 < s_max).
template <int D>
PICO_DEV void load_step(const bf16_t* kb, const bf16_t* vb, int64_t ks2, int64_t vs2, int key0, int end, int lane,
                        u16x8 (&kr)[2][D / 32], u16x8 (&vr)[D / 16]) {
  const int c = lane & 15, h = lane >> 4;
#pragma unroll
  for (int tile = 0; tile < 2; ++tile) {
    const int key = key0 + 16 * tile + c;
    const bf16_t* p = kb + (int64_t)(key < end ? key : end - 1) * ks2 + 8 * h;
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) kr[tile][ks] = *reinterpret_cast<const u16x8*>(p + 32 * ks);
  }
#pragma unroll
  for (int i = 0; i < D / 16; ++i) {
    const int idx = i * 64 + lane, row = idx / (D / 8), chunk = idx % (D / 8);
    const int key = key0 + row;
    vr[i] = *reinterpret_cast<const u16x8*>(vb + (int64_t)(key < end ? key : end - 1) * vs2 + 8 * chunk);
  }
}

template <int D, int NB>
__global__ __launch_bounds__(EXT_THREADS) void attn_extend_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    const int* __restrict__ seqlens, float* __restrict__ pm, float* __restrict__ pl, float* __restrict__ po,
    int s_max, int split_keys, int nsplit, int qblocks, int tokens, int group, int64_t qs0, int64_t qs1, int64_t qs2,
    int64_t ks0, int64_t ks1, int64_t ks2, int64_t vs0, int64_t vs1, int64_t vs2, float scale_log2) {
  constexpr int KS = D / 32;           // k slices of the score product
  constexpr int DT = D / 16;           // 16-d tiles of O^T; also the V loads per lane and step
  constexpr int WROWS = 16 * NB;       // query rows of this workgroup
  constexpr int IMG = 32 * D * 2;      // bytes of one V image
  // 4 waves x 2 V images; after the key loop: o[3][WROWS][D], m[3][WROWS], l[3][WROWS] fp32 of waves 1..3
  __shared__ __attribute__((aligned(16))) char smem[4 * 2 * IMG];
  static_assert(3 * WROWS * (D + 2) * 4 <= 4 * 2 * IMG, "the merge fits the V images");

  const int split = blockIdx.x / qblocks, qb = blockIdx.x % qblocks, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 15, h = lane >> 4;
  const int rows = tokens * group;
  const int hq_total = gridDim.y * group;

  int len_raw = seqlens[b];  // clamp(len_raw - k, 0, s_max) for 0 <= k < 16 is the same after this clamp
  len_raw = len_raw < 0 ? 0 : (len_raw > s_max + EXT_MAX_TOKENS ? s_max + EXT_MAX_TOKENS : len_raw);
  const int len = min(len_raw, s_max);
  const int c0 = split * split_keys;  // < s_max
  const int end = min(c0 + split_keys, len);

  // this lane's query row of each block: validity, partial index, visible keys of this chunk
  bool valid[NB];
  int64_t pidx[NB];
  int vis[NB];  // keys below it are visible: min(the query's limit, end)
  int tq[NB], hq[NB];
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    const int r = qb * WROWS + 16 * blk + c;
    valid[blk] = r < rows;
    tq[blk] = valid[blk] ? r / group : 0;
    hq[blk] = hk * group + (valid[blk] ? r % group : 0);
    pidx[blk] = (((int64_t)b * tokens + tq[blk]) * hq_total + hq[blk]) * nsplit + split;
    const int lim = len_raw - (tokens - 1 - tq[blk]);
    vis[blk] = valid[blk] ? min(max(lim, 0), end) : 0;
  }

  if (c0 >= end) {  // nothing of this chunk is live (uniform over the workgroup): o stays unwritten
    if (wave == 0 && h == 0) {
#pragma unroll
      for (int blk = 0; blk < NB; ++blk)
        if (valid[blk]) {
          pm[pidx[blk]] = NEG_INF;
          pl[pidx[blk]] = 0.f;
        }
    }
    return;
  }

  bf16x8 qop[NB][KS];
  float m[NB], l[NB];
  f32x4 acc[NB][DT];
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    const bf16_t* qp = q + (int64_t)b * qs0 + (int64_t)tq[blk] * qs1 + (int64_t)hq[blk] * qs2 + 8 * h;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (valid[blk]) v = *reinterpret_cast<const u16x8*>(qp + 32 * ks);
      qop[blk][ks] = __builtin_bit_cast(bf16x8, v);
    }
    m[blk] = NEG_INF;
    l[blk] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[blk][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const bf16_t* kb = kc + (int64_t)b * ks0 + (int64_t)hk * ks1;
  const bf16_t* vb = vc + (int64_t)b * vs0 + (int64_t)hk * vs1;
  char* wimg = smem + wave * 2 * IMG;
  // transposed V read: the 16-lane group h addresses rows 4h + (i >> 2), columns 16 dt + 4 (i & 3) .. + 3 of the
  // image and gets rows 4h .. 4h + 3 of column 16 dt + i; the second read is 16 rows further (the swizzle repeats)
  const int trow = 4 * h + (c >> 2), tchunk = (c & 3) >> 1, tsub = (c & 1) * 8;

  u16x8 kr[2][KS], vr[DT];
  const int wkey0 = c0 + wave * EXT_STEP_KEYS;
  if (wkey0 < end) load_step<D>(kb, vb, ks2, vs2, wkey0, end, lane, kr, vr);
  int buf = 0;
  for (int key0 = wkey0; key0 < end; key0 += EXT_TRIP_KEYS, buf ^= 1) {
    char* img = wimg + buf * IMG;
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const int idx = i * 64 + lane;
      *reinterpret_cast<u16x8*>(img + lds_off<D>(idx / (D / 8), idx % (D / 8))) = vr[i];
    }
    bf16x8 ka[2][KS];
#pragma unroll
    for (int tile = 0; tile < 2; ++tile)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) ka[tile][ks] = __builtin_bit_cast(bf16x8, kr[tile][ks]);
    if (key0 + EXT_TRIP_KEYS < end) load_step<D>(kb, vb, ks2, vs2, key0 + EXT_TRIP_KEYS, end, lane, kr, vr);

    bf16x8 pop[NB];
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {
      float s[8];
#pragma unroll
      for (int tile = 0; tile < 2; ++tile) {
        f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) st = mfma16(ka[tile][ks], qop[blk][ks], st);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          s[4 * tile + j] = key0 + 16 * tile + 4 * h + j < vis[blk] ? st[j] * scale_log2 : NEG_INF;
      }
      float mx = s[0];
#pragma unroll
      for (int j = 1; j < 8; ++j) mx = fmaxf(mx, s[j]);
      mx = cross_h(mx, [](float a, float b_) { return fmaxf(a, b_); });
      const float mn = fmaxf(m[blk], mx);
      const float ms = finite_or_zero(mn);
      const float alpha = fast_exp2(m[blk] - ms);
      float p[8], ps = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        p[j] = fast_exp2(s[j] - ms);
        ps += p[j];
      }
      l[blk] = l[blk] * alpha + ps;
      m[blk] = mn;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[blk][dt][j] *= alpha;
      pop[blk] = pack_bf16x8(p);
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const bf16x8 vt = lds_read_tr_rows(img + lds_off<D>(trow, 2 * dt + tchunk) + tsub, 16 * D * 2);
#pragma unroll
      for (int blk = 0; blk < NB; ++blk) acc[blk][dt] = mfma16(vt, pop[blk], acc[blk][dt]);
    }
  }

  // a row's l over its four h groups (m is already common to them)
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) l[blk] = cross_h(l[blk], [](float a, float b_) { return a + b_; });

  // waves 1..3 hand (m, l, O^T) to wave 0 through LDS; wave 0 adds them in wave order and writes the partial
  float* sm_o = reinterpret_cast<float*>(smem);
  float* sm_m = sm_o + 3 * WROWS * D;
  float* sm_l = sm_m + 3 * WROWS;
  __syncthreads();  // every wave is done with its V images
  if (wave > 0) {
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {
      const int row = (wave - 1) * WROWS + 16 * blk + c;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(sm_o + row * D + 16 * dt + 4 * h) = acc[blk][dt];
      if (h == 0) {
        sm_m[row] = m[blk];
        sm_l[row] = l[blk];
      }
    }
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    float mw[3], mt = m[blk];
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      mw[w] = sm_m[w * WROWS + 16 * blk + c];
      mt = fmaxf(mt, mw[w]);
    }
    const float ms = finite_or_zero(mt);
    const float sc0 = fast_exp2(m[blk] - ms);
    float lt = l[blk] * sc0;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[blk][dt][j] *= sc0;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      const int row = w * WROWS + 16 * blk + c;
      const float sc = fast_exp2(mw[w] - ms);
      lt = fmaf(sm_l[row], sc, lt);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const f32x4 ow = *reinterpret_cast<const f32x4*>(sm_o + row * D + 16 * dt + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[blk][dt][j] = fmaf(ow[j], sc, acc[blk][dt][j]);
      }
    }
    if (valid[blk]) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(po + pidx[blk] * D + 16 * dt + 4 * h) = acc[blk][dt];
      if (h == 0) {
        pm[pidx[blk]] = mt;
        pl[pidx[blk]] = lt;
      }
    }
  }
}

// one workgroup of D threads per (b, t, query head): O = sum_c o_c 2^(m_c - M) / sum_c l_c 2^(m_c - M), in chunk
// order (the decode kernel's combine, kept here as a copy so that attn_decode.hip's object stays what it is)
template <int D>
__global__ __launch_bounds__(D) void attn_extend_combine_kernel(const float* __restrict__ pm,
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
  // branch-free; a chunk with m = -inf may never have written its o: it is loaded and selected away, with weight 0
#pragma unroll 8
  for (int c = 0; c < nsplit; ++c) {
    const float mc = rm[c];
    const bool empty = mc == NEG_INF;
    const float sc = empty ? 0.f : fast_exp2(mc - mt);
    const float oc = po[(row * nsplit + c) * D + d];
    lt = fmaf(rl[c], sc, lt);
    acc = fmaf(empty ? 0.f : oc, sc, acc);
  }
  const bool any = lt > 0.f;
  o[row * D + d] = f2bf(any ? acc / lt : 0.f);
  if (d == 0) lse[row] = any ? fmaf(mt, LN2, __logf(lt)) : NEG_INF;
}

int extend_check(int64_t batch, int64_t tokens, int64_t heads_q, int64_t heads_kv, int64_t s_max, int64_t head_dim,
                 int64_t split_keys) {
  PICO_REQUIRE(head_dim == 64 || head_dim == 128, "pico_attn_extend: head_dim=%lld unsupported (64, 128)",
               (long long)head_dim);
  PICO_REQUIRE(tokens >= 1 && tokens <= EXT_MAX_TOKENS, "pico_attn_extend: tokens=%lld; 1 to %d are supported",
               (long long)tokens, EXT_MAX_TOKENS);
  PICO_REQUIRE(batch >= 0 && batch <= 65535 && heads_kv > 0 && heads_kv <= 65535 && heads_q > 0,
               "pico_attn_extend: bad batch=%lld / heads_q=%lld / heads_kv=%lld", (long long)batch, (long long)heads_q,
               (long long)heads_kv);
  PICO_REQUIRE(heads_q % heads_kv == 0, "pico_attn_extend: heads_q=%lld is not a multiple of heads_kv=%lld",
               (long long)heads_q, (long long)heads_kv);
  PICO_REQUIRE(heads_q / heads_kv <= EXT_MAX_GROUP,
               "pico_attn_extend: %lld query heads per kv head; at most %d are supported",
               (long long)(heads_q / heads_kv), EXT_MAX_GROUP);
  PICO_REQUIRE(s_max > 0 && s_max <= (1 << 30), "pico_attn_extend: bad cache length %lld", (long long)s_max);
  PICO_REQUIRE(split_keys <= (1 << 30), "pico_attn_extend: bad split_keys %lld", (long long)split_keys);
  return 0;
}

template <int D, int NB>
int launch_extend(const ExtendPlan& p, hipStream_t s, const bf16_t* q, const bf16_t* kc, const bf16_t* vc,
                  const int* seqlens, float* pm, float* pl, float* po, bf16_t* o, float* lse, int64_t batch,
                  int64_t tokens, int64_t heads_q, int64_t heads_kv, int s_max, const int64_t* qs, const int64_t* ks,
                  const int64_t* vs, float scale_log2) {
  const dim3 grid((unsigned)(p.nsplit * p.qblocks), (unsigned)heads_kv, (unsigned)batch);
  PICO_TRY(pico_launch(PICO_K_ATTN_FWD, "attn_extend", attn_extend_kernel<D, NB>, grid, dim3(EXT_THREADS), 0, s, q,
                       kc, vc, seqlens, pm, pl, po, s_max, (int)p.split_keys, (int)p.nsplit, (int)p.qblocks,
                       (int)tokens, (int)(heads_q / heads_kv), qs[0], qs[1], qs[2], ks[0], ks[1], ks[2], vs[0], vs[1],
                       vs[2], scale_log2));
  return pico_launch(PICO_K_ATTN_MERGE, "attn_extend_combine", attn_extend_combine_kernel<D>,
                     dim3((unsigned)(batch * tokens * heads_q)), dim3(D), 0, s, pm, pl, po, o, lse, (int)p.nsplit);
}

}  // namespace

extern "C" int64_t pico_attn_extend_split_keys(int64_t batch, int64_t tokens, int64_t heads_q, int64_t heads_kv,
                                               int64_t s_max, int64_t head_dim) {
  if (extend_check(batch, tokens, heads_q, heads_kv, s_max, head_dim, 0)) return -1;
  return extend_default_split(batch, tokens, heads_q, heads_kv, s_max, pico_num_cus());
}

extern "C" int64_t pico_attn_extend_workspace_bytes(int64_t batch, int64_t tokens, int64_t heads_q, int64_t heads_kv,
                                                    int64_t s_max, int64_t head_dim, int64_t split_keys) {
  if (extend_check(batch, tokens, heads_q, heads_kv, s_max, head_dim, split_keys)) return -1;
  return extend_plan(batch, tokens, heads_q, heads_kv, s_max, head_dim, split_keys, pico_num_cus()).bytes;
}

extern "C" int pico_attn_extend(const void* q, const int64_t* q_strides, const void* k_cache,
                                const int64_t* k_strides, const void* v_cache, const int64_t* v_strides,
                                const int32_t* seqlens, void* o, float* lse, void* workspace, int64_t batch,
                                int64_t tokens, int64_t heads_q, int64_t heads_kv, int64_t s_max, int64_t head_dim,
                                float softmax_scale, int64_t split_keys, void* stream) {
  PICO_REQUIRE(q && q_strides && k_cache && k_strides && v_cache && v_strides && seqlens && o && lse && workspace,
               "pico_attn_extend: null pointer");
  PICO_TRY(extend_check(batch, tokens, heads_q, heads_kv, s_max, head_dim, split_keys));
  for (int d = 0; d < 3; ++d)
    PICO_REQUIRE(k_strides[d] % 8 == 0 && v_strides[d] % 8 == 0 && q_strides[d] % 8 == 0,
                 "pico_attn_extend: strides must be multiples of 8 elements");
  PICO_REQUIRE(((uintptr_t)q | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)o | (uintptr_t)workspace) % 16 == 0,
               "pico_attn_extend: pointers must be 16-byte aligned");
  if (batch == 0) return 0;
  const ExtendPlan p = extend_plan(batch, tokens, heads_q, heads_kv, s_max, head_dim, split_keys, pico_num_cus());
  PICO_REQUIRE(p.nsplit * p.qblocks <= 0x7fffffff / 2, "pico_attn_extend: too many chunks");
  char* ws = (char*)workspace;
  float* pm = (float*)(ws + p.m_off);
  float* pl = (float*)(ws + p.l_off);
  float* po = (float*)(ws + p.o_off);
  hipStream_t s = (hipStream_t)stream;
  const float scale_log2 = softmax_scale * LOG2E;
#define PICO_EXT_ARGS                                                                                                \
  p, s, (const bf16_t*)q, (const bf16_t*)k_cache, (const bf16_t*)v_cache, seqlens, pm, pl, po, (bf16_t*)o, lse, batch, \
      tokens, heads_q, heads_kv, (int)s_max, q_strides, k_strides, v_strides, scale_log2
  if (head_dim == 64) return p.blocks == 1 ? launch_extend<64, 1>(PICO_EXT_ARGS) : launch_extend<64, 2>(PICO_EXT_ARGS);
  return p.blocks == 1 ? launch_extend<128, 1>(PICO_EXT_ARGS) : launch_extend<128, 2>(PICO_EXT_ARGS);
#undef PICO_EXT_ARGS
}
