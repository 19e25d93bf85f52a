// Fused RoPE + quantising KV-cache append for an FP8 (OCP e4m3) cache.
//
// pico_kv_append's contract (kv_append.hip) with another cache format: k_cache / v_cache hold one e4m3 code per
// element, head-major [B, Hkv, S_max, D] bytes, and k_scale / v_scale [B, Hkv, S_max] hold one fp32 scale per cached
// head vector: element (.., s, d) has the value scale[.., s] * e4m3(code[.., s, d]). For token p = pos[b] + t: q is
// rotated in place; k is rotated, written back IN PLACE in qkv as bf16 (the prompt attention of a prefill reads it
// there), and the same bf16 values are quantised into the cache; v is quantised into the cache and stays untouched
// in qkv. A token with p outside [0, min(S_max, table rows)) is skipped whole: no q, no k, no codes, no scales.
//
// The rotation is rope_kernel's (rope.hip), rounding point for rounding point, and the thread decomposition
// kv_append_kernel's: one thread owns 8 consecutive rotary pairs (elements i..i+7 and i+D/2..) of one (b, t, head),
// so a head vector is owned by D / 16 adjacent lanes (4 or 8), aligned within a wave. The quantiser is
// pico_quantize_rows_fp8's arithmetic (decode_linear_fp8.hip) with the head vector as the row: the exact absmax as
// an integer maximum over the magnitudes' bits, reduced across the vector's lanes with DPP (quad_perm xor 1, xor 2,
// row_half_mirror; no LDS), scale = absmax / 448 (correctly rounded; a vector of zeros: 1), code = RNE to e4m3 of
// clamp(x / scale, -448, 448) by v_cvt_pk_fp8_f32. Every lane of the workgroup takes part in the reduction: the
// loop's trip count is the workgroup's, and the skips (beyond the tensor, p out of range) only mask loads and
// stores, so no DPP operand comes from an inactive lane.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

constexpr float E4M3_MAX = 448.f;

struct KVA8Params {
  bf16_t* qkv;
  const bf16_t* cosp;
  const bf16_t* sinp;
  const int* pos;
  uint8_t* kc;
  uint8_t* vc;
  float* ksc;
  float* vsc;
  int64_t total;
  int64_t xs0, xs1, cs;
  int64_t ks[3], vs[3], kss[3], vss[3];
  int heads_q, heads_kv, tokens, half, limit;
};

// the larger of the two magnitudes (bf16 bits without the sign) over the VECS adjacent lanes of a head vector
template <int VECS>
PICO_DEV unsigned vec_max(unsigned v) {
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));
  if constexpr (VECS == 8) v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));
  return v;
}

PICO_DEV unsigned top8(const u16x8& v) {
  unsigned t = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) t = max(t, (unsigned)(v[j] & 0x7fffu));
  return t;
}

// 8 bf16 -> 8 e4m3 codes of x / s, ascending
PICO_DEV u32x2 quant8(const u16x8& v, float s) {
  float q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) q[j] = fminf(fmaxf(__fdiv_rn(bf2f(v[j]), s), -E4M3_MAX), E4M3_MAX);
  u32x2 o;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    int pk = __builtin_amdgcn_cvt_pk_fp8_f32(q[4 * d], q[4 * d + 1], 0, false);
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(q[4 * d + 2], q[4 * d + 3], pk, true);
    o[d] = (unsigned)pk;
  }
  return o;
}

template <int VECS>
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(const KVA8Params a) {
  const int heads = a.heads_q + 2 * a.heads_kv;
  const int half = a.half;
  // the trip count is the same for every lane of the workgroup; a lane beyond the tensor idles through the trip
  for (int64_t t0 = (int64_t)blockIdx.x * 256; t0 < a.total; t0 += (int64_t)gridDim.x * 256) {
    const int64_t t = t0 + threadIdx.x;
    const bool inside = t < a.total;
    const int64_t tc = inside ? t : 0;
    const int vi = (int)(tc % VECS);
    const int64_t r0 = tc / VECS;
    const int hd = (int)(r0 % heads);
    const int64_t r1 = r0 / heads;
    const int tok = (int)(r1 % a.tokens);
    const int b = (int)(r1 / a.tokens);
    const int64_t p = (int64_t)a.pos[b] + tok;
    const bool ok = inside && p >= 0 && p < a.limit;  // limit = min(S_max, table rows); shared by a vector's lanes
    const int i = vi * 8;
    bf16_t* xp = a.qkv + (int64_t)b * a.xs0 + (int64_t)tok * a.xs1 + (int64_t)hd * (2 * half) + i;
    const bool is_v = hd >= a.heads_q + a.heads_kv;
    u16x8 o1 = {}, o2 = {};
    if (ok) {
      o1 = *reinterpret_cast<const u16x8*>(xp);
      o2 = *reinterpret_cast<const u16x8*>(xp + half);
      if (!is_v) {
        const u16x8 c = *reinterpret_cast<const u16x8*>(a.cosp + p * a.cs + i);
        const u16x8 sn = *reinterpret_cast<const u16x8*>(a.sinp + p * a.cs + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float x1 = bf2f(o1[j]), x2 = bf2f(o2[j]);
          const float cf = bf2f(c[j]), sf = bf2f(sn[j]);
          // rope_kernel's expression: products rounded before the sum (no FMA contraction)
          o1[j] = f2bf(__fmul_rn(x1, cf) - __fmul_rn(x2, sf));
          o2[j] = f2bf(__fmul_rn(x2, cf) + __fmul_rn(x1, sf));
        }
        *reinterpret_cast<u16x8*>(xp) = o1;  // q, and k: the rotated bf16 stays in qkv
        *reinterpret_cast<u16x8*>(xp + half) = o2;
      }
    }
    // every lane: the vector's absmax (zeros from the lanes that skip), before anything diverges on hd
    const unsigned top = vec_max<VECS>(max(top8(o1), top8(o2)));
    if (!ok || hd < a.heads_q) continue;
    const float s = top ? __fdiv_rn(bf2f((unsigned short)top), E4M3_MAX) : 1.f;
    const int hk = is_v ? hd - a.heads_q - a.heads_kv : hd - a.heads_q;
    const int64_t* cst = is_v ? a.vs : a.ks;
    const int64_t* sst = is_v ? a.vss : a.kss;
    uint8_t* op = (is_v ? a.vc : a.kc) + (int64_t)b * cst[0] + (int64_t)hk * cst[1] + p * cst[2] + i;
    *reinterpret_cast<u32x2*>(op) = quant8(o1, s);
    *reinterpret_cast<u32x2*>(op + half) = quant8(o2, s);
    if (vi == 0) (is_v ? a.vsc : a.ksc)[(int64_t)b * sst[0] + (int64_t)hk * sst[1] + p * sst[2]] = s;
  }
}

}  // namespace

extern "C" int pico_kv_append_fp8(void* qkv, int64_t batch_stride, int64_t token_stride, const void* cos,
                                  const void* sin, int64_t cs_stride, int64_t table_rows, const int32_t* pos,
                                  void* k_cache, const int64_t* k_strides, float* k_scale,
                                  const int64_t* k_scale_strides, void* v_cache, const int64_t* v_strides,
                                  float* v_scale, const int64_t* v_scale_strides, int64_t batch, int64_t tokens,
                                  int64_t heads_q, int64_t heads_kv, int64_t s_max, int64_t head_dim, void* stream) {
  PICO_REQUIRE(qkv && cos && sin && pos && k_cache && k_strides && k_scale && k_scale_strides && v_cache && v_strides &&
                   v_scale && v_scale_strides,
               "pico_kv_append_fp8: null pointer");
  PICO_REQUIRE(head_dim == 64 || head_dim == 128, "pico_kv_append_fp8: head_dim=%lld unsupported (64, 128)",
               (long long)head_dim);
  PICO_REQUIRE(batch >= 0 && tokens >= 0 && heads_q > 0 && heads_kv > 0 && heads_q + 2 * heads_kv < (1 << 20),
               "pico_kv_append_fp8: bad batch=%lld / tokens=%lld / heads_q=%lld / heads_kv=%lld", (long long)batch,
               (long long)tokens, (long long)heads_q, (long long)heads_kv);
  PICO_REQUIRE(heads_q % heads_kv == 0, "pico_kv_append_fp8: heads_q=%lld is not a multiple of heads_kv=%lld",
               (long long)heads_q, (long long)heads_kv);
  PICO_REQUIRE(s_max > 0 && s_max <= (1 << 30) && table_rows >= 0,
               "pico_kv_append_fp8: bad cache length %lld / table rows %lld", (long long)s_max, (long long)table_rows);
  PICO_REQUIRE(batch_stride % 8 == 0 && token_stride % 8 == 0 && token_stride >= (heads_q + 2 * heads_kv) * head_dim,
               "pico_kv_append_fp8: qkv strides must be multiples of 8 elements and a token row must hold q|k|v");
  for (int d = 0; d < 3; ++d)
    PICO_REQUIRE(k_strides[d] % 8 == 0 && v_strides[d] % 8 == 0,
                 "pico_kv_append_fp8: cache strides must be multiples of 8 bytes");
  PICO_REQUIRE(cs_stride % 8 == 0 && cs_stride >= head_dim / 2, "pico_kv_append_fp8: bad cos/sin row stride %lld",
               (long long)cs_stride);
  PICO_REQUIRE(((uintptr_t)qkv | (uintptr_t)cos | (uintptr_t)sin) % 16 == 0 &&
                   ((uintptr_t)k_cache | (uintptr_t)v_cache) % 8 == 0 &&
                   ((uintptr_t)k_scale | (uintptr_t)v_scale) % 4 == 0,
               "pico_kv_append_fp8: qkv / cos / sin must be 16-byte, the caches 8-byte and the scales 4-byte aligned");
  PICO_REQUIRE(batch < (1 << 24) && tokens < (1 << 30), "pico_kv_append_fp8: tensor too large");
  const int vecs = (int)(head_dim / 16);
  KVA8Params a{};
  a.total = batch * tokens * (heads_q + 2 * heads_kv) * vecs;
  if (a.total == 0) return 0;
  int64_t nb = (a.total + 255) / 256;
  if (nb > 8192) nb = 8192;
  a.qkv = (bf16_t*)qkv, a.cosp = (const bf16_t*)cos, a.sinp = (const bf16_t*)sin, a.pos = pos;
  a.kc = (uint8_t*)k_cache, a.vc = (uint8_t*)v_cache, a.ksc = k_scale, a.vsc = v_scale;
  a.xs0 = batch_stride, a.xs1 = token_stride, a.cs = cs_stride;
  for (int d = 0; d < 3; ++d)
    a.ks[d] = k_strides[d], a.vs[d] = v_strides[d], a.kss[d] = k_scale_strides[d], a.vss[d] = v_scale_strides[d];
  a.heads_q = (int)heads_q, a.heads_kv = (int)heads_kv, a.tokens = (int)tokens, a.half = (int)(head_dim / 2);
  a.limit = (int)(s_max < table_rows ? s_max : table_rows);
  return pico_launch(PICO_K_ROPE, "kv_append_fp8", vecs == 4 ? kv_append_fp8_kernel<4> : kv_append_fp8_kernel<8>,
                     dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, a);
}
