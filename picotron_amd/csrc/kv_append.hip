// Fused RoPE + KV-cache append for generation.
//
// qkv is the fused q|k|v GEMM output [B, T, (Hq + 2 Hkv) D] (T = 1 for a decode step, the prompt length for
// prefill). For row b, token t, p = pos[b] + t (pos: int32 [B] on the device, so a decode step needs no host round
// trip): q is rotated in place with table row p, k is rotated with row p and stored at k_cache[b, :, p, :], v is
// copied to v_cache[b, :, p, :]. The caches are head-major [B, Hkv, S_max, D] views with free strides: a kv head's
// keys are one contiguous stream for attn_decode_kernel, and the causal forward kernel reads the same memory
// through its stride arguments. A token with p outside [0, min(S_max, table rows)) is skipped whole: no q write, no
// cache write, nothing is ever stored outside the cache.
//
// The rotation is rope_kernel's (rope.hip): rotate-half, fp32 products rounded before the sum, one rounding to
// bf16, so the cached k and the rotated q are bit-identical to pico_rope's. Thread decomposition as there: one
// thread owns 8 consecutive rotary pairs (elements i..i+7 and i+D/2..) of one (b, t, head); a v head's thread
// copies the same two 16-byte pieces.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void kv_append_kernel(bf16_t* __restrict__ qkv, const bf16_t* __restrict__ cosp,
                                                        const bf16_t* __restrict__ sinp,
                                                        const int* __restrict__ pos, bf16_t* __restrict__ kc,
                                                        bf16_t* __restrict__ vc, int64_t total, int vecs, int heads_q,
                                                        int heads_kv, int tokens, int half, int limit, int64_t xs0,
                                                        int64_t xs1, int64_t cs, int64_t ks0, int64_t ks1, int64_t ks2,
                                                        int64_t vs0, int64_t vs1, int64_t vs2) {
  const int heads = heads_q + 2 * heads_kv;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int vi = (int)(t % vecs);
    const int64_t r0 = t / vecs;
    const int hd = (int)(r0 % heads);
    const int64_t r1 = r0 / heads;
    const int tok = (int)(r1 % tokens);
    const int b = (int)(r1 / tokens);
    const int64_t p = (int64_t)pos[b] + tok;
    if (p < 0 || p >= limit) continue;  // limit = min(S_max, table rows): beyond the cache or the table
    const int i = vi * 8;
    bf16_t* xp = qkv + (int64_t)b * xs0 + (int64_t)tok * xs1 + (int64_t)hd * (2 * half) + i;
    const u16x8 x1 = *reinterpret_cast<const u16x8*>(xp);
    const u16x8 x2 = *reinterpret_cast<const u16x8*>(xp + half);
    if (hd >= heads_q + heads_kv) {  // v: a copy
      bf16_t* op = vc + (int64_t)b * vs0 + (int64_t)(hd - heads_q - heads_kv) * vs1 + p * vs2 + i;
      *reinterpret_cast<u16x8*>(op) = x1;
      *reinterpret_cast<u16x8*>(op + half) = x2;
      continue;
    }
    const u16x8 c = *reinterpret_cast<const u16x8*>(cosp + p * cs + i);
    const u16x8 sn = *reinterpret_cast<const u16x8*>(sinp + p * cs + i);
    u16x8 o1, o2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = bf2f(x1[j]), bb = bf2f(x2[j]);
      const float cf = bf2f(c[j]), sf = bf2f(sn[j]);
      // rope_kernel's expression: products rounded before the sum (no FMA contraction)
      o1[j] = f2bf(__fmul_rn(a, cf) - __fmul_rn(bb, sf));
      o2[j] = f2bf(__fmul_rn(bb, cf) + __fmul_rn(a, sf));
    }
    bf16_t* op = hd < heads_q ? xp : kc + (int64_t)b * ks0 + (int64_t)(hd - heads_q) * ks1 + p * ks2 + i;
    *reinterpret_cast<u16x8*>(op) = o1;
    *reinterpret_cast<u16x8*>(op + half) = o2;
  }
}

}  // namespace

extern "C" int pico_kv_append(void* qkv, int64_t batch_stride, int64_t token_stride, const void* cos, const void* sin,
                              int64_t cs_stride, int64_t table_rows, const int32_t* pos, void* k_cache,
                              const int64_t* k_strides, void* v_cache, const int64_t* v_strides, int64_t batch,
                              int64_t tokens, int64_t heads_q, int64_t heads_kv, int64_t s_max, int64_t head_dim,
                              void* stream) {
  PICO_REQUIRE(qkv && cos && sin && pos && k_cache && k_strides && v_cache && v_strides,
               "pico_kv_append: null pointer");
  PICO_REQUIRE(head_dim == 64 || head_dim == 128, "pico_kv_append: head_dim=%lld unsupported (64, 128)",
               (long long)head_dim);
  PICO_REQUIRE(batch >= 0 && tokens >= 0 && heads_q > 0 && heads_kv > 0 && heads_q + 2 * heads_kv < (1 << 20),
               "pico_kv_append: bad batch=%lld / tokens=%lld / heads_q=%lld / heads_kv=%lld", (long long)batch,
               (long long)tokens, (long long)heads_q, (long long)heads_kv);
  PICO_REQUIRE(heads_q % heads_kv == 0, "pico_kv_append: heads_q=%lld is not a multiple of heads_kv=%lld",
               (long long)heads_q, (long long)heads_kv);
  PICO_REQUIRE(s_max > 0 && s_max <= (1 << 30) && table_rows >= 0, "pico_kv_append: bad cache length %lld / table rows %lld",
               (long long)s_max, (long long)table_rows);
  PICO_REQUIRE(batch_stride % 8 == 0 && token_stride % 8 == 0 && token_stride >= (heads_q + 2 * heads_kv) * head_dim,
               "pico_kv_append: qkv strides must be multiples of 8 elements and a token row must hold q|k|v");
  for (int d = 0; d < 3; ++d)
    PICO_REQUIRE(k_strides[d] % 8 == 0 && v_strides[d] % 8 == 0,
                 "pico_kv_append: strides must be multiples of 8 elements");
  PICO_REQUIRE(cs_stride % 8 == 0 && cs_stride >= head_dim / 2, "pico_kv_append: bad cos/sin row stride %lld",
               (long long)cs_stride);
  PICO_REQUIRE(((uintptr_t)qkv | (uintptr_t)cos | (uintptr_t)sin | (uintptr_t)k_cache | (uintptr_t)v_cache) % 16 == 0,
               "pico_kv_append: pointers must be 16-byte aligned");
  PICO_REQUIRE(batch < (1 << 24) && tokens < (1 << 30), "pico_kv_append: tensor too large");
  const int vecs = (int)(head_dim / 16);
  const int64_t total = batch * tokens * (heads_q + 2 * heads_kv) * vecs;
  if (total == 0) return 0;
  int64_t nb = (total + 255) / 256;
  if (nb > 8192) nb = 8192;
  const int64_t limit = s_max < table_rows ? s_max : table_rows;
  PICO_TRY(pico_launch(PICO_K_ROPE, "kv_append", kv_append_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream,
                       (bf16_t*)qkv, (const bf16_t*)cos, (const bf16_t*)sin, pos, (bf16_t*)k_cache, (bf16_t*)v_cache,
                       total, vecs, (int)heads_q, (int)heads_kv, (int)tokens, (int)(head_dim / 2), (int)limit,
                       batch_stride, token_stride, cs_stride, k_strides[0], k_strides[1], k_strides[2], v_strides[0],
                       v_strides[1], v_strides[2]));
  return 0;
}
