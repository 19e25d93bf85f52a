// Host plan of the split-KV decode attention (attn_decode.hip): the chunk length, the number of chunks and the
// workspace layout, computed from the shape and the CU count alone (never from the device lengths, so that a decode
// step needs no host round trip and keeps one grid for every step). Plain C++, no HIP: the workspace query, the
// launch and tests/attn_decode_plan_check.cpp read the same DecodePlan.
#pragma once
#include <stdint.h>

constexpr int DEC_MAX_GROUP = 8;    // query heads per kv head one workgroup serves (its q / accumulator registers)
constexpr int DEC_THREADS = 256;    // 4 waves
constexpr int DEC_UNROLL = 4;       // key rows in flight per lane group (x 2 16-byte loads: K and V)
constexpr int DEC_MIN_SPLIT = 256;  // shortest default chunk: below it the in-workgroup merge outweighs the stream
constexpr int DEC_WG_PER_CU = 2;    // workgroups per CU the default split aims at
constexpr int64_t DEC_ALIGN = 256;  // bytes: workspace regions start on their own cache lines

// keys one workgroup takes per loop trip: (4 waves x 64 lanes / (D / 8) lanes per key row) x DEC_UNROLL
constexpr int dec_keys_per_trip(int head_dim) { return DEC_THREADS / (head_dim / 8) * DEC_UNROLL; }

struct DecodePlan {
  int64_t split_keys;  // keys per chunk; chunk c covers [c * split_keys, min((c + 1) * split_keys, s_max))
  int64_t nsplit;      // chunks = ceil(s_max / split_keys); the grid is nsplit x heads_kv x batch
  // workspace, byte offsets. Partial p = (b * heads_q + h) * nsplit + c: m[p] (running maximum, log2 domain) and
  // l[p] (sum of exp2(s - m)) fp32, o[p][head_dim] fp32 (unnormalised). A chunk at or beyond the row's length
  // writes m = -inf, l = 0 and leaves o[p] alone; the combine kernel skips it.
  int64_t m_off, l_off, o_off, bytes;
};

// Default chunk: B * Hkv * nsplit >= DEC_WG_PER_CU * CUs where the cache is long enough (B = 1 fills the chip),
// in whole loop trips, never shorter than DEC_MIN_SPLIT keys.
inline int64_t decode_default_split(int64_t batch, int64_t heads_kv, int64_t s_max, int64_t head_dim, int cus) {
  const int64_t trip = dec_keys_per_trip((int)head_dim);
  const int64_t rows = batch * heads_kv > 0 ? batch * heads_kv : 1;
  const int64_t want = ((int64_t)DEC_WG_PER_CU * (cus > 0 ? cus : 1) + rows - 1) / rows;  // chunks per (b, kv head)
  int64_t sk = (s_max + want - 1) / want;
  sk = (sk + trip - 1) / trip * trip;
  if (sk < DEC_MIN_SPLIT) sk = DEC_MIN_SPLIT;
  return sk;
}

// split_keys <= 0: the default rule.
inline DecodePlan decode_plan(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t s_max, int64_t head_dim,
                              int64_t split_keys, int cus) {
  DecodePlan p{};
  p.split_keys = split_keys > 0 ? split_keys : decode_default_split(batch, heads_kv, s_max, head_dim, cus);
  p.nsplit = s_max > 0 ? (s_max + p.split_keys - 1) / p.split_keys : 1;
  const int64_t parts = batch * heads_q * p.nsplit;
  const int64_t ml = (parts * 4 + DEC_ALIGN - 1) / DEC_ALIGN * DEC_ALIGN;
  p.m_off = 0;
  p.l_off = ml;
  p.o_off = 2 * ml;
  p.bytes = p.o_off + (parts * head_dim * 4 + DEC_ALIGN - 1) / DEC_ALIGN * DEC_ALIGN;
  return p;
}
