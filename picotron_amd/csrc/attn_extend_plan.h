// Host plan of the multi-token extend attention (attn_extend.hip): the chunk length, the number of chunks, the
// query blocks and the workspace layout, computed from the shape and the CU count alone (never from the device
// lengths: an extend step needs no host round trip and keeps one grid for every step). Plain C++, no HIP.
#pragma once
#include <stdint.h>

constexpr int EXT_MAX_TOKENS = 16;   // new tokens per row and call (mirrored as generate.MAX_EXTEND_TOKENS)
constexpr int EXT_MAX_GROUP = 8;     // query heads per kv head
constexpr int EXT_THREADS = 256;     // 4 waves
constexpr int EXT_STEP_KEYS = 32;    // keys of one wave step: two 16-key score tiles = one PV product's k extent
constexpr int EXT_TRIP_KEYS = 128;   // keys one workgroup takes per trip: 4 waves x EXT_STEP_KEYS, interleaved by wave
constexpr int EXT_BLOCK_ROWS = 16;   // query rows of one MFMA block (the n extent of 16x16x32)
constexpr int EXT_WG_ROWS = 32;      // query rows per workgroup: two blocks (one where the call has <= 16 rows)
constexpr int EXT_MIN_SPLIT = 256;   // shortest default chunk, as the decode kernel's
constexpr int EXT_WG_PER_CU = 2;     // workgroups per CU the default split aims at
constexpr int64_t EXT_ALIGN = 256;   // bytes: workspace regions start on their own cache lines

struct ExtendPlan {
  int64_t rows;        // query rows per kv head: tokens x (heads_q / heads_kv); row r is (t = r / G, g = r % G)
  int blocks;          // MFMA blocks a workgroup runs: 1 if rows <= 16, else 2
  int64_t qblocks;     // workgroups per chunk: ceil(rows / (16 blocks))
  int64_t split_keys;  // keys per chunk; chunk c covers [c * split_keys, min((c + 1) * split_keys, s_max))
  int64_t nsplit;      // chunks; the grid is (nsplit * qblocks) x heads_kv x batch, x = chunk * qblocks + qblock
  // workspace, byte offsets. Partial p = ((b * tokens + t) * heads_q + h) * nsplit + c: m[p] (maximum, log2 domain),
  // l[p] (sum of exp2(s - m)) fp32, o[p][head_dim] fp32 (unnormalised). A (row, chunk) with no visible key has
  // m = -inf, l = 0; a chunk beyond the batch row's length leaves o[p] unwritten, and the combine kernel skips it.
  int64_t m_off, l_off, o_off, bytes;
};

inline int64_t extend_rows(int64_t tokens, int64_t heads_q, int64_t heads_kv) {
  return tokens * (heads_kv > 0 ? heads_q / heads_kv : 0);
}

// Default chunk: B * Hkv * qblocks * nsplit >= EXT_WG_PER_CU * CUs where the cache is long enough, in whole
// workgroup trips, never shorter than EXT_MIN_SPLIT keys.
inline int64_t extend_default_split(int64_t batch, int64_t tokens, int64_t heads_q, int64_t heads_kv, int64_t s_max,
                                    int cus) {
  const int64_t rows = extend_rows(tokens, heads_q, heads_kv);
  const int64_t qb = rows <= EXT_BLOCK_ROWS ? 1 : (rows + EXT_WG_ROWS - 1) / EXT_WG_ROWS;
  const int64_t wgs = batch * heads_kv * qb > 0 ? batch * heads_kv * qb : 1;
  const int64_t want = ((int64_t)EXT_WG_PER_CU * (cus > 0 ? cus : 1) + wgs - 1) / wgs;
  int64_t sk = (s_max + want - 1) / want;
  sk = (sk + EXT_TRIP_KEYS - 1) / EXT_TRIP_KEYS * EXT_TRIP_KEYS;
  if (sk < EXT_MIN_SPLIT) sk = EXT_MIN_SPLIT;
  return sk;
}

// split_keys <= 0: the default rule.
inline ExtendPlan extend_plan(int64_t batch, int64_t tokens, int64_t heads_q, int64_t heads_kv, int64_t s_max,
                              int64_t head_dim, int64_t split_keys, int cus) {
  ExtendPlan p{};
  p.rows = extend_rows(tokens, heads_q, heads_kv);
  p.blocks = p.rows <= EXT_BLOCK_ROWS ? 1 : 2;
  p.qblocks = (p.rows + EXT_BLOCK_ROWS * p.blocks - 1) / (EXT_BLOCK_ROWS * p.blocks);
  p.split_keys = split_keys > 0 ? split_keys : extend_default_split(batch, tokens, heads_q, heads_kv, s_max, cus);
  p.nsplit = s_max > 0 ? (s_max + p.split_keys - 1) / p.split_keys : 1;
  const int64_t parts = batch * tokens * heads_q * p.nsplit;
  const int64_t ml = (parts * 4 + EXT_ALIGN - 1) / EXT_ALIGN * EXT_ALIGN;
  p.m_off = 0;
  p.l_off = ml;
  p.o_off = 2 * ml;
  p.bytes = p.o_off + (parts * head_dim * 4 + EXT_ALIGN - 1) / EXT_ALIGN * EXT_ALIGN;
  return p;
}
