// Host plan of the split flash-attention backward (attn_bwd_split.hip): which dK/dV kernel runs, the grids and the
// workspace layout, computed once per call from the shape, the CU count and the pico_select knobs. Plain C++, no
// HIP: the workspace query, the launch and tests/attn_bwd_plan_check.cpp read the same SplitPlan, so a size and a
// write cannot come from two functions.
#pragma once
#include <algorithm>

#include "../../include/picotron_hip.h"

constexpr int QB = 128;   // dQ kernel: query rows per workgroup (4 waves x 32)
constexpr int KVB = 128;  // 32-row dK/dV kernel: keys per workgroup
constexpr int QT = 32;    // 32-row dK/dV kernel: query rows per tile (the tile unit of every rule below)

// One-round causal schedule of the dK/dV kernel (round 5). A causal grid of one workgroup per 128-key block has
// blocks of unequal work (C2: 32, 28, ..., 4 query tiles per key block) and, at three workgroups per CU, 1024
// workgroups for 768 slots: the light blocks that do not fit the first round ran as a tail in a near-empty chip
// (blocks 6-7 from 39 to 52 us, one slot in three busy; profiles/r03_attn_wg_timelines.json). Grouped, each
// workgroup runs a short list of key blocks of one (batch, kv-head) one after the other, sized so that every
// head's groups fill exactly one round: with the CU's SIMD arbitration by age (the oldest of three resident
// workgroups runs a tile in ~1.15 us, the youngest in ~2.2), the groups dispatched first get the most work
// (block_groups). Same box, 3 interleaved rounds (profiles/r05_ab_attn_groups.jsonl): C2 dK/dV 57.4 -> 56.3 us,
// C4 (B 4, D 128, one workgroup per CU: 512 blocks -> 256 groups of equal work) 59.3 -> 58.4; the same grouping of
// the dQ kernel's query blocks measured slower (C2 42.8 -> 47.3 us, GQA-4 40.0 -> 43.9: its lightest-first front,
// q_front, frees slots early for the heavy blocks, which a one-round grid cannot), so the dQ grid stays plain.
// grp.n == 0: the plain grid, one block per workgroup.
constexpr int GRP_MAX = 16;  // groups per (batch, head)
struct BlkGroups {
  int n;                   // groups per (batch, head); 0 = one block per workgroup
  unsigned long long cnt;  // blocks in group g: nibble g (1..4)
  unsigned w[GRP_MAX];     // block ids of group g: byte j of w[g], j < its count (heaviest first)
};

// what the plan reads besides the shape
struct SplitEnv {
  int cus;                 // compute units of the device
  int kvp, waves, groups;  // PICO_SEL_ATTN_KVP, PICO_SEL_KVP_WAVES, PICO_SEL_ATTN_GROUPS (PICO_SEL_AUTO: the shape rule)
  int64_t stamp_bytes;     // workspace tail of a diagnostic stamp build (attn_bwd_split.h STAMP_BYTES), else 0
};

struct SplitPlan {
  bool kvp;    // dK/dV by the 64-row kernel (attn_bwd_kvp_kernel at D = 64, attn_bwd_kvp128_kernel at 128), else the 32-row one
  int waves;   // waves (x 32 keys) per dK/dV workgroup: 4, or 8 (attn_bwd_kvp_kernel only)
  int kvb;     // keys per dK/dV workgroup block = 32 waves
  int minb;    // dK/dV workgroups per CU the kernel's register budget is sized for
  int hsplit;  // workgroups sharing a key block's tile list (fp32 partials, summed by attn_bwd_dkv_kernel)
  BlkGroups grp;
  int q_front;  // dQ kernel: query blocks dispatched lightest-first
  int sq_pad;   // rows of the LSE / delta workspace per (batch, head): padded to the 64-row tiles
  int64_t q_grid, kv_grid;  // workgroups of the dQ and the dK/dV kernel
  // workspace, byte offsets: [lse2 | delta] each [B*Hq][sq_pad] fp32 (+ fp32 dK/dV partials when a small grid
  // splits key blocks) (+ the stamps of a diagnostic build): O(S), independent of the number of key blocks
  int64_t lse2_off, delta_off, part_off, stamp_off, bytes;
};

// attn_bwd_kvp_kernel (64-row tiles) for D = 64 up to 1536 causal / 4096 non-causal keys, the 32-row kernel beyond.
// Same box, 3 interleaved rounds each (profiles/r05_ab_kvp_default.jsonl, r05_ab_kvp_long.jsonl,
// r05_ab_kvp_waves.jsonl): dK/dV C2 55.2 -> 53.5 us, GQA-4 57.4 -> 53.2, C2 non-causal 76.7 -> 72.7, S 4096
// non-causal (config 5's off-diagonal ring blocks) 266.7 -> 255.5; at S 2048 causal the two kernels measured equal
// on one box (81.3 vs 81.0) and 91.0 vs 95.7 on another, at S 4096 causal 138.5 vs 144.7 and 143.7 vs 150.6.
// attn_bwd_kvp128_kernel always for head_dim 128. pico_select(PICO_SEL_ATTN_KVP, 0 / 1) forces either (A/B switch).
inline bool kvp_enabled(const pico_attn_args* a, int sel) {
  if (a->head_dim != 64 && a->head_dim != 128) return false;
  if (sel != PICO_SEL_AUTO) return sel != 0;
  return a->head_dim == 128 || a->seqlen_k <= (a->causal ? 1536 : 4096);
}

// waves (x 32 keys) per attn_bwd_kvp_kernel workgroup: 4 (two 128-key workgroups per CU), or 8 (one 256-key
// workgroup per CU: each Q / dO tile loaded and each barrier taken once for twice the keys) for non-causal blocks of
// 2048 keys and more: S 4096 non-causal 259.8 -> 256.8 us; at C2 shapes 8 waves lose (C2 52.9 -> 57.9, GQA-4
// 53.1 -> 65.5: a 256-workgroup grid is too coarse there). pico_select(PICO_SEL_KVP_WAVES, 4 / 8) forces either.
inline int kvp_waves(const pico_attn_args* a, int sel) {
  if (sel == 4 || sel == 8) return sel;
  return !a->causal && a->seqlen_k >= 2048 ? 8 : 4;
}

// workgroups per CU the kernels' register budgets are sized for (their __launch_bounds__ read these too).
// dQ kernel: 3 at D = 64 (168 VGPRs), 2 at D = 128 (248 VGPRs). attn_bwd_kvp_kernel: two waves per SIMD, <= 256
// VGPRs. 32-row dK/dV kernel: 3 (168 VGPRs) for causal grids, whose LPT-ordered
// uneven blocks fill any number of slots (C2 58.5 -> 52.6 us, S 4096 153 -> 143); 2 (256 VGPRs) for non-causal
// grids, whose equal blocks would leave a third round partly empty (C2 full: 1024 blocks = 2 rounds of 512 slots
// vs 1.33 rounds of 768) and whose mask-free body spills at 168 VGPRs (83 vs 123 us); 1 at D = 128 (≈ 340
// registers, AGPRs allowed).
constexpr int q_minb(int d) { return d == 64 ? 3 : 2; }
constexpr int kvp_minb(int waves) { return waves == 8 ? 1 : 2; }
constexpr int kv_minb(int d, bool causal) { return d == 128 ? 1 : causal ? 3 : 2; }

// split of a key block's tile list so that the dK/dV grid fills the 256 CUs (minb workgroups each; GQA-4
// C2 at MINB 3: kv + dkv 55.5 + 13.8 us with 4 parts, 67.2 + 9.6 with 2, 62.1 + 9.7 at MINB 2)
inline int kv_hsplit(const pico_attn_args* a, int kvb, int minb) {
  if (a->heads_kv <= 0 || a->heads_q % a->heads_kv != 0) return 1;
  const int64_t nblk = ((a->seqlen_k + kvb - 1) / kvb) * a->batch * a->heads_kv;
  const int64_t tiles = (a->heads_q / a->heads_kv) * ((a->seqlen_q + QT - 1) / QT);
  if (nblk <= 0) return 1;
  int d = 1;
  while (d < 8 && nblk * d < 256 * minb && 2 * d <= tiles) d *= 2;
  return d;
}

// dQ kernel: query blocks dispatched lightest-first (see attn_bwd_q_kernel)
inline int q_front(const pico_attn_args* a, int cus) {
  if (!a->causal) return 0;
  const int nmb = (int)((a->seqlen_q + QB - 1) / QB);
  const int64_t nbh = a->batch * a->heads_q;
  const int64_t first = (int64_t)cus * q_minb((int)a->head_dim) / (nbh > 0 ? nbh : 1);  // groups resident at once
  return first < nmb ? (int)(nmb - first) : 0;
}

// The one-round schedule of BlkGroups: the nblk blocks of each (batch, head) (work wt[i] in tiles) cut into
// G = minb * CUs / nbh groups, so that the grid is exactly one round of minb workgroups per CU. Groups are
// dispatched g-major, so a group's place among a CU's resident workgroups (oldest first) is g * nbh / CUs; its
// target work is proportional to the tile rate of that place (measured at three per CU, C2 dK/dV: 1.15 / 1.53 /
// 2.2 us per tile -> 1 / 0.75 / 0.53). Blocks go heaviest first to the group with the most target left (at most
// 4 per group). n = 0 (the plain grid) when that grid is one round already or the cut does not fit the table.
inline BlkGroups block_groups(const int* wt, int nblk, int64_t nbh, int minb, int cus) {
  BlkGroups t{};
  const int64_t slots = (int64_t)minb * cus;
  if (nbh <= 0 || nblk > 32 || (int64_t)nblk * nbh <= slots) return t;
  const int G = (int)(slots / nbh);
  if (G < 2 || G > GRP_MAX || nblk > 4 * G) return t;
  static const double spd[3] = {1.0, 0.75, 0.53};
  double tgt[GRP_MAX], load[GRP_MAX] = {0.0}, tot = 0.0, ssum = 0.0;
  int cnt[GRP_MAX] = {0};
  for (int i = 0; i < nblk; ++i) tot += wt[i];
  for (int g = 0; g < G; ++g) {
    const int cls = (int)std::min<int64_t>(minb - 1, (int64_t)g * nbh / cus);
    tgt[g] = minb == 1 ? 1.0 : spd[std::min(cls, 2)];
    ssum += tgt[g];
  }
  for (int g = 0; g < G; ++g) tgt[g] *= tot / ssum;
  int order[32];
  for (int i = 0; i < nblk; ++i) order[i] = i;
  std::stable_sort(order, order + nblk, [&](int x, int y) { return wt[x] > wt[y]; });
  for (int k = 0; k < nblk; ++k) {
    const int i = order[k];
    int best = -1;
    for (int g = 0; g < G; ++g)
      if (cnt[g] < 4 && (best < 0 || tgt[g] - load[g] > tgt[best] - load[best])) best = g;
    if (best < 0) return BlkGroups{};
    t.w[best] |= (unsigned)i << (8 * cnt[best]);
    ++cnt[best];
    load[best] += wt[i];
  }
  for (int g = 0; g < G; ++g) {
    if (cnt[g] == 0) return BlkGroups{};
    t.cnt |= (unsigned long long)cnt[g] << (4 * g);
  }
  t.n = G;
  return t;
}

// dK/dV kernel groups: key block kb sees (Hq / Hkv) * ceil((Sq - kvb kb) / 32) query tiles (causal, no hsplit).
// pico_select(PICO_SEL_ATTN_GROUPS, 0) restores the plain causal grids (one block per workgroup; A/B switch)
inline BlkGroups kv_groups(const pico_attn_args* a, const SplitPlan& p, const SplitEnv& e) {
  if (e.groups == 0 || !a->causal || p.hsplit != 1 || a->heads_kv <= 0) return BlkGroups{};
  const int nkb = (int)((a->seqlen_k + p.kvb - 1) / p.kvb);
  if (nkb > 32) return BlkGroups{};
  int wt[32];
  for (int kb = 0; kb < nkb; ++kb) {
    const int64_t q0 = (int64_t)kb * p.kvb;
    wt[kb] = (int)((a->heads_q / a->heads_kv) * (a->seqlen_q > q0 ? (a->seqlen_q - q0 + QT - 1) / QT : 0));
  }
  return block_groups(wt, nkb, a->batch * a->heads_kv, p.minb, e.cus);
}

inline SplitPlan split_plan(const pico_attn_args* a, const SplitEnv& e) {
  SplitPlan p{};
  p.kvp = kvp_enabled(a, e.kvp);
  p.waves = p.kvp && a->head_dim == 64 ? kvp_waves(a, e.waves) : KVB / 32;
  p.kvb = 32 * p.waves;
  p.minb = p.kvp && a->head_dim == 64 ? kvp_minb(p.waves) : kv_minb((int)a->head_dim, a->causal != 0);
  p.hsplit = kv_hsplit(a, p.kvb, p.minb);
  p.grp = kv_groups(a, p, e);
  p.q_front = q_front(a, e.cus);
  p.sq_pad = (int)((a->seqlen_q + 63) / 64) * 64;
  p.q_grid = (a->seqlen_q + QB - 1) / QB * a->batch * a->heads_q;
  const int64_t nkb = (a->seqlen_k + p.kvb - 1) / p.kvb;
  p.kv_grid = (p.grp.n ? p.grp.n : nkb) * a->batch * a->heads_kv * p.hsplit;
  const int64_t lsd = (a->batch * a->heads_q * (int64_t)p.sq_pad + 63) / 64 * 64 * 4;
  const int64_t part = p.hsplit > 1 ? 2 * p.hsplit * a->batch * a->seqlen_k * a->heads_kv * a->head_dim * 4 : 0;
  p.lse2_off = 0;
  p.delta_off = lsd;
  p.part_off = 2 * lsd;
  p.stamp_off = 2 * lsd + part;
  p.bytes = p.stamp_off + e.stamp_bytes;
  return p;
}
