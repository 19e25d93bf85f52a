// Host-only sweep of the split attention backward's plan (picotron_amd/csrc/attn_bwd_plan.h), built and run by
// tests/test_attn_bwd_plan.py: every shape x knob x CU count below must give a consistent SplitPlan. Exits
// non-zero with the failing shape printed.
// With arguments it prints plans instead (tests/test_attn_tiles_host.py): every 11 integers
//   head_dim causal batch seqlen_q seqlen_k heads_q heads_kv kvp waves groups cus      (knobs: -1 = PICO_SEL_AUTO)
// give one line "kvp waves kvb minb hsplit grp_n q_front q_grid kv_grid bytes".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../picotron_amd/csrc/attn_bwd_plan.h"

static const char* check(const pico_attn_args& a, const SplitEnv& e, const SplitPlan& p) {
  const int64_t nkb = (a.seqlen_k + p.kvb - 1) / p.kvb;
  // the block size: 128 keys, or 256 exactly when the 8-wave kernel is chosen
  const bool wave8 = p.kvp && a.head_dim == 64 && p.waves == 8;
  if (p.kvb != (wave8 ? 256 : 128) || p.kvb != 32 * p.waves) return "keys per block";
  if (p.waves != 4 && !wave8) return "waves";
  if (p.minb < 1 || p.minb > 3) return "minb";
  // hsplit: a power of two <= 8, and 1 whenever groups are on
  if (p.hsplit != 1 && p.hsplit != 2 && p.hsplit != 4 && p.hsplit != 8) return "hsplit";
  const BlkGroups& g = p.grp;
  if (g.n != 0 && (g.n < 2 || g.n > GRP_MAX)) return "group count";
  if (g.n != 0 && (p.hsplit != 1 || !a.causal || e.groups == 0)) return "groups on without a plain causal grid";
  if (g.n != 0) {  // every key block in exactly one group, 1-4 blocks per group
    int seen[256] = {0};
    for (int i = 0; i < g.n; ++i) {
      const int cnt = (int)((g.cnt >> (4 * i)) & 15);
      if (cnt < 1 || cnt > 4) return "blocks per group";
      for (int j = 0; j < cnt; ++j) ++seen[(g.w[i] >> (8 * j)) & 255];
    }
    for (int kb = 0; kb < 256; ++kb)
      if (seen[kb] != (kb < nkb ? 1 : 0)) return "a key block not in exactly one group";
    if (g.n < GRP_MAX && (g.cnt >> (4 * g.n)) != 0) return "count nibbles past the last group";
  }
  if (p.q_grid != (a.seqlen_q + QB - 1) / QB * a.batch * a.heads_q) return "dQ grid";
  if (p.kv_grid != (g.n ? g.n : nkb) * a.batch * a.heads_kv * p.hsplit) return "dK/dV grid";
  if (p.q_front < 0 || p.q_front > (a.seqlen_q + QB - 1) / QB || (!a.causal && p.q_front)) return "q_front";
  if (p.sq_pad % 64 || p.sq_pad < a.seqlen_q || p.sq_pad >= a.seqlen_q + 64) return "sq_pad";
  // the workspace regions: in order, disjoint, 4-byte aligned, large enough, ending at the reported total
  const int64_t lsd = a.batch * a.heads_q * p.sq_pad * 4;
  const int64_t part = p.hsplit > 1 ? 2 * p.hsplit * a.batch * a.seqlen_k * a.heads_kv * a.head_dim * 4 : 0;
  if (p.lse2_off != 0 || p.delta_off - p.lse2_off < lsd || p.part_off - p.delta_off < lsd) return "LSE / delta regions";
  if (p.stamp_off - p.part_off != part) return "partials region";
  if ((p.stamp_off > p.part_off) != (p.hsplit > 1)) return "partials exactly when hsplit > 1";
  if (p.bytes - p.stamp_off != e.stamp_bytes) return "stamp region / total";
  if ((p.delta_off | p.part_off | p.stamp_off | p.bytes) % 4) return "alignment";
  return nullptr;
}

static int print_plans(int argc, char** argv) {
  if ((argc - 1) % 11) return 3;
  for (int i = 1; i < argc; i += 11) {
    long x[11];
    for (int j = 0; j < 11; ++j) x[j] = strtol(argv[i + j], nullptr, 10);
    pico_attn_args a;
    memset(&a, 0, sizeof a);
    a.head_dim = x[0], a.causal = (int)x[1], a.batch = x[2], a.seqlen_q = x[3], a.seqlen_k = x[4];
    a.heads_q = x[5], a.heads_kv = x[6];
    const SplitEnv e{(int)x[10], (int)x[7], (int)x[8], (int)x[9], 0};
    const SplitPlan p = split_plan(&a, e);
    if (const char* why = check(a, e, p)) {
      printf("FAIL %s\n", why);
      return 1;
    }
    printf("%d %d %d %d %d %d %d %lld %lld %lld\n", (int)p.kvp, p.waves, p.kvb, p.minb, p.hsplit, p.grp.n, p.q_front,
           (long long)p.q_grid, (long long)p.kv_grid, (long long)p.bytes);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return print_plans(argc, argv);
  const int dims[] = {64, 128}, seqs[] = {1, 31, 32, 64, 200, 256, 1024, 1536, 1537, 2048, 4096, 4097};
  const int bhs[][2] = {{1, 1}, {3, 1}, {4, 16}, {5, 16}, {3, 100}};  // batch x heads_kv = 1, 3, 64, 80, 300
  const int sel3[] = {PICO_SEL_AUTO, 0, 1}, selw[] = {PICO_SEL_AUTO, 4, 8};
  long cases = 0, grouped = 0, split = 0;
  for (int d : dims) for (int causal : {0, 1}) for (int s : seqs) for (auto& bh : bhs) for (int gqa : {1, 4})
  for (int kvp : sel3) for (int waves : selw) for (int groups : sel3) for (int cus : {256, 304})
  for (int64_t stamps : {(int64_t)0, (int64_t)65536 * 32}) {
    pico_attn_args a;
    memset(&a, 0, sizeof a);
    a.batch = bh[0], a.heads_kv = bh[1], a.heads_q = bh[1] * gqa, a.seqlen_q = a.seqlen_k = s, a.head_dim = d;
    a.causal = causal;
    const SplitEnv e{cus, kvp, waves, groups, stamps};
    const SplitPlan p = split_plan(&a, e);
    ++cases, grouped += p.grp.n > 0, split += p.hsplit > 1;
    if (const char* why = check(a, e, p)) {
      printf("FAIL %s: head_dim %d causal %d seqlen %d batch %d heads_kv %d gqa %d | kvp %d waves %d groups %d cus %d "
             "stamps %lld -> kvp %d waves %d kvb %d minb %d hsplit %d grp.n %d offsets %lld %lld %lld %lld bytes %lld\n",
             why, d, causal, s, bh[0], bh[1], gqa, kvp, waves, groups, cus, (long long)stamps, p.kvp, p.waves, p.kvb,
             p.minb, p.hsplit, p.grp.n, (long long)p.lse2_off, (long long)p.delta_off, (long long)p.part_off,
             (long long)p.stamp_off, (long long)p.bytes);
      return 1;
    }
  }
  printf("ok: %ld plans, %ld with block groups, %ld with hsplit > 1\n", cases, grouped, split);
  return grouped > 0 && split > 0 ? 0 : 2;  // the sweep must reach both forms
}
