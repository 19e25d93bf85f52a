// Host-only sweep of the decode attention's plan (picotron_amd/csrc/attn_decode_plan.h), built and run by
// tests/test_generate_host.py: for every shape x split_keys x CU count below, the chunks must tile [0, S_max)
// exactly once and the workspace regions must be disjoint, aligned, large enough and end at the reported total.
// Exits non-zero with the failing shape printed.
#include <cstdio>
#include <vector>

#include "../picotron_amd/csrc/attn_decode_plan.h"

static const char* check(int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D, int64_t sk_arg, int cus,
                         const DecodePlan& p) {
  if (p.split_keys <= 0 || p.nsplit <= 0) return "non-positive split";
  if (sk_arg > 0 && p.split_keys != sk_arg) return "an explicit split_keys was not kept";
  if (sk_arg <= 0) {  // the default rule
    if (p.split_keys != decode_default_split(B, Hkv, S, D, cus)) return "default rule";
    if (p.split_keys < DEC_MIN_SPLIT) return "default chunk below the minimum";
    if (p.split_keys % dec_keys_per_trip((int)D)) return "default chunk is not whole loop trips";
    // never more chunks per (batch, kv head) than the fill target asks for
    const int64_t want = ((int64_t)DEC_WG_PER_CU * cus + B * Hkv - 1) / (B * Hkv);
    if (p.nsplit > want) return "more chunks than the fill target";
  }
  // chunks: [c * sk, min((c + 1) * sk, S)) tile [0, S) exactly once, none empty
  if (p.nsplit != (S + p.split_keys - 1) / p.split_keys) return "chunk count";
  if (S <= 4096) {
    std::vector<int> seen((size_t)S, 0);
    for (int64_t c = 0; c < p.nsplit; ++c) {
      const int64_t a = c * p.split_keys, b = (c + 1) * p.split_keys < S ? (c + 1) * p.split_keys : S;
      if (a >= b) return "an empty chunk in the grid";
      for (int64_t k = a; k < b; ++k) ++seen[(size_t)k];
    }
    for (int64_t k = 0; k < S; ++k)
      if (seen[(size_t)k] != 1) return "a key not in exactly one chunk";
  } else {
    if ((p.nsplit - 1) * p.split_keys >= S || p.nsplit * p.split_keys < S) return "chunks do not tile the cache";
  }
  // workspace: m | l | o in order, disjoint, aligned, large enough, ending at the total
  const int64_t parts = B * Hq * p.nsplit;
  if (p.m_off != 0) return "m offset";
  if (p.l_off - p.m_off < parts * 4) return "m region";
  if (p.o_off - p.l_off < parts * 4) return "l region";
  if (p.bytes - p.o_off < parts * D * 4) return "o region";
  if (p.bytes - p.o_off >= parts * D * 4 + DEC_ALIGN) return "total beyond the padded o region";
  if ((p.l_off | p.o_off | p.bytes) % DEC_ALIGN) return "alignment";
  return nullptr;
}

int main() {
  const int64_t dims[] = {64, 128}, batches[] = {1, 2, 3, 8, 32, 257};
  const int64_t hkvs[] = {1, 2, 8, 32}, groups[] = {1, 2, 3, 4, 6, 8};
  const int64_t smax[] = {1, 15, 16, 17, 160, 255, 256, 257, 1024, 2048, 4097, 8192, 131072};
  const int64_t splits[] = {0, 1, 16, 32, 64, 256, 1000, 1 << 20};
  const int cus[] = {1, 64, 256, 304};
  long n = 0;
  for (int64_t D : dims)
    for (int64_t B : batches)
      for (int64_t Hkv : hkvs)
        for (int64_t G : groups)
          for (int64_t S : smax)
            for (int64_t sk : splits)
              for (int cu : cus) {
                if (sk == 1 && S > 4096) continue;
                const DecodePlan p = decode_plan(B, Hkv * G, Hkv, S, D, sk, cu);
                const char* err = check(B, Hkv * G, Hkv, S, D, sk, cu, p);
                if (err) {
                  std::printf("FAIL %s: B=%lld Hq=%lld Hkv=%lld S=%lld D=%lld split_keys=%lld cus=%d -> split %lld x %lld\n",
                              err, (long long)B, (long long)(Hkv * G), (long long)Hkv, (long long)S, (long long)D,
                              (long long)sk, cu, (long long)p.split_keys, (long long)p.nsplit);
                  return 1;
                }
                ++n;
              }
  // B = 1 fills the chip: SmolLM geometry, 8192 keys, 256 CUs
  const DecodePlan f = decode_plan(1, 32, 32, 8192, 64, 0, 256);
  if (f.nsplit * 32 < 2 * 256) {
    std::printf("FAIL B=1 does not fill the chip: %lld chunks x 32 heads\n", (long long)f.nsplit);
    return 1;
  }
  std::printf("ok: %ld plans\n", n);
  return 0;
}
