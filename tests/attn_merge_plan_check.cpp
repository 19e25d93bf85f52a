// Host check of picotron_amd/csrc/attn_merge_plan.h (no HIP, CPU only; built and run by tests/test_split_host.py).
//
// Without arguments: the sweep. For every D = 8..256 step 8 and row counts around every multiple of the rows per
// workgroup (and a few large ones), walking every lane of every workgroup of the grid (sampled workgroups for the
// large counts): the live lanes of a row lie within one 64-lane wave of one workgroup, every (row, sub) with
// sub < D / 8 is served exactly once and nothing else is, the grid fits 2^31 - 1 and has no workgroup without a row;
// where D / 8 is a power of two, lane t of workgroup w serves row (256 w + t) / (D / 8), columns (256 w + t) % (D / 8):
// the mapping before the lane groups were padded. Prints "ok: <lanes walked>" or the first failure (exit 1).
//
// With arguments: one line "case key=value ..." per case, for the coverage assertions of the host tests:
//   merge:ROWS:D             lanes per row, lane group, rows per workgroup, grid, rows straddling a wave under the
//                            unpadded mapping
//   decode:D:SPLIT:SMAX      keys per loop trip, lane groups, chunks, trips per full chunk (attn_decode_plan.h; SPLIT
//                            must be an explicit positive chunk length)
//   decode_consts            DEC_MAX_GROUP, DEC_UNROLL, DEC_THREADS
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "../picotron_amd/csrc/attn_decode_plan.h"
#include "../picotron_amd/csrc/attn_merge_plan.h"

namespace {

long long walked = 0;

int fail(const char* what, int64_t rows, int D, int64_t block, int tid) {
  std::printf("FAIL %s: rows=%lld D=%d workgroup=%lld lane=%d\n", what, (long long)rows, D, (long long)block, tid);
  return 1;
}

// every lane of workgroups [b0, b1): returns non-zero on the first failure; counts the live lanes into *served
int walk(int64_t rows, int D, const MergePlan& p, int64_t b0, int64_t b1, std::vector<unsigned char>* seen,
         long long* served) {
  const bool pow2 = (p.lpr & (p.lpr - 1)) == 0;
  for (int64_t blk = b0; blk < b1; ++blk) {
    std::vector<int> wave_of((size_t)p.rows_per_wg, -1);
    bool any = false;
    for (int tid = 0; tid < MERGE_THREADS; ++tid) {
      ++walked;
      const MergeLane l = merge_lane(p.lpr, p.shift, blk, tid, rows);
      if (!l.live) continue;
      any = true;
      ++*served;
      if (l.row < 0 || l.row >= rows || l.sub < 0 || l.sub >= p.lpr) return fail("lane out of range", rows, D, blk, tid);
      const int64_t local = l.row - blk * p.rows_per_wg;
      if (local < 0 || local >= p.rows_per_wg) return fail("row of another workgroup", rows, D, blk, tid);
      const int wave = tid / MERGE_WAVE;
      if (wave_of[(size_t)local] < 0) wave_of[(size_t)local] = wave;
      if (wave_of[(size_t)local] != wave) return fail("a row spans two waves", rows, D, blk, tid);
      if (seen) {
        unsigned char& s = (*seen)[(size_t)(l.row * p.lpr + l.sub)];
        if (s) return fail("served twice", rows, D, blk, tid);
        s = 1;
      }
      if (pow2) {
        const int64_t gid = blk * MERGE_THREADS + tid;
        if (l.row != gid / p.lpr || l.sub != (int)(gid % p.lpr))
          return fail("differs from the unpadded mapping", rows, D, blk, tid);
      }
    }
    if (!any) return fail("a workgroup without a row", rows, D, blk, 0);
  }
  return 0;
}

int sweep() {
  for (int D = MERGE_VEC; D <= MERGE_MAX_DIM; D += MERGE_VEC) {
    if (!merge_dim_ok(D)) return fail("merge_dim_ok", 0, D, 0, 0);
    const MergePlan q = merge_plan(1, D);
    if (q.lpr != D / MERGE_VEC || (1 << q.shift) < q.lpr || (q.shift && (1 << (q.shift - 1)) >= q.lpr) ||
        (1 << q.shift) > MERGE_WAVE / 2 || q.rows_per_wg << q.shift != MERGE_THREADS)
      return fail("lane group", 1, D, 0, 0);
    std::vector<int64_t> counts = {1, 2, 3, 5, 63, 64, 65, 4096, 4112, 4113};
    for (int m = 1; m <= 3; ++m)
      for (int d = -1; d <= 1; ++d) counts.push_back((int64_t)m * q.rows_per_wg + d);
    for (int64_t rows : counts) {
      if (rows <= 0) continue;
      const MergePlan p = merge_plan(rows, D);
      if (p.grid != (rows + p.rows_per_wg - 1) / p.rows_per_wg || p.grid > 0x7fffffff)
        return fail("grid", rows, D, p.grid, 0);
      std::vector<unsigned char> seen((size_t)(rows * p.lpr), 0);
      long long served = 0;
      if (walk(rows, D, p, 0, p.grid, &seen, &served)) return 1;
      if (served != rows * p.lpr) return fail("not every (row, sub) served", rows, D, p.grid, 0);
      // one workgroup further would serve nothing
      for (int tid = 0; tid < MERGE_THREADS; ++tid)
        if (merge_lane(p.lpr, p.shift, p.grid, tid, rows).live) return fail("row beyond the grid", rows, D, p.grid, tid);
    }
    // large row counts: the first, a middle and the last workgroups; 2^31 - 1 rows is the entry point's limit at H = 1
    for (int64_t rows : {(int64_t)1 << 24, ((int64_t)1 << 31) - 1, (int64_t)0x7fffffff * q.rows_per_wg}) {
      const MergePlan p = merge_plan(rows, D);
      if (p.grid > 0x7fffffff || p.grid * p.rows_per_wg < rows || (p.grid - 1) * p.rows_per_wg >= rows)
        return fail("grid (large)", rows, D, p.grid, 0);
      long long served = 0;
      if (walk(rows, D, p, 0, 2, nullptr, &served) || walk(rows, D, p, p.grid / 2, p.grid / 2 + 1, nullptr, &served) ||
          walk(rows, D, p, p.grid - 2, p.grid, nullptr, &served))
        return 1;
    }
  }
  for (int64_t bad : {(int64_t)0, (int64_t)-8, (int64_t)4, (int64_t)12, (int64_t)260, (int64_t)264, (int64_t)512})
    if (merge_dim_ok(bad)) return fail("merge_dim_ok accepts", 0, (int)bad, 0, 0);
  std::printf("ok: %lld lanes\n", walked);
  return 0;
}

std::vector<long long> fields(const std::string& s, std::string* name) {
  std::vector<long long> v;
  std::stringstream ss(s);
  std::string tok;
  bool first = true;
  while (std::getline(ss, tok, ':')) {
    if (first) *name = tok;
    else v.push_back(std::atoll(tok.c_str()));
    first = false;
  }
  return v;
}

int describe(const std::string& c) {
  std::string name;
  const std::vector<long long> a = fields(c, &name);
  if (name == "merge" && a.size() == 2 && merge_dim_ok(a[1])) {
    const MergePlan p = merge_plan(a[0], a[1]);
    long long straddle = 0;  // rows whose lanes gid = row * lpr .. row * lpr + lpr - 1 cross a multiple of 64
    for (long long r = 0; r < a[0]; ++r) straddle += (r * p.lpr) / MERGE_WAVE != (r * p.lpr + p.lpr - 1) / MERGE_WAVE;
    std::printf("%s lpr=%d group=%d rows_per_wg=%d grid=%lld straddle=%lld\n", c.c_str(), p.lpr, 1 << p.shift,
                p.rows_per_wg, (long long)p.grid, straddle);
  } else if (name == "decode" && a.size() == 3 && a[1] > 0) {
    const DecodePlan p = decode_plan(1, 1, 1, a[2], a[0], a[1], 256);
    const int trip = dec_keys_per_trip((int)a[0]);
    std::printf("%s trip=%d groups=%d nsplit=%lld chunk_trips=%lld\n", c.c_str(), trip, trip / DEC_UNROLL,
                (long long)p.nsplit, (long long)((p.split_keys + trip - 1) / trip));
  } else if (name == "decode_consts" && a.empty()) {
    std::printf("%s max_group=%d unroll=%d threads=%d\n", c.c_str(), DEC_MAX_GROUP, DEC_UNROLL, DEC_THREADS);
  } else {
    std::printf("FAIL: bad case %s\n", c.c_str());
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return sweep();
  for (int i = 1; i < argc; ++i)
    if (describe(argv[i])) return 1;
  return 0;
}
