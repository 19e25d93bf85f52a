// Lane mapping of the ring-attention block merge (attn_merge.hip): which lane of which workgroup serves which
// 8 columns of which (b, s, h) row. Plain C++, no HIP: the kernel, the launch and tests/attn_merge_plan_check.cpp
// read the same functions.
//
// A row is D / 8 lanes of 8 columns each. Every lane of a row reads the row's running lse and the lane of columns
// 0..7 then overwrites it, which is ordered only while all lanes of the row execute together: a row never spans two
// waves. So a row gets a lane group of the next power of two >= D / 8 (1..32, a divisor of the 64-lane wave), the
// surplus lanes of a group idle, and a workgroup serves 256 / group whole rows. For D / 8 a power of two (D = 8, 16,
// 32, 64, 128, 256) no lane idles and lane t of workgroup w serves what global lane 256 w + t always served.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define MERGE_HD __host__ __device__ inline
#else
#define MERGE_HD inline
#endif

constexpr int MERGE_THREADS = 256;  // 4 waves
constexpr int MERGE_WAVE = 64;
constexpr int MERGE_VEC = 8;        // columns per lane
constexpr int MERGE_MAX_DIM = 256;  // 32 lanes per row at the most

struct MergePlan {
  int lpr;          // live lanes per row = D / 8
  int shift;        // log2 of the lane group (lanes reserved per row)
  int rows_per_wg;  // 256 >> shift
  int64_t grid;     // workgroups = ceil(rows / rows_per_wg)
};

struct MergeLane {
  int64_t row;  // (b * S + s) * H + h
  int sub;      // columns sub * 8 .. sub * 8 + 7
  bool live;    // false: a surplus lane of its group, or a row past the end
};

inline bool merge_dim_ok(int64_t head_dim) {
  return head_dim > 0 && head_dim % MERGE_VEC == 0 && head_dim <= MERGE_MAX_DIM;
}

inline MergePlan merge_plan(int64_t rows, int64_t head_dim) {
  MergePlan p{};
  p.lpr = (int)(head_dim / MERGE_VEC);
  p.shift = 0;
  while ((1 << p.shift) < p.lpr) ++p.shift;
  p.rows_per_wg = MERGE_THREADS >> p.shift;
  p.grid = (rows + p.rows_per_wg - 1) / p.rows_per_wg;
  return p;
}

MERGE_HD MergeLane merge_lane(int lpr, int shift, int64_t block, int tid, int64_t rows) {
  MergeLane l;
  l.row = block * (MERGE_THREADS >> shift) + (tid >> shift);
  l.sub = tid & ((1 << shift) - 1);
  l.live = l.sub < lpr && l.row < rows;
  return l;
}
