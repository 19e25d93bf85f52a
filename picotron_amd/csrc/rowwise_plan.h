// Host dispatch of the row-wise and elementwise kernels (rmsnorm.hip, cross_entropy.hip, swiglu.hip, rope.hip):
// which template instantiation runs, the grids and the loop trips, computed from the shape alone. Plain C++, no HIP:
// the launches and tests/rowwise_plan_check.cpp read the same functions, so the case tables of the tests can be
// shown to reach every instantiation without a device.
#pragma once
#include <stdint.h>

#include <initializer_list>

#if defined(__HIP__) || defined(__HIPCC__)
#define RW_HD __host__ __device__ __forceinline__
#else
#define RW_HD inline
#endif

namespace rw {

// ---------------------------------------------------------------------------------------------------- RMSNorm
constexpr int RMS_FWD_WAVES = 4;  // forward: one wave per row, rows per 256-thread workgroup

// 512-column chunks a lane keeps in registers (the kernels' MAXC); -1: more than 8192 columns
inline int maxc_for(int64_t cols) {
  int64_t c = (cols + 511) / 512;
  if (c <= 1) return 1;
  if (c <= 2) return 2;
  if (c <= 4) return 4;
  if (c <= 8) return 8;
  if (c <= 16) return 16;
  return -1;
}

// backward: waves per workgroup (16 up to 1024 columns, 8 up to 2048, 4 above)
constexpr int bwd_waves(int maxc) { return maxc <= 2 ? 16 : (maxc == 4 ? 8 : 4); }

#ifndef PICO_RMS_BWD_MAXB
#define PICO_RMS_BWD_MAXB 256
#endif

inline int bwd_blocks(int64_t rows, int64_t cols) {  // one workgroup per CU at most: few dw partial rows
  const int nw = bwd_waves(maxc_for(cols));
  int64_t nb = (rows + nw - 1) / nw;
  return (int)(nb < PICO_RMS_BWD_MAXB ? nb : PICO_RMS_BWD_MAXB);
}

constexpr int PREV_COLS = 16;  // chained dw: column slots per workgroup

// chained dw: columns of the previous call's dw that each of this launch's nb workgroups reduces; above
// PREV_COLS the previous partials are reduced in their own launch first
inline int64_t chain_cpw(int64_t prev_cols, int nb) { return (prev_cols + nb - 1) / nb; }

// ---------------------------------------------------------------------------------------------------- CE
// 16-byte chunks of a logits row a thread keeps in registers (the kernels' NCH) at nt threads per row; -1: too large
inline int nch_for(int64_t vocab, int nt = 256) {
  const int64_t per = (vocab / 8 + nt - 1) / nt;
  for (int n : {2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64})
    if (per <= n) return n;
  return -1;
}

// pico_ce_scale_grad: workgroups over the n / 8 16-byte vectors of the flat gradient (grid-stride beyond 4096)
inline int scale_grid(int64_t n) {
  int64_t nb = (n / 8 + 255) / 256;
  if (nb < 1) nb = 1;
  if (nb > 4096) nb = 4096;
  return (int)nb;
}

// ---------------------------------------------------------------------------------------------------- embedding
constexpr int EMB_COLS_PER_TRIP = 256 * 8;  // embedding_bwd_kernel: columns one trip of the workgroup's loop covers
constexpr int EMB_RUN_BLOCK = 64;           // positions of a run summed from zero before they join the run's sum

// ---------------------------------------------------------------------------------------------------- SwiGLU
inline int grid_for(int64_t work) {
  int64_t nb = (work + 255) / 256;
  if (nb < 1) nb = 1;
  if (nb > 4096) nb = 4096;  // 256 CUs x 16 workgroups, grid-stride beyond
  return (int)nb;
}

inline bool vec_ok(int64_t cols, int64_t is, int64_t os, const void* a, const void* b, const void* c) {
  return cols % 8 == 0 && is % 8 == 0 && os % 8 == 0 && ((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16 == 0;
}

// ---------------------------------------------------------------------------------------------------- RoPE
constexpr int ROPE_MAX_BLOCKS = 8192;  // 256-thread workgroups, grid-stride beyond

inline int rope_grid(int64_t total) {
  int64_t nb = (total + 255) / 256;
  if (nb > ROPE_MAX_BLOCKS) nb = ROPE_MAX_BLOCKS;
  return (int)nb;
}

// n / d for 0 <= n < 2^31 by a multiply-high (round-up method; m and l precomputed on the host): the rope
// thread's index decomposition otherwise costs three 32-bit integer divisions (~40 VALU each), a sizeable
// share of a kernel that issues four 16-byte loads per thread
struct FastDiv {
  unsigned d, m, l;
};
inline FastDiv make_fastdiv(unsigned d) {
  FastDiv f;
  f.d = d;
  f.l = 0;
  while ((1ull << f.l) < d) ++f.l;
  f.m = (unsigned)((((1ull << 32) * ((1ull << f.l) - d)) / d) + 1);
  return f;
}
// high 32 bits of the 64-bit product: the host form, and on the device the same expression (one v_mul_hi_u32)
RW_HD unsigned mulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
RW_HD unsigned fdiv(unsigned n, const FastDiv& f) { return (mulhi(n, f.m) + n) >> f.l; }

}  // namespace rw
