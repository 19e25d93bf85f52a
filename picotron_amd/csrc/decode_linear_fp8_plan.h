// Host plan of the FP8 weight-only skinny linear (decode_linear_fp8.hip), beside decode_linear_plan.h: the same
// workgroup (4 waves, 32 rows of W, x staged in LDS as bf16) over K steps of 64 columns, one 16-byte load of e4m3
// codes per lane. From (N, K, epilogue, CU count) alone; M does not enter. Plain C++, no HIP.
#pragma once
#include "decode_linear_plan.h"

constexpr int DL8_KSTEP = 64;        // columns of one 16-byte load per lane group: two v_mfma_f32_16x16x32_bf16
constexpr int DL8_UNROLL = 4;        // loads per row block, wave and trip: a trip is 256 columns
constexpr int DL8_MAX_SLICE = 2048;  // x is staged as bf16 as in the bf16 kernel: the same 72.3 KiB at M = 16
// The default rule splits no finer than two trips (waves 0 and 1 one trip each). A slice is half the bytes of the
// bf16 kernel's slice of the same columns, but a finer cut buys workgroups only beyond one per CU on the shapes that
// split at all, and every slice adds an [M, N] fp32 partial to the finishing launch.
constexpr int DL8_MIN_SLICE = 512;

// Default split: one workgroup per CU where the column blocks alone leave CUs idle, slices no shorter than
// DL8_MIN_SLICE; always enough slices for one to fit LDS. split_k > 0: the caller's split (slices evened out to
// multiples of DL8_KSTEP).
inline DecodeLinearPlan decode_linear_fp8_plan(int64_t m, int64_t n, int64_t k, int epilogue, int64_t split_k,
                                               int cus) {
  DecodeLinearPlan p{};
  const int64_t outs = epilogue == DL_EPI_SWIGLU ? n / 2 : n;
  const int64_t per = epilogue == DL_EPI_SWIGLU ? DL_BLOCK_ROWS / 2 : DL_BLOCK_ROWS;
  p.blocks = (outs + per - 1) / per;
  const int64_t steps = k / DL8_KSTEP;
  int64_t ks = split_k;
  if (ks <= 0) {
    ks = (cus > 0 ? cus : 1) / (p.blocks > 0 ? p.blocks : 1);
    const int64_t cap = k / DL8_MIN_SLICE;
    if (ks > cap) ks = cap;
    const int64_t fit = (k + DL8_MAX_SLICE - 1) / DL8_MAX_SLICE;
    if (ks < fit) ks = fit;
  }
  if (ks < 1) ks = 1;
  if (ks > steps) ks = steps > 0 ? steps : 1;
  const int64_t slice_steps = (steps + ks - 1) / ks;
  p.k_slice = slice_steps * DL8_KSTEP;
  p.split_k = slice_steps > 0 ? (steps + slice_steps - 1) / slice_steps : 1;
  p.bytes = p.split_k > 1 ? (p.split_k * m * n * 4 + DL_ALIGN - 1) / DL_ALIGN * DL_ALIGN : 0;
  return p;
}
