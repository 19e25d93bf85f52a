// Host plan of the MXFP4 weight-only skinny linear (decode_linear_mxfp4.hip), beside decode_linear_fp8_plan.h: the
// same workgroup (4 waves, 32 rows of W, x staged in LDS as bf16) over K steps of 128 columns, one 16-byte load of 32
// e2m1 codes (one MX block) per lane. From (N, K, epilogue, CU count) alone; M does not enter. Plain C++, no HIP.
#pragma once
#include "decode_linear_plan.h"

constexpr int MX4_BLOCK = 32;         // elements that share one E8M0 scale byte
constexpr int DL4_KSTEP = 128;        // columns of one 16-byte load per lane group: four v_mfma_f32_16x16x32_bf16
constexpr int DL4_UNROLL = 4;         // loads per row block, wave and trip: a trip is 512 columns, 16 scale bytes a row
constexpr int DL4_TRIP = DL4_KSTEP * DL4_UNROLL;
constexpr int DL4_MAX_SLICE = 2048;   // x is staged as bf16 as in the bf16 kernel: the same 72.3 KiB at M = 16
// The default rule splits no finer than two trips, as the FP8 rule does: 1024 columns here. That slice holds the
// bytes of the FP8 kernel's 512-column slice (16 KiB of codes per workgroup) and keeps two waves streaming; a
// 512-column slice would be one trip, three waves of four idle behind 8 KiB, and every slice adds an [M, N] fp32
// partial to the finishing launch, which already costs the FP8 route more than its stream saves on the small shapes.
constexpr int DL4_MIN_SLICE = 1024;
// a slice holds at most four trips, one per wave: the kernel has no second trip to prefetch
static_assert(DL4_MAX_SLICE / DL4_TRIP <= DL_WAVES, "a wave takes at most one trip of its slice");

// Default split: one workgroup per CU where the column blocks alone leave CUs idle, slices no shorter than
// DL4_MIN_SLICE; always enough slices for one to fit LDS. split_k > 0: the caller's split (slices evened out to
// multiples of DL4_KSTEP).
inline DecodeLinearPlan decode_linear_mxfp4_plan(int64_t m, int64_t n, int64_t k, int epilogue, int64_t split_k,
                                                 int cus) {
  DecodeLinearPlan p{};
  const int64_t outs = epilogue == DL_EPI_SWIGLU ? n / 2 : n;
  const int64_t per = epilogue == DL_EPI_SWIGLU ? DL_BLOCK_ROWS / 2 : DL_BLOCK_ROWS;
  p.blocks = (outs + per - 1) / per;
  const int64_t steps = k / DL4_KSTEP;
  int64_t ks = split_k;
  if (ks <= 0) {
    ks = (cus > 0 ? cus : 1) / (p.blocks > 0 ? p.blocks : 1);
    const int64_t cap = k / DL4_MIN_SLICE;
    if (ks > cap) ks = cap;
    const int64_t fit = (k + DL4_MAX_SLICE - 1) / DL4_MAX_SLICE;
    if (ks < fit) ks = fit;
  }
  if (ks < 1) ks = 1;
  if (ks > steps) ks = steps > 0 ? steps : 1;
  const int64_t slice_steps = (steps + ks - 1) / ks;
  p.k_slice = slice_steps * DL4_KSTEP;
  p.split_k = slice_steps > 0 ? (steps + slice_steps - 1) / slice_steps : 1;
  p.bytes = p.split_k > 1 ? (p.split_k * m * n * 4 + DL_ALIGN - 1) / DL_ALIGN * DL_ALIGN : 0;
  return p;
}
