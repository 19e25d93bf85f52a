// Host plan of the skinny weight-streaming linear (decode_linear.hip): how many workgroups share a column block's
// K range and the fp32 workspace their partials need, from (N, K, epilogue, CU count) alone. M does not enter, so
// a row computed alone and the same row inside a batch of 16 take the same split and give the same bits. Plain
// C++, no HIP: the workspace query and the launch read the same DecodeLinearPlan.
#pragma once
#include <stdint.h>

constexpr int DL_MAX_M = 16;         // rows of x: the B operand's 16 columns of one MFMA
constexpr int DL_THREADS = 256;      // 4 waves; they split the workgroup's K slice between them
constexpr int DL_WAVES = DL_THREADS / 64;
constexpr int DL_KSTEP = 32;         // K of v_mfma_f32_16x16x32_bf16
constexpr int DL_UNROLL = 4;         // K steps per wave and trip: 2 row blocks x 4 16-byte loads per lane in flight
constexpr int DL_BLOCK_ROWS = 32;    // rows of W per workgroup: two 16-row MFMA blocks (SWIGLU: 16 gate + 16 up)
constexpr int DL_MAX_SLICE = 2048;   // K per workgroup: 16 staged rows of x + the reduction = 72.3 KiB of LDS, 2 per CU
constexpr int DL_MIN_SLICE = 512;    // the default rule splits no finer: one trip of every wave
constexpr int DL_X_PAD = 8;          // bf16 elements between staged rows of x (16 lanes on 16 different banks)
constexpr int DL_RED_BYTES = DL_WAVES * 2 * 64 * 16;  // the waves' accumulators, reduced in wave order
constexpr int64_t DL_ALIGN = 256;

enum { DL_EPI_BF16 = 0, DL_EPI_F32 = 1, DL_EPI_SWIGLU = 2 };

struct DecodeLinearPlan {
  int64_t blocks;   // grid.x: column blocks (32 outputs; SWIGLU: 16 outputs = 16 gate + 16 up rows)
  int64_t split_k;  // grid.y: workgroups per column block; slice s covers [s * k_slice, min((s + 1) * k_slice, K))
  int64_t k_slice;  // a multiple of DL_KSTEP
  int64_t bytes;    // workspace: fp32 partials [split_k][M][N], 0 when split_k == 1
};

inline int64_t decode_linear_lds_bytes(int64_t m, int64_t k_slice) {
  return DL_RED_BYTES + m * (k_slice + DL_X_PAD) * 2;
}

// Default split: enough workgroups for every CU where the column blocks alone leave CUs idle, slices no shorter
// than DL_MIN_SLICE; always enough slices for one to fit LDS. split_k > 0: the caller's split (slices evened out).
inline DecodeLinearPlan decode_linear_plan(int64_t m, int64_t n, int64_t k, int epilogue, int64_t split_k, int cus) {
  DecodeLinearPlan p{};
  const int64_t outs = epilogue == DL_EPI_SWIGLU ? n / 2 : n;
  const int64_t per = epilogue == DL_EPI_SWIGLU ? DL_BLOCK_ROWS / 2 : DL_BLOCK_ROWS;
  p.blocks = (outs + per - 1) / per;
  const int64_t steps = k / DL_KSTEP;
  int64_t ks = split_k;
  if (ks <= 0) {
    ks = (cus > 0 ? cus : 1) / (p.blocks > 0 ? p.blocks : 1);
    const int64_t cap = k / DL_MIN_SLICE;
    if (ks > cap) ks = cap;
    const int64_t fit = (k + DL_MAX_SLICE - 1) / DL_MAX_SLICE;
    if (ks < fit) ks = fit;
  }
  if (ks < 1) ks = 1;
  if (ks > steps) ks = steps > 0 ? steps : 1;
  const int64_t slice_steps = (steps + ks - 1) / ks;
  p.k_slice = slice_steps * DL_KSTEP;
  p.split_k = slice_steps > 0 ? (steps + slice_steps - 1) / slice_steps : 1;
  p.bytes = p.split_k > 1 ? (p.split_k * m * n * 4 + DL_ALIGN - 1) / DL_ALIGN * DL_ALIGN : 0;
  return p;
}
