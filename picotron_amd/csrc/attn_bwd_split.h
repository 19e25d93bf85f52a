// Shared by the kernels of the split flash-attention backward (attn_bwd_split.hip: overview; attn_bwd_q.hip,
// attn_bwd_kv.hip, attn_bwd_kvp.hip, attn_bwd_kvp128.hip: one kernel and its launcher each).
#pragma once
#include "attn_bwd_plan.h"
#include "attn_common.h"

constexpr int KT = 64;                                   // dq kernel: keys per tile
constexpr int KPW = 32, KH = KPW / 32, KNW = KVB / KPW;  // 32-row dkv kernel: keys per wave (one 32-key half), waves per workgroup
constexpr int QT2 = 64;                                  // 64-row dkv kernels: query rows per ring tile

// Diagnostic builds (scripts/gpu_attn_timeline.sh; results unchanged), the define given to every source that
// includes this header:
// PICO_BWDKV_WGSTAMP: diagnostic build — every dK/dV workgroup records s_memrealtime (100 MHz, chip-wide)
// at entry, loop start, loop end and after its stores drained (4 x 8 B per workgroup, grids <= 65536)
#ifndef PICO_BWDKV_WGSTAMP
#define PICO_BWDKV_WGSTAMP 0
#endif
// PICO_BWDQ_WGSTAMP: the same four stamps for every dQ workgroup (same workspace tail)
#ifndef PICO_BWDQ_WGSTAMP
#define PICO_BWDQ_WGSTAMP 0
#endif
// PICO_KVP_STAMP: diagnostic build — every wave of attn_bwd_kvp_kernel / attn_bwd_kvp128_kernel accumulates
// s_memtime (shader clock) deltas per phase of its tiles (0 wait, 1 barrier, 2 DMA issue, 3-6 M1(A), M1(B), M2(A),
// M2(B)), the tile count, the block prologue / epilogue cycles and the wave's start / end clocks: 16 x 8 B per wave
// at stamp_out[(block * NW + wave) * 16] (NW = waves per workgroup; scripts/kvp_stamps.py)
#ifndef PICO_KVP_STAMP
#define PICO_KVP_STAMP 0
#endif
constexpr int64_t STAMP_BYTES = (PICO_BWDKV_WGSTAMP || PICO_BWDQ_WGSTAMP || PICO_KVP_STAMP) ? 65536 * 4 * 8 : 0;

// the 64-row kernels' streams: a fence between two MFMA slots, and a phase stamp into the kernel's ph[] / tlast
#define KV_SLOT() __builtin_amdgcn_sched_barrier(0)
#if PICO_KVP_STAMP
#define KV_ST(i)                                                \
  {                                                             \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
    ph[i] += t_ - tlast;                                        \
    tlast = t_;                                                 \
  }
#else
#define KV_ST(i)
#endif

// w[g] for a wave-uniform g without indexing the kernel-argument array (selects, no scratch copy)
PICO_DEV unsigned grp_sel(const BlkGroups& t, int g) {
  unsigned r = t.w[0];
#pragma unroll
  for (int i = 1; i < GRP_MAX; ++i) r = g == i ? t.w[i] : r;
  return r;
}

PICO_DEV float halves_sum2(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

PICO_DEV bf16x8 tr_pair(const char* base, unsigned lo_off, unsigned hi_off) {
  const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)(base + lo_off));
  const i16x4 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)(base + hi_off));
  typedef __attribute__((ext_vector_type(8))) short i16x8;
  i16x8 v = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// Per-lane byte offsets of the 32x32x16 transposed operand of a [rows][D] lds_off<D> image: rows
// 4 (lane >> 5) + ((lane & 15) >> 2) (+8 for the second read), columns 32 dt + 16 ((lane >> 4) & 1) +
// 4 (lane & 3). A read at row0 (a multiple of 16: the swizzles see row bits 0-3 only) adds row0 * 2D.
template <int D>
PICO_DEV void tr_offsets(int lane, unsigned (&tro)[D / 32][2]) {
  const int g = lane >> 4, i = lane & 15, hh = g >> 1, q = i >> 2, p = i & 3;
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) {
    const int col = 32 * dt + 16 * (g & 1) + 4 * p;
    tro[dt][0] = lds_off<D>(4 * hh + q, col >> 3) + (col & 7) * 2;
    tro[dt][1] = lds_off<D>(4 * hh + q + 8, col >> 3) + (col & 7) * 2;
  }
}

// Accumulation into AGPR-resident accumulators (attn_bwd_kvp128_kernel: the VGPR-form build keeps every builtin MFMA's
// accumulator in VGPRs, which the wave cannot hold beside its S / dP pipeline; the same form in the D = 128 dQ
// kernel, two waves per SIMD, measured slower: C4 41.0 -> 44.8 us, profiles/r06_dq128_agpr/): the compiler sees an opaque
// instruction, so the asm carries what its hazard recognizer would add (s_nop 1: VALU write -> MFMA read of the
// packed operand, 2 wait states); the accumulators are AGPR-class from their zero-initialisation (no copies at the
// loop edge) and are read only after a drain (acc_drain: the last MFMA's write before any VALU read)
PICO_DEV void mfma32_acc(f32x16& acc, const bf16x8& x, const bf16x8& y) {
  asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(x), "v"(y));
}
PICO_DEV void acc_drain4(f32x16 (&v)[4]) {
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" : "+a"(v[0]), "+a"(v[1]), "+a"(v[2]), "+a"(v[3]));
}

// The launchers, one per kernel file: the pico_launch of the instantiation the shape and the plan name.
int attn_bwd_q_launch(const pico_attn_args* a, const SplitPlan& p, hipStream_t s);       // attn_bwd_q.hip
int attn_bwd_kv_launch(const pico_attn_args* a, const SplitPlan& p, hipStream_t s);      // attn_bwd_kv.hip
int attn_bwd_kvp_launch(const pico_attn_args* a, const SplitPlan& p, hipStream_t s);     // attn_bwd_kvp.hip, D = 64
int attn_bwd_kvp128_launch(const pico_attn_args* a, const SplitPlan& p, hipStream_t s);  // attn_bwd_kvp128.hip

// a region of the call's workspace (SplitPlan byte offset)
template <typename T>
inline T* split_ws(const pico_attn_args* a, int64_t off) {
  return (T*)((char*)a->workspace + off);
}
