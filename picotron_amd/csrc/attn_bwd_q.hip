// Split flash-attention backward (attn_bwd_split.hip), the dQ kernel (query-major, runs first):
//   attn_bwd_q_kernel: one workgroup = 4 waves = 128 query rows of one (batch, q-head),
//     sweeping 64-key tiles of K and V (LDS-DMA ring). Swapped products with the query on the lane:
//     S^T = K Q^T and dP^T = V dO^T (A = K / V rows from LDS, B = Q / dO fragments held in registers),
//     P^T and dS^T lane-local (LSE and delta are per-lane constants; dP starts from -delta as the
//     MFMA's C operand), dQ^T += K^T dS^T (A = transposed reads of the same K image, B = the dS^T
//     accumulator packed to bf16 in place). It also computes delta = rowsum(dO*O) from registers and
//     writes delta / LSE*log2(e) for the second kernel (no separate pre-pass).
// It recomputes S and dP (3 products per score here, 4 in the dK/dV kernel: 7 vs the fused form's 5), trading
// 40 % more MFMA work for no slabs, no atomics, no cross-wave dS exchange and no barrier other than the ring's.
// RoPE^-1 (PICO_ATTN_ROPE_BWD) is applied in the epilogue: the rotation pairs (d, d + D/2) sit in
// one lane (accumulator tiles dt and dt + D/64), so it is register-local.
#include "attn_bwd_split.h"

namespace {

// dQ kernel: ring slots and workgroups per CU the register budget is sized for. D = 64: 3 slots (48 KiB), three
// workgroups per CU at 168 VGPRs (the two 32-key halves of a tile in turn: C2 45.7 -> 44.1 us, S 4096 115.9 ->
// 107.4). D = 128: 2 slots (64 KiB), two workgroups per CU at 248 VGPRs (V's fragments read after the S chain):
// C4 dQ 36.5 -> 33.8 us, GQA-4 44.5 -> 39.4.
template <int D>
struct QCfg {
  static constexpr int KS = D / 16, DT = D / 32, CPR = D / 8, RB = 2 * D;
  static constexpr int MINB = q_minb(D);         // workgroups per CU (register budget 168 / 248 VGPRs)
  static constexpr int IMG = KT * RB;            // one K (or V) tile image (lds_off<D> layout)
  static constexpr int SLOT = 2 * IMG;           // K | V
#ifndef PICO_Q_NBUF64
#define PICO_Q_NBUF64 3
#endif
  static constexpr int NBUF = D == 64 ? PICO_Q_NBUF64 : 2;   // ring slots; prefetch NBUF - 1
  static constexpr int RPP = 1024 / RB;        // image rows per 1-KiB DMA piece
  static constexpr int NP = SLOT / 1024;       // pieces per tile
  static constexpr int NPW = NP / 4;           // per wave
};

// (Round 5 measured and removed a pipelined form of this tile — the two 32-key halves as one hand-ordered stream
// of 24 MFMA slots at two workgroups per CU, as attn_bwd_kvp_kernel: C2 40.5 vs 40.6 us, profiles/r05_ab_kvp_qp.jsonl.)
template <int D, bool CAUSAL>
__global__ __launch_bounds__(256, QCfg<D>::MINB) void attn_bwd_q_kernel(const pico_attn_args a, float scale, float scale_log2,
                                                             float* __restrict__ lse2_g, float* __restrict__ delta_g,
                                                             int sq_pad, unsigned long long* __restrict__ stamp_out,
                                                             int nfront, float lse_mul, float lse_pad) {
  using C = QCfg<D>;
#if PICO_BWDQ_WGSTAMP
  unsigned long long wgs[4];
  wgs[0] = __builtin_amdgcn_s_memrealtime();
#endif
  constexpr int KS = C::KS, DT = C::DT, RB = C::RB;
  __shared__ __attribute__((aligned(16))) char smem[C::NBUF * C::SLOT];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int Sq = (int)a.seqlen_q, Sk = (int)a.seqlen_k;

  // causal dispatch order (a head's blocks sit nbh block ids apart): the `nfront` lightest query blocks
  // first, then the rest heaviest-first. nfront = the blocks a heaviest-first order leaves for after the
  // first round of resident workgroups: run there, in a near-empty chip, each paid its whole prologue
  // latency alone (C2: blocks 0-1 started at 27-29 us and ended at 36 of 40); run first (oldest, so
  // favoured by the SIMD arbitration) they finish early and hand their slots to the heavy blocks.
  const int nmb = (Sq + QB - 1) / QB;
  const int nbh = (int)(a.batch * a.heads_q);
  const int lin = blockIdx.x;
  const int gi = lin / nbh;
  const int mb = !CAUSAL ? gi : (gi < nfront ? gi : nmb - 1 - (gi - nfront));
  const int bh = lin % nbh;
  const int b = bh / (int)a.heads_q, hq = bh % (int)a.heads_q;
  const int hk = hq / (int)(a.heads_q / a.heads_kv);
  const int q0 = mb * QB, qw = q0 + 32 * wave, my_q = qw + r;
  const int qc = min(my_q, Sq - 1);

  const bf16_t* kg = (const bf16_t*)a.k + b * a.k_strides[0] + hk * a.k_strides[2];
  const bf16_t* vg = (const bf16_t*)a.v + b * a.v_strides[0] + hk * a.v_strides[2];
  const int64_t ksd = a.k_strides[1], vsd = a.v_strides[1];

  int kend = Sk;
  if (CAUSAL) kend = min(Sk, q0 + QB);
  const int ntiles = (kend + KT - 1) / KT;
  const int lim_last = CAUSAL ? min(qw + 31, Sk - 1) : Sk - 1;   // last key any row of the wave sees
  const int lim_first = CAUSAL ? min(qw, Sk - 1) : Sk - 1;       // keys <= this need no mask
  const int lim_lane = CAUSAL ? min(my_q, Sk - 1) : Sk - 1;      // this lane's row sees keys <= it

  // ---- DMA: piece j = wave + 4 i of a tile; j < NP/2: K image piece j, else V image piece j - NP/2 ----
  int src_row[C::NPW], src_col[C::NPW];
  unsigned dst_off[C::NPW];
  bool is_k[C::NPW];
#pragma unroll
  for (int i = 0; i < C::NPW; ++i) {
    const int j = wave + 4 * i;
    is_k[i] = j < C::NP / 2;
    const int jj = is_k[i] ? j : j - C::NP / 2;
    const int row = C::RPP * jj + lane / C::CPR;
    src_row[i] = row;
    src_col[i] = 8 * ((lane % C::CPR) ^ swz<D>(row));
    dst_off[i] = (is_k[i] ? 0u : (unsigned)C::IMG) + (unsigned)jj * 1024u;
  }
  const unsigned smem_lds = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr(smem));
  unsigned full_off[C::NPW];  // per-lane byte offsets within a full tile (computed once)
#pragma unroll
  for (int i = 0; i < C::NPW; ++i) full_off[i] = (unsigned)(src_row[i] * (is_k[i] ? ksd : vsd) + src_col[i]) * 2u;
  // K and V tile rows advance by constant byte strides: wave-uniform pointers, bumped per tile
  const int64_t kst = (int64_t)KT * ksd * 2, vst = (int64_t)KT * vsd * 2;
  const char* kp_nxt = (const char*)kg;
  const char* vp_nxt = (const char*)vg;
  auto issue_piece = [&](int tile, int slot_i, int i) __attribute__((always_inline)) {
    const unsigned slot = smem_lds + (unsigned)slot_i * (unsigned)C::SLOT;
    const int base = tile * KT;
    const int lastrow = Sk - 1 - base;  // rows past it are clamped (finite; masked by the softmax)
    const bool full = base + KT <= Sk;
    const char* tb = is_k[i] ? kp_nxt : vp_nxt;
    const unsigned off = full ? full_off[i]
                              : (unsigned)(min(src_row[i], lastrow) * (is_k[i] ? ksd : vsd) + src_col[i]) * 2u;
    dma_piece(tb, off, slot + dst_off[i]);
  };
  auto bump = [&]() __attribute__((always_inline)) {
    kp_nxt += kst;
    vp_nxt += vst;
  };
  auto issue = [&](int tile, int slot_i) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < C::NPW; ++i) issue_piece(tile, slot_i, i);
    bump();
  };
  constexpr int P = C::NBUF - 1;  // prefetch distance
#pragma unroll
  for (int t = 0; t < P; ++t)
    if (t < ntiles) issue(t, t);

  // ---- Q, dO fragments (B operands), delta = rowsum(dO * O), LSE ----
  bf16x8 qf[KS], df[KS];
  float dsum = 0.f;
  {
    const int64_t qoff = b * a.q_strides[0] + hq * a.q_strides[2] + (int64_t)qc * a.q_strides[1] + 8 * h;
    const int64_t dooff = b * a.do_strides[0] + hq * a.do_strides[2] + (int64_t)qc * a.do_strides[1] + 8 * h;
    const int64_t ooff = b * a.o_strides[0] + hq * a.o_strides[2] + (int64_t)qc * a.o_strides[1] + 8 * h;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const u16x8 qv = *reinterpret_cast<const u16x8*>((const bf16_t*)a.q + qoff + 16 * ks);
      const u16x8 dv = *reinterpret_cast<const u16x8*>((const bf16_t*)a.dout + dooff + 16 * ks);
      const u16x8 ov = *reinterpret_cast<const u16x8*>((const bf16_t*)a.o + ooff + 16 * ks);
      qf[ks] = __builtin_bit_cast(bf16x8, qv);
      df[ks] = __builtin_bit_cast(bf16x8, dv);
#pragma unroll
      for (int j = 0; j < 8; ++j) dsum += bf2f(ov[j]) * bf2f(dv[j]);
    }
  }
  // consume the prologue loads here: otherwise the compiler's own vmcnt waits for them sit at their
  // first use inside the tile loop, where vmcnt also counts the ring's in-flight DMA (-> vmcnt(0) per tile)
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]), "+v"(df[ks]));
  const float dall = halves_sum2(dsum);
  const bool row_ok = my_q < Sq;
  const float delta = row_ok ? dall : 0.f;
  const float lse2 = row_ok ? a.lse[((int64_t)b * a.heads_q + hq) * Sq + my_q] * LOG2E : INFINITY;
  if (h == 0 && my_q < sq_pad) {  // for the dK/dV kernel (padding rows: P = 0, delta = 0)
    // attn_bwd_kv_kernel: LSE log2 e (+inf padding); attn_bwd_kvp_kernel: -LSE / scale (-inf padding)
    lse2_g[(int64_t)bh * sq_pad + my_q] = row_ok ? a.lse[((int64_t)b * a.heads_q + hq) * Sq + my_q] * lse_mul : lse_pad;
    delta_g[(int64_t)bh * sq_pad + my_q] = -delta;
  }

  // per-lane LDS offsets, pinned in registers (the compiler would otherwise re-derive the swizzles)
  unsigned ro[KS], tro[DT][2];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) ro[ks] = lds_off<D>(r, 2 * ks + h);
  tr_offsets<D>(lane, tro);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(ro[ks]));
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) asm volatile("" : "+v"(tro[dt][0]), "+v"(tro[dt][1]));

  f32x16 dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dq[dt] = (f32x16)0.f;
  const f32x16 ndelta = (f32x16)(-delta);
  const float nl2 = -lse2;

  // One 64-key tile: S^T, dP^T (8 + 8 MFMAs), P^T and dS^T in registers, dQ^T += K^T dS^T (8 MFMAs).
  // kb: the slot's K image (V image at +IMG). One body for every tile (the causal / padding mask is an
  // in-place branch on S), so the loop-carried dQ accumulators never move between registers.
  // the two 32-key halves of a tile one after the other (half the K / V fragments and S / dP registers
  // live at a time: room for a third workgroup per CU at D = 64)
  auto tile = [&](const char* kb, bool mask, int n0) __attribute__((always_inline)) {
    const char* vb = kb + C::IMG;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      // D = 128 at two workgroups per CU (248 VGPRs): V's fragments are read after the S chain has
      // consumed K's (32 fewer live VGPRs)
      constexpr bool seqv = D == 128;
      bf16x8 kf[KS], vf[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        kf[ks] = lds_read_b128(kb, ro[ks] + kt * 32 * RB);
        if (!seqv) vf[ks] = lds_read_b128(vb, ro[ks] + kt * 32 * RB);
      }
      f32x16 sc, dpc;
      if (mask) {
        const int rel = lim_lane - n0 - 4 * h;
        f32x16 m;
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] = (32 * kt + (i & 3) + 8 * (i >> 2)) <= rel ? 0.f : -INFINITY;
        sc = mfma32(kf[0], qf[0], m);
      } else {
        sc = mfma32(kf[0], qf[0], (f32x16)0.f);
      }
#pragma unroll
      for (int ks = 1; ks < KS; ++ks) sc = mfma32(kf[ks], qf[ks], sc);
      if constexpr (seqv) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) vf[ks] = lds_read_b128(vb, ro[ks] + kt * 32 * RB);
      }
      dpc = mfma32(vf[0], df[0], ndelta);
#pragma unroll
      for (int ks = 1; ks < KS; ++ks) dpc = mfma32(vf[ks], df[ks], dpc);
      float ds[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) ds[i] = fast_exp2(__builtin_fmaf(sc[i], scale_log2, nl2)) * dpc[i];
      const bf16x8 dsf[2] = {pack_bf16x8(ds), pack_bf16x8(ds + 8)};
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const char* rowb = kb + (32 * kt + 16 * st) * RB;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dq[dt] = mfma32(tr_pair(rowb, tro[dt][0], tro[dt][1]), dsf[st], dq[dt]);
      }
    }
  };
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // prologue tiles and loads landed
#if PICO_BWDQ_WGSTAMP
  wgs[1] = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
#endif
  // unrolled by the ring depth: every LDS read of a tile has a compile-time slot (immediate offsets)
  for (int t0 = 0; t0 < ntiles; t0 += C::NBUF) {
#pragma unroll
    for (int u = 0; u < C::NBUF; ++u) {
      const int t = t0 + u;
      if (t >= ntiles) break;
      if (t > 0) {  // tile t landed (this wave's pieces); the younger tiles stay in flight
        if constexpr (P == 2) {  // counts as immediates (a runtime wait_vmcnt(n) is a compare-and-branch chain)
          if (t + 1 < ntiles) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NPW) : "memory");
          else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if constexpr (P == 1) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
          wait_vmcnt(min(P - 1, ntiles - 1 - t) * C::NPW);  // issued tiles after t stay in flight
        }
      }
      lds_barrier();  // every wave's pieces of tile t visible; slot (t + P) % NBUF no longer read
      const int n0 = t * KT;
      const bool busy = n0 <= lim_last;  // wave-uniform: some row of the wave sees some key of the tile
      if (t + P < ntiles) issue(t + P, (u + P) % C::NBUF);
      if (busy) tile(smem + u * C::SLOT, n0 + KT - 1 > lim_first, n0);
    }
  }

#if PICO_BWDQ_WGSTAMP
  wgs[2] = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
#endif
  // ---- epilogue: lane = query my_q, register i of tile dt = d 32 dt + acc_row(i, h) ----
  // (every lane stays: the bf16 store's lane exchange needs the whole wave; only row_ok lanes store)
  if (a.flags & PICO_ATTN_ROPE_BWD) {  // rotate back by -theta: pairs (d, d + D/2) = tiles (dt, dt + DT/2)
    const bf16_t* cp = (const bf16_t*)a.rope_cos + (int64_t)qc * a.rope_stride;
    const bf16_t* sp = (const bf16_t*)a.rope_sin + (int64_t)qc * a.rope_stride;
#pragma unroll
    for (int dt = 0; dt < DT / 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const u16x4 c4 = *reinterpret_cast<const u16x4*>(cp + 32 * dt + 8 * g + 4 * h);
        const u16x4 s4 = *reinterpret_cast<const u16x4*>(sp + 32 * dt + 8 * g + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float cf = bf2f(c4[j]), sf = bf2f(s4[j]);
          const float x1 = dq[dt][4 * g + j], x2 = dq[dt + DT / 2][4 * g + j];
          dq[dt][4 * g + j] = x1 * cf + x2 * sf;
          dq[dt + DT / 2][4 * g + j] = x2 * cf - x1 * sf;
        }
      }
  }
  if (a.flags & PICO_ATTN_DQ_F32_ACCUM) {
    if (row_ok) {
      float* dst = (float*)a.dq + b * a.dq_strides[0] + hq * a.dq_strides[2] + (int64_t)my_q * a.dq_strides[1];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float* p = dst + 32 * dt + 8 * g + 4 * h;
#pragma unroll
          for (int j = 0; j < 4; ++j) p[j] += dq[dt][4 * g + j] * scale;
        }
    }
  } else {
    bf16_t* dst = (bf16_t*)a.dq + b * a.dq_strides[0] + hq * a.dq_strides[2] + (int64_t)qc * a.dq_strides[1];
    store_row_bf16_x16<DT>(dst, h, row_ok, [&](int dt, int i) { return dq[dt][i] * scale; });
  }
#if PICO_BWDQ_WGSTAMP
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  wgs[3] = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  if (wave == 0 && lane < 4 && blockIdx.x < 65536) stamp_out[blockIdx.x * 4 + lane] = wgs[lane & 3];
#endif
}

}  // namespace

int attn_bwd_q_launch(const pico_attn_args* a, const SplitPlan& p, hipStream_t s) {
  const auto kernel = a->head_dim == 64 ? (a->causal ? attn_bwd_q_kernel<64, true> : attn_bwd_q_kernel<64, false>)
                                        : (a->causal ? attn_bwd_q_kernel<128, true> : attn_bwd_q_kernel<128, false>);
  // the LSE form the dK/dV kernel reads: LSE log2 e (+inf padding rows) for the 32-row one, -LSE / scale (-inf) for the 64-row ones
  return pico_launch(PICO_K_ATTN_BWD_Q, "attn_bwd_q", kernel, dim3((int)p.q_grid), dim3(256), 0, s, *a,
                     a->softmax_scale, a->softmax_scale * LOG2E, split_ws<float>(a, p.lse2_off),
                     split_ws<float>(a, p.delta_off), p.sq_pad, split_ws<unsigned long long>(a, p.stamp_off), p.q_front,
                     p.kvp ? -1.0f / a->softmax_scale : LOG2E, p.kvp ? -INFINITY : INFINITY);
}
