// Split flash-attention backward (attn_bwd_split.hip), the 32-row dK/dV kernel (key-major; D = 64 beyond 1536
// causal / 4096 non-causal keys, and the A/B partner of the 64-row kernels: attn_bwd_plan.h kvp_enabled):
//   attn_bwd_kv_kernel: one workgroup = 4 waves x 32 keys = 128 keys of one (batch, kv-head),
//     sweeping (query head of the group) x 32-row query tiles (Q, dO, LSE/delta by LDS-DMA). Key on
//     the lane: S = Q K^T, dP = dO V^T (K, V fragments resident in registers), then dV^T += dO^T P and
//     dK^T += Q^T dS with the P / dS accumulators as B operands (no LDS round trip at all).
// RoPE^-1 (PICO_ATTN_ROPE_BWD) is applied in the epilogue, register-local as in the dQ kernel.
// The workgroup: 128 keys = 4 waves (one per SIMD) of 32 keys. Two or three workgroups resident per CU
// (kv_minb) overlap one's prologue (K/V fragments, first tiles) and epilogue (dK/dV stores) with the others' main
// loops, which the 8-wave 256-key form (one workgroup per CU) could not: C2 causal 62 vs 68 us. Measured and
// dropped: 64 keys per wave (69-71 vs 52 us), a tile-pipelined body carrying S / dP of tile
// t + 1 across the barrier (+6 % at D = 64, noise at D = 128), two tiles per barrier interval.
#include "attn_bwd_split.h"

namespace {

template <int D>
struct KVCfg {
  static constexpr int KS = D / 16, DT = D / 32, CPR = D / 8, RB = 2 * D;
  static constexpr int QIMG = QT * RB;   // one Q (or dO) tile image
  static constexpr int LSD = 1024;       // LSE*log2e [32] | -delta [32] (one DMA piece)
  static constexpr int SLOT = 2 * QIMG + LSD;
#ifndef PICO_KV_NBUF
#define PICO_KV_NBUF 3
#endif
  static constexpr int NBUF = PICO_KV_NBUF;  // ring slots
  static constexpr int PD = NBUF - 1;        // prefetch distance (tiles)
  static constexpr int RPP = 1024 / RB;
  static constexpr int NQP = QIMG / 1024;
  static constexpr int NP = 2 * NQP + 1;
  static constexpr int NPW = (NP + KNW - 1) / KNW;
};

template <int D, bool CAUSAL, int MINB>
__global__ __launch_bounds__(KNW * 64, MINB) void attn_bwd_kv_kernel(const pico_attn_args a, float scale, float scale_log2,
                                                              const float* __restrict__ lse2_g,
                                                              const float* __restrict__ delta_g, int sq_pad,
                                                              int hsplit, float* __restrict__ dkv_part,
                                                              unsigned long long* __restrict__ stamp_out,
                                                              const BlkGroups grp) {
  using C = KVCfg<D>;
  constexpr int KS = C::KS, DT = C::DT, CPR = C::CPR, RB = C::RB;
  __shared__ __attribute__((aligned(16))) char smem[C::NBUF * C::SLOT];

  const int lane0 = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int Sq = (int)a.seqlen_q, Sk = (int)a.seqlen_k;
  const int Hq = (int)a.heads_q;
  const int G = (int)(a.heads_q / a.heads_kv);
#if PICO_BWDKV_WGSTAMP
  unsigned long long wgs[4];
  wgs[0] = __builtin_amdgcn_s_memrealtime();
#endif

  // heaviest key blocks first (causal: block 0 sees every query; lightest-first fronts as in the dQ kernel
  // measured neutral here); small grids split a key block's (query head, query tile) list over `hsplit`
  // workgroups with fp32 partials (attn_bwd_dkv_kernel sums)
  const int nbh = (int)(a.batch * a.heads_kv) * hsplit;
  const int gi = blockIdx.x / nbh;  // the key block, or with a one-round schedule (grp.n > 0) the block group
  const int bhs = blockIdx.x % nbh;
  const int hs = bhs % hsplit;
  const int bh = bhs / hsplit;
  const int b = bh / (int)a.heads_kv, hk = bh % (int)a.heads_kv;
  // the group's key blocks one after the other (grp.n == 0: the one block gi)
  const unsigned gw = grp.n ? grp_sel(grp, gi) : 0u;
  const int nblk_wg = grp.n ? (int)((grp.cnt >> (4 * gi)) & 15ull) : 1;
#pragma clang loop unroll(disable)
  for (int jb = 0; jb < nblk_wg; ++jb) {
  const int kb = grp.n ? (int)((gw >> (8 * jb)) & 255u) : gi;
  if (jb > 0) lds_barrier();  // every wave is done with the ring before this block's prologue DMA refills it
  // the lane id through an opaque copy: nothing lane-dependent is hoisted out of the block loop and kept live
  // across the whole body (that cost 100-180 B of scratch per lane at these register budgets)
  int lane_l = lane0;
  asm volatile("" : "+v"(lane_l));
  const int lane = lane_l, r = lane & 31, h = lane >> 5;
  const int k0 = kb * KVB;
  const int kw = k0 + KPW * wave;  // this wave's first key

  const int qstart = CAUSAL ? k0 : 0;  // k0 is a multiple of QT
  const int nqt = Sq > qstart ? (Sq - qstart + QT - 1) / QT : 0;
  const int ntot = G * nqt;
  const int tb = (int)((int64_t)ntot * hs / hsplit);
  const int ntiles = (int)((int64_t)ntot * (hs + 1) / hsplit) - tb;
  const int hq0 = hk * G + (nqt ? tb / nqt : 0), q00 = qstart + (nqt ? tb % nqt : 0) * QT;

  // ---- tile DMA: piece j = wave + KNW i: Q pieces, dO pieces, then the LSE/delta piece ----
  int pc_row[C::NPW], pc_col[C::NPW], pc_kind[C::NPW];
  unsigned pc_dst[C::NPW];
#pragma unroll
  for (int i = 0; i < C::NPW; ++i) {
    const int j = wave + KNW * i;  // wave-uniform
    if (j < 2 * C::NQP) {
      const int jj = j % C::NQP, row = C::RPP * jj + lane / CPR;
      pc_kind[i] = j < C::NQP ? 0 : 1;
      pc_row[i] = row;
      pc_col[i] = 8 * ((lane % CPR) ^ swz<D>(row));
      pc_dst[i] = (j < C::NQP ? 0 : C::QIMG) + jj * 1024;
    } else {  // lanes 0-7: LSE*log2e rows 4l..4l+3; 8-15: -delta rows (16-63 repeat)
      const int l = lane & 15;
      pc_kind[i] = 2;
      pc_row[i] = 4 * (l & 7);
      pc_col[i] = l >> 3;
      pc_dst[i] = 2 * C::QIMG;
    }
  }
  // A tile = (query head hq, 32 query rows from q0). Each of this wave's pieces reads from one wave-uniform
  // source pointer (Q rows, dO rows or the lse2 row) advanced by a constant stride per tile: the per-tile
  // issue is one DMA instruction per piece (no 64-bit index arithmetic and no source select in the loop).
  const int64_t qs1 = a.q_strides[1] * 2, ds1 = a.do_strides[1] * 2;  // bytes per query row
  const char* const qbase = (const char*)((const bf16_t*)a.q + b * a.q_strides[0]);
  const char* const dobase = (const char*)((const bf16_t*)a.dout + b * a.do_strides[0]);
  int64_t pc_step[C::NPW];  // bytes per tile of piece i's source
#pragma unroll
  for (int i = 0; i < C::NPW; ++i) pc_step[i] = pc_kind[i] == 0 ? QT * qs1 : (pc_kind[i] == 1 ? QT * ds1 : QT * 4);
  struct Tc {
    int hq, q0;
    const char* p[C::NPW];
  };
  auto make_tc = [&](int hq, int q0) __attribute__((always_inline)) {
    Tc c;
    c.hq = hq;
    c.q0 = q0;
#pragma unroll
    for (int i = 0; i < C::NPW; ++i)
      c.p[i] = pc_kind[i] == 0 ? qbase + hq * a.q_strides[2] * 2 + q0 * qs1
             : pc_kind[i] == 1 ? dobase + hq * a.do_strides[2] * 2 + q0 * ds1
                               : (const char*)(lse2_g + ((int64_t)b * Hq + hq) * sq_pad + q0);
    return c;
  };
  const int qend = qstart + nqt * QT;
  auto advance = [&](Tc& c) __attribute__((always_inline)) {
    if (c.q0 + QT >= qend) {
      c = make_tc(c.hq + 1, qstart);
    } else {
      c.q0 += QT;
#pragma unroll
      for (int i = 0; i < C::NPW; ++i) c.p[i] += pc_step[i];
    }
  };
  const unsigned delta_off = (unsigned)((const char*)delta_g - (const char*)lse2_g);  // same workspace
  const unsigned ring_lds = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr(smem));
  // per-lane byte offsets of this wave's pieces within a full tile (computed once; partial tiles clamp)
  unsigned pc_off[C::NPW];
#pragma unroll
  for (int i = 0; i < C::NP / KNW; ++i) pc_off[i] = (unsigned)(pc_row[i] * (pc_kind[i] == 0 ? qs1 : ds1) + pc_col[i] * 2);
  const bool ragged = Sq % QT != 0;
  auto issue = [&](int si, const Tc& c) __attribute__((always_inline)) {
    const unsigned dst = ring_lds + (unsigned)si * (unsigned)C::SLOT;
#pragma unroll
    for (int i = 0; i < C::NPW; ++i) {
      if (i < C::NP / KNW) {
        unsigned off = pc_off[i];
        if (ragged && c.q0 + QT > Sq && pc_kind[i] != 2)  // partial tile: clamp rows past Sq - 1
          off = (unsigned)((min(c.q0 + pc_row[i], Sq - 1) - c.q0) * (pc_kind[i] == 0 ? qs1 : ds1) + pc_col[i] * 2);
        dma_piece(c.p[i], off, dst + pc_dst[i]);
      } else if (wave < C::NP % KNW) {
        // the tile's LSE / delta piece (wave 0 only, pc_kind 2): its per-lane offset is re-derived from the lane
        // id here instead of being held in a VGPR for the whole sweep — at 168 VGPRs that VGPR was spilled, and
        // its scratch reload's vmcnt(0) drained wave 0's whole DMA queue (two tiles of prefetch) every tile
        static_assert(C::NP % KNW == 1 && C::NP / KNW == C::NPW - 1, "the LSE / delta piece is wave 0's last");
        // (from an opaque copy of the lane id: a plain __lane_id() expression is loop-invariant and gets hoisted
        // out of the tile loop into that same long-lived, spilled VGPR)
        int l = lane0;
        asm volatile("" : "+v"(l));
        l &= 15;
        dma_piece(c.p[i], (unsigned)(16 * (l & 7)) + ((l >> 3) ? delta_off : 0u), dst + pc_dst[i]);
      }
    }
  };
  constexpr int PD = C::PD;
  Tc nxt = make_tc(hq0, q00);
#pragma unroll
  for (int j = 0; j < PD; ++j) {
    if (j < ntiles) issue(j, nxt);
    advance(nxt);
  }

  // ---- K, V fragments of this wave's 64 keys (B operands of S = Q K^T, dP = dO V^T) ----
  const bf16_t* kg = (const bf16_t*)a.k + b * a.k_strides[0] + hk * a.k_strides[2];
  const bf16_t* vg = (const bf16_t*)a.v + b * a.v_strides[0] + hk * a.v_strides[2];
  bf16x8 kf[KH][KS], vf[KH][KS];
#pragma unroll
  for (int kt = 0; kt < KH; ++kt) {
    const int key = kw + 32 * kt + r;
    const bool ok = key < Sk;
    const bf16_t* kp = kg + (int64_t)min(key, Sk - 1) * a.k_strides[1] + 8 * h;
    const bf16_t* vp = vg + (int64_t)min(key, Sk - 1) * a.v_strides[1] + 8 * h;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const u16x8 kv = *reinterpret_cast<const u16x8*>(kp + 16 * ks);
      const u16x8 vv = *reinterpret_cast<const u16x8*>(vp + 16 * ks);
      kf[kt][ks] = __builtin_bit_cast(bf16x8, ok ? kv : (u16x8)0);
      vf[kt][ks] = __builtin_bit_cast(bf16x8, ok ? vv : (u16x8)0);
    }
  }

  // consume the loads before the loop (see attn_bwd_q_kernel)
#pragma unroll
  for (int kt = 0; kt < KH; ++kt)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(kf[kt][ks]), "+v"(vf[kt][ks]));

  f32x16 dk[DT][KH], dv[DT][KH];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int kt = 0; kt < KH; ++kt) {
      dk[dt][kt] = (f32x16)0.f;
      dv[dt][kt] = (f32x16)0.f;
    }

  unsigned qo[KS], tro[DT][2];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qo[ks] = lds_off<D>(r, 2 * ks + h);
  tr_offsets<D>(lane, tro);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qo[ks]));
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) asm volatile("" : "+v"(tro[dt][0]), "+v"(tro[dt][1]));

  const bool kpad = kw + KPW - 1 >= Sk;  // wave-uniform: some of the wave's keys are padding
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // prologue tiles visible
#if PICO_BWDKV_WGSTAMP
  wgs[1] = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
#endif

  // One 32-query tile = M1 (S = Q K^T and dP = dO V^T - delta: 8 MFMAs, mask and -delta in the C operand),
  // then V (P = exp2(S scale log2e - LSE log2e), dS = P dP: VALU) and M2 (dV^T += dO^T P, dK^T += Q^T dS:
  // 8 MFMAs with the packed accumulators as B operands). A tile wholly above the wave's keys (causal) is
  // masked to P = 0 rather than skipped (no per-wave branch around the body).
  auto m1 = [&](int si, int q0, f32x16 (&s)[KH], f32x16 (&dp)[KH]) __attribute__((always_inline)) {
    const char* qs = smem + (unsigned)si * (unsigned)C::SLOT;
    const char* dos = qs + C::QIMG;
    const float* lsd = (const float*)(qs + 2 * C::QIMG);
    bf16x8 qa[KS], da[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      qa[ks] = lds_read_b128(qs, qo[ks]);
    }
    f32x16 nd;  // rows of this lane's accumulator registers: q = q0 + 8 g + 4 h + (0..3)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(lsd + 32 + 8 * g + 4 * h);
#pragma unroll
      for (int j = 0; j < 4; ++j) nd[4 * g + j] = v[j];
    }
    // The causal / padding mask enters as the C operand of each S chain's first MFMA (-inf where key > q or
    // key >= Sk, else 0): the branch covers only those MFMAs, the rest of the tile is straight-line code.
    if ((CAUSAL && kw + KPW - 1 > q0) || kpad) {  // wave-uniform: diagonal / wholly masked tiles, padding keys
#pragma unroll
      for (int kt = 0; kt < KH; ++kt) {
        const int key = kw + 32 * kt + r;
        // masked iff (i&3) + 8(i>>2) < rel: causal key > q, or every row for a padding key
        const int rel = key >= Sk ? 64 : (CAUSAL ? key - q0 - 4 * h : -1);
        f32x16 m;
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] = ((i & 3) + 8 * (i >> 2) < rel) ? -INFINITY : 0.f;
        s[kt] = mfma32(qa[0], kf[kt][0], m);
      }
    } else {
#pragma unroll
      for (int kt = 0; kt < KH; ++kt) s[kt] = mfma32(qa[0], kf[kt][0], (f32x16)0.f);
    }
    // the dO fragments are read once the S chain has consumed Q's (16 fewer live VGPRs: room for a third
    // workgroup per CU; C2 58.5 -> 56.1 us at two)
#pragma unroll
    for (int kt = 0; kt < KH; ++kt)
#pragma unroll
      for (int ks = 1; ks < KS; ++ks) s[kt] = mfma32(qa[ks], kf[kt][ks], s[kt]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) da[ks] = lds_read_b128(dos, qo[ks]);
#pragma unroll
    for (int kt = 0; kt < KH; ++kt) {
      dp[kt] = mfma32(da[0], vf[kt][0], nd);
#pragma unroll
      for (int ks = 1; ks < KS; ++ks) dp[kt] = mfma32(da[ks], vf[kt][ks], dp[kt]);
    }
  };
  // V: P = exp2(S scale log2e - LSE log2e), dS = P dP, packed to bf16 (the B operands of M2)
  auto read_l2 = [&](int si, f32x4 (&l2)[4]) __attribute__((always_inline)) {
    const float* lsd = (const float*)(smem + (unsigned)si * (unsigned)C::SLOT + 2 * C::QIMG);
#pragma unroll
    for (int g = 0; g < 4; ++g) l2[g] = *reinterpret_cast<const f32x4*>(lsd + 8 * g + 4 * h);
  };
  auto vsm_l2 = [&](const f32x4 (&l2)[4], const f32x16 (&s)[KH], const f32x16 (&dp)[KH], bf16x8 (&pf)[KH][2],
                    bf16x8 (&sf)[KH][2]) __attribute__((always_inline)) {
#pragma unroll
    for (int kt = 0; kt < KH; ++kt) {
      float pv[16], sv[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        pv[i] = fast_exp2(__builtin_fmaf(s[kt][i], scale_log2, -l2[i >> 2][i & 3]));
        sv[i] = pv[i] * dp[kt][i];
      }
      pf[kt][0] = pack_bf16x8(pv);
      pf[kt][1] = pack_bf16x8(pv + 8);
      sf[kt][0] = pack_bf16x8(sv);
      sf[kt][1] = pack_bf16x8(sv + 8);
    }
  };
  auto vsm = [&](int si, const f32x16 (&s)[KH], const f32x16 (&dp)[KH], bf16x8 (&pf)[KH][2], bf16x8 (&sf)[KH][2])
      __attribute__((always_inline)) {
    f32x4 l2[4];
    read_l2(si, l2);
    vsm_l2(l2, s, dp, pf, sf);
  };
  // M2: dV^T[d][key] += dO^T[d][q] P[q][key], dK^T[d][key] += Q^T[d][q] dS[q][key] (A = transposed reads)
  auto m2 = [&](int si, const bf16x8 (&pf)[KH][2], const bf16x8 (&sf)[KH][2]) __attribute__((always_inline)) {
    const char* qs = smem + (unsigned)si * (unsigned)C::SLOT;
    const char* dos = qs + C::QIMG;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 dot = tr_pair(dos + 16 * st * RB, tro[dt][0], tro[dt][1]);
        const bf16x8 qt = tr_pair(qs + 16 * st * RB, tro[dt][0], tro[dt][1]);
#pragma unroll
        for (int kt = 0; kt < KH; ++kt) {
          dv[dt][kt] = mfma32(dot, pf[kt][st], dv[dt][kt]);
          dk[dt][kt] = mfma32(qt, sf[kt][st], dk[dt][kt]);
        }
      }
  };

  // Unrolled by the ring depth: the slot of every LDS read is a compile-time constant (immediate offsets).
  // (Measured and dropped, C2 causal: a stagger of the two waves of each SIMD by one phase — +2 %; carrying
  // S / dP of tile t + 1 across the barrier so M1(t + 1) overlaps V(t) inside the wave — +6 %.)
  constexpr int NPMY_LO = C::NP / KNW;  // this wave's pieces per tile: NPMY_LO or NPMY_LO + 1
  int q0cur = q00;
  for (int t0 = 0; t0 < ntiles; t0 += C::NBUF) {
#pragma unroll
    for (int u = 0; u < C::NBUF; ++u) {
      const int t = t0 + u;
      if (t >= ntiles) break;
      if (t > 0) {
        if constexpr (C::PD == 2) {
          if (t + 2 <= ntiles) {  // this wave's pieces of tile t landed; the next tile's may stay in flight
            if (wave < C::NP % KNW) wait_vmcnt(NPMY_LO + 1);
            else wait_vmcnt(NPMY_LO);
          } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          }
        } else {
          const int younger = min(C::PD - 1, ntiles - 1 - t);  // issued tiles after t (still in flight)
          wait_vmcnt(younger * (wave < C::NP % KNW ? NPMY_LO + 1 : NPMY_LO));
        }
        lds_barrier();  // everyone's pieces visible; the slot of tile t - 1 is no longer read
      }
      if (t + PD < ntiles) issue((u + PD) % C::NBUF, nxt);
      advance(nxt);
      f32x16 s[KH], dp[KH];
      bf16x8 pf[KH][2], sf[KH][2];
      m1(u, q0cur, s, dp);
      if constexpr (D == 128) {
        // one wave per SIMD: nothing else hides the transposed reads' LDS latency, so all of M2's A operands
        // (2 x DT x 2 fragments, 64 VGPRs) are requested before the softmax VALU instead of just before their MFMAs
        // (C4 dK/dV 46.8-47.1 -> 45.3-45.4 us, S 4096 166-170 -> 161-164; profiles/r04_ab_kv_m2pre_d128.jsonl)
        const char* qs = smem + (unsigned)u * (unsigned)C::SLOT;
        const char* dos = qs + C::QIMG;
        f32x4 l2[4];
        read_l2(u, l2);
        bf16x8 od[2][DT], oq[2][DT];
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            od[st][dt] = tr_pair(dos + 16 * st * RB, tro[dt][0], tro[dt][1]);
            oq[st][dt] = tr_pair(qs + 16 * st * RB, tro[dt][0], tro[dt][1]);
          }
        __builtin_amdgcn_sched_barrier(0);
        vsm_l2(l2, s, dp, pf, sf);
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int kt = 0; kt < KH; ++kt) {
              dv[dt][kt] = mfma32(od[st][dt], pf[kt][st], dv[dt][kt]);
              dk[dt][kt] = mfma32(oq[st][dt], sf[kt][st], dk[dt][kt]);
            }
      } else {
        vsm(u, s, dp, pf, sf);
        m2(u, pf, sf);
      }
      q0cur = q0cur + QT >= qend ? qstart : q0cur + QT;
    }
  }

#if PICO_BWDKV_WGSTAMP
  wgs[2] = __builtin_amdgcn_s_memrealtime();
#endif
  // ---- epilogue: lane = key kw + 32 kt + r, register i of tile dt = d 32 dt + acc_row(i, h) ----
  if (hsplit == 1) {
    const bool rope = (a.flags & PICO_ATTN_ROPE_BWD) != 0;
#pragma unroll
    for (int kt = 0; kt < KH; ++kt) {
      const int key = kw + 32 * kt + r;
      const int kc = min(key, Sk - 1);  // every lane runs the stores' lane exchange; only key < Sk store
      if (rope) {
        const bf16_t* cp = (const bf16_t*)a.rope_cos + (int64_t)kc * a.rope_stride;
        const bf16_t* sp = (const bf16_t*)a.rope_sin + (int64_t)kc * a.rope_stride;
#pragma unroll
        for (int dt = 0; dt < DT / 2; ++dt)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const u16x4 c4 = *reinterpret_cast<const u16x4*>(cp + 32 * dt + 8 * g + 4 * h);
            const u16x4 s4 = *reinterpret_cast<const u16x4*>(sp + 32 * dt + 8 * g + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float cf = bf2f(c4[j]), sn = bf2f(s4[j]);
              const float x1 = dk[dt][kt][4 * g + j], x2 = dk[dt + DT / 2][kt][4 * g + j];
              dk[dt][kt][4 * g + j] = x1 * cf + x2 * sn;
              dk[dt + DT / 2][kt][4 * g + j] = x2 * cf - x1 * sn;
            }
          }
      }
      bf16_t* dkp = (bf16_t*)a.dk + b * a.dk_strides[0] + hk * a.dk_strides[2] + (int64_t)kc * a.dk_strides[1];
      bf16_t* dvp = (bf16_t*)a.dv + b * a.dv_strides[0] + hk * a.dv_strides[2] + (int64_t)kc * a.dv_strides[1];
      store_row_bf16_x16<DT>(dkp, h, key < Sk, [&](int dt, int i) { return dk[dt][kt][i] * scale; });
      store_row_bf16_x16<DT>(dvp, h, key < Sk, [&](int dt, int i) { return dv[dt][kt][i]; });
    }
  } else {  // fp32 partials [hs][dK | dV][b][key][hk][D]
    const int64_t part = a.batch * a.seqlen_k * a.heads_kv * D;
    float* pk = dkv_part + (int64_t)(2 * hs) * part + ((int64_t)b * Sk * a.heads_kv + hk) * D;
    float* pv = pk + part;
#pragma unroll
    for (int kt = 0; kt < KH; ++kt) {
      const int key = kw + 32 * kt + r;
      if (key >= Sk) continue;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 wk, wv;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            wk[j] = dk[dt][kt][4 * g + j] * scale;
            wv[j] = dv[dt][kt][4 * g + j];
          }
          const int64_t o = (int64_t)key * a.heads_kv * D + 32 * dt + 8 * g + 4 * h;
          *reinterpret_cast<f32x4*>(pk + o) = wk;
          *reinterpret_cast<f32x4*>(pv + o) = wv;
        }
    }
  }
  }  // key blocks of the group
#if PICO_BWDKV_WGSTAMP
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  wgs[3] = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  if (wave == 0 && lane0 < 4 && blockIdx.x < 65536) stamp_out[blockIdx.x * 4 + lane0] = wgs[lane0 & 3];
#endif
}

}  // namespace

int attn_bwd_kv_launch(const pico_attn_args* a, const SplitPlan& p, hipStream_t s) {
  const auto kernel = a->head_dim == 128 ? (a->causal ? attn_bwd_kv_kernel<128, true, kv_minb(128, true)>
                                                      : attn_bwd_kv_kernel<128, false, kv_minb(128, false)>)
                                         : (a->causal ? attn_bwd_kv_kernel<64, true, kv_minb(64, true)>
                                                      : attn_bwd_kv_kernel<64, false, kv_minb(64, false)>);
  return pico_launch(PICO_K_ATTN_BWD_KV, "attn_bwd_kv", kernel, dim3((int)p.kv_grid), dim3(KNW * 64), 0, s, *a,
                     a->softmax_scale, a->softmax_scale * LOG2E, split_ws<float>(a, p.lse2_off),
                     split_ws<float>(a, p.delta_off), p.sq_pad, p.hsplit, split_ws<float>(a, p.part_off),
                     split_ws<unsigned long long>(a, p.stamp_off), p.grp);
}
