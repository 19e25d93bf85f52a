// MXFP4 (OCP e2m1 codes, one E8M0 scale per 32 elements) weight-only skinny linear for decode steps, and the block
// quantiser that makes its weights.
//
//   format       codes [N, K/2], two e2m1 codes per byte (element 2j the low nibble, 2j + 1 the high one), and scales
//                [N, K/32], one E8M0 byte per block of 32 columns: element (n, k) has the value 2^(scales[n, k/32] -
//                127) * e2m1(code), e2m1 in +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}. The scale runs along K inside a row, so
//                stacking (q|k|v, gate|up) is a concatenation and a split-K partial carries no scale.
//   quantiser    pico_quantize_rows_mxfp4: a lane per 8 elements, 4 lanes per block. The block's largest magnitude
//                is an integer max over the bf16 magnitude bits; its exponent field E gives the shared exponent e =
//                clamp(E - 127 - 2, -120, 125) (a block of zeros: e = 0), byte e + 127. A code is the round-to-nearest-
//                even of |w| 2^-e on the e2m1 grid, saturated at 6, with w's sign bit: integer arithmetic on the bf16
//                bits (mx4_code below), which plain torch reproduces bit for bit. v_cvt_scalef32_pk_fp4_f32 is not
//                used: what it returns for a negative value that rounds to zero and for a denormal input is not
//                something the builtin's documentation fixes, and the integer form is checked against the torch
//                restatement without a device.
//   stream       pico_decode_linear_mxfp4: y[M, N] = epilogue(prologue(x)[M, K] . dequant(W)[N, K]^T), 1 <= M <= 16.
//                pico_decode_linear_fp8's workgroup (4 waves, 32 rows of W, x staged in LDS as bf16, the waves'
//                accumulators added through LDS in wave order, K slices across workgroups finished by a second
//                launch in slice order) with another operand path:
//   W            lane l = (c = l & 15, g = l >> 4): its 16-byte non-temporal load holds the 32 codes of one MX block
//                of row n0 + c, columns k0 + 32 g .. + 31. A wave's load covers 64 contiguous bytes of 16 rows: 128
//                columns, one K step, the load pattern of the FP8 kernel. Dword u of the load (codes 8 u .. 8 u + 7)
//                is the A operand of MFMA u of four v_mfma_f32_16x16x32_bf16: from lane group g it takes columns k0 +
//                32 g + 8 u .. + 7, a permutation of the instruction's own K order that the B operand repeats.
//   scale        the load's one E8M0 byte, shifted into an fp32 exponent (byte << 23), is the scale operand of the
//                load's sixteen v_cvt_scalef32_pk_bf16_fp4: the conversion dequantises, exactly (a 2-bit significand
//                times a power of two; the quantiser's clamp keeps every value a normal bf16). No scale reaches the
//                accumulator, the partials or the epilogue.
//   scale bytes  a trip is 4 loads per row block, 512 columns, 16 scale bytes of a row. Lane (c, g) loads dword g of
//                them, once: the four lane groups read the row's 16 bytes contiguously and no byte twice. Load u
//                needs byte 4 u + g: byte g of lane (c, u)'s dword, fetched by one ds_bpermute_b32 per load (the LDS
//                crossbar; no LDS memory). The alternative, four consecutive blocks per lane so that its own dword
//                serves the trip, makes every 16-byte load instruction touch four 16-byte pieces 64 bytes apart in
//                each row (64 quarter-used 64-byte segments per instruction where this one reads 16 whole ones), on
//                the one path whose rate the kernel lives on; four bpermutes beside sixteen ds_read_b128 cost less
//                than that risk. A slice's last steps (fewer than a trip) take a byte load each.
//   trips        a slice holds at most 2048 columns = 4 trips, one per wave: a wave issues all its loads (8 x 16 bytes
//                and 2 dwords per lane, plus one lone step's) before its first conversion; there is no second trip to
//                prefetch. Lone steps go to the waves after the last trip's.
//   x            staged in LDS as bf16 as in the FP8 kernel (row pitch k_slice + 8 elements: 16 bytes past a multiple
//                of 256). MFMA u of lane (c, g) reads x[c][k0 + 32 g + 8 u ..]: 64 g + 16 u bytes into its row, so
//                the 16 rows of a lane group's ds_read_b128 fall on the 16 different 16-byte bank groups (c + 4 g +
//                u) mod 16 of the 256-byte bank row, as in the FP8 kernel (there 2 g + u). Padding columns take
//                zeros from a register.
//   prologue, epilogue: pico_decode_linear's, rounding point for rounding point, on acc.
#include "attn_common.h"
#include "common.h"
#include "decode_linear_mxfp4_plan.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// ------------------------------------------------------------------------------------------------
// Block quantiser
// ------------------------------------------------------------------------------------------------
// The e2m1 code of the bf16 value `bits` under the shared exponent e: RNE of |w| 2^-e in units of the code (codes
// are monotonic in the magnitude: exponent field code >> 1, significand bit code & 1), saturated at 7 (= 6.0).
PICO_DEV unsigned mx4_code(unsigned bits, int e) {
  const unsigned sign = (bits >> 12) & 8u, E = (bits >> 7) & 0xffu, man = bits & 0x7fu;
  if (E == 0) return sign;                  // zero or a bf16 denormal: below a quarter of the grid's first step
  const int ex = (int)E - 127 - e;          // |w| 2^-e = 2^ex (1 + man / 128), ex <= 2
  unsigned n, shift;
  if (ex >= 0) {
    n = ((unsigned)(ex + 1) << 7) | man, shift = 6;  // code = 2 (ex + 1) + man / 64
  } else {
    n = 128u | man, shift = (unsigned)min(6 - ex, 16);  // the subnormal step 0.5: code = (128 + man) 2^(ex - 6)
  }
  unsigned r = n >> shift;
  const unsigned rem = n & ((1u << shift) - 1u), half = 1u << (shift - 1);
  r += (rem > half || (rem == half && (r & 1u))) ? 1u : 0u;
  return sign | min(r, 7u);
}

__global__ __launch_bounds__(256) void quantize_rows_mxfp4_kernel(const bf16_t* __restrict__ w, int64_t ldw,
                                                                  uint8_t* __restrict__ codes, int64_t ldc,
                                                                  uint8_t* __restrict__ scales, int64_t lds, int N,
                                                                  int K) {
  const int per_row = K / 8;  // a multiple of 4: the 4 lanes of a block share a row and are live together
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)N * per_row) return;
  const int n = (int)(idx / per_row), j = (int)(idx - (int64_t)n * per_row);
  const u16x8 v = *reinterpret_cast<const u16x8*>(w + (int64_t)n * ldw + 8 * j);
  unsigned top = 0;  // the largest magnitude's bits: |a| <= |b| <=> bits(|a|) <= bits(|b|) for finite bf16
#pragma unroll
  for (int i = 0; i < 8; ++i) top = max(top, (unsigned)(v[i] & 0x7fffu));
  top = max(top, (unsigned)__shfl_xor((int)top, 1));
  top = max(top, (unsigned)__shfl_xor((int)top, 2));
  const int e = top ? min(max((int)(top >> 7) - 129, -120), 125) : 0;
  unsigned o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= mx4_code(v[i], e) << (4 * i);
  *reinterpret_cast<unsigned*>(codes + (int64_t)n * ldc + 4 * j) = o;
  if ((j & 3) == 0) scales[(int64_t)n * lds + (j >> 2)] = (uint8_t)(e + 127);
}

// ------------------------------------------------------------------------------------------------
// Stream kernel
// ------------------------------------------------------------------------------------------------
struct DL4Params {
  const bf16_t* x;
  const bf16_t* res;
  const bf16_t* nw;
  bf16_t* res_out;
  const uint8_t* w;
  const uint8_t* sc;
  void* y;
  float* part;
  int64_t ldx, ldr, ldro, ldw, lds, ldy;
  int M, N, K, k_slice;
  float eps;
};

PICO_DEV void dl4_load8(const bf16_t* p, float* f) {
  const u16x8 v = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = bf2f(v[j]);
}

PICO_DEV u16x8 dl4_pack8(const float* f) {
  u16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = f2bf(f[j]);
  return v;
}

// xe = bf16(x + residual) (x itself without a residual), 8 elements of row m at column c
PICO_DEV void dl4_xe8(const DL4Params& p, int m, int c, float* v) {
  dl4_load8(p.x + (int64_t)m * p.ldx + c, v);
  if (p.res) {
    float r[8];
    dl4_load8(p.res + (int64_t)m * p.ldr + c, r);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf2f(f2bf(v[j] + r[j]));
  }
}

// an E8M0 byte as the conversions' scale operand: 2^(byte - 127) in fp32 (bytes 1 .. 254)
PICO_DEV float dl4_scale(unsigned byte) { return __uint_as_float((byte & 0xffu) << 23); }

// 8 e2m1 codes (one dword, ascending K from the low nibble) times the block's scale -> the bf16x8 MFMA operand
PICO_DEV bf16x8 dl4_operand(unsigned d, float scale) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2);
  const bf16x2 e = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3);
  const bf16x4 lo = __builtin_shufflevector(a, b, 0, 1, 2, 3), hi = __builtin_shufflevector(c, e, 0, 1, 2, 3);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int EPI, bool NORM>
__global__ __launch_bounds__(DL_THREADS) void decode_linear_mxfp4_kernel(const DL4Params p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dl4_smem[];
  f32x4* red = reinterpret_cast<f32x4*>(dl4_smem);                  // [wave][row block][lane]
  bf16_t* xs = reinterpret_cast<bf16_t*>(dl4_smem + DL_RED_BYTES);  // [M][pitch]
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int kbeg = blockIdx.y * p.k_slice;
  const int klen = min(p.k_slice, p.K - kbeg);
  const int pitch = p.k_slice + DL_X_PAD;
  const bool split = gridDim.y > 1;

  // ---- stage the B operand: rows wid, wid + 4, ... of x (or of h), this workgroup's K slice
  for (int m = wid; m < p.M; m += DL_WAVES) {
    float rs = 1.f;
    if constexpr (NORM) {
      const bool writer = p.res_out && blockIdx.x == 0 && blockIdx.y == 0;
      float ss = 0.f;
      for (int c = lane * 8; c < p.K; c += 512) {
        float v[8];
        dl4_xe8(p, m, c, v);
        if (writer) *reinterpret_cast<u16x8*>(p.res_out + (int64_t)m * p.ldro + c) = dl4_pack8(v);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
      }
      rs = rsqrtf(wave_sum_dpp(ss) / (float)p.K + p.eps);
    }
    for (int c = lane * 8; c < klen; c += 512) {
      if constexpr (NORM) {
        float v[8], wf[8];
        dl4_xe8(p, m, kbeg + c, v);
        dl4_load8(p.nw + kbeg + c, wf);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] * rs * wf[j];
        *reinterpret_cast<u16x8*>(xs + m * pitch + c) = dl4_pack8(v);
      } else {
        *reinterpret_cast<u16x8*>(xs + m * pitch + c) =
            *reinterpret_cast<const u16x8*>(p.x + (int64_t)m * p.ldx + kbeg + c);
      }
    }
  }
  __syncthreads();

  // ---- the stream: lane l reads the MX block (l >> 4) of row (l & 15) of both row blocks in every step
  const int li = lane & 15, g = lane >> 4;
  int row[2], out0;  // out0: the first of the 16 (SWIGLU) or 32 outputs this workgroup owns
  if constexpr (EPI == DL_EPI_SWIGLU) {
    const int inter = p.N / 2;
    out0 = blockIdx.x * 16;
    row[0] = min(out0 + li, inter - 1);  // a row past the end re-reads the last one; its result is not stored
    row[1] = inter + row[0];
  } else {
    out0 = blockIdx.x * DL_BLOCK_ROWS;
    row[0] = min(out0 + li, p.N - 1);
    row[1] = min(out0 + 16 + li, p.N - 1);
  }
  const uint8_t* wp[2] = {p.w + (int64_t)row[0] * p.ldw + kbeg / 2 + 16 * g,
                          p.w + (int64_t)row[1] * p.ldw + kbeg / 2 + 16 * g};
  const uint8_t* sp[2] = {p.sc + (int64_t)row[0] * p.lds + kbeg / MX4_BLOCK,
                          p.sc + (int64_t)row[1] * p.lds + kbeg / MX4_BLOCK};
  const bf16_t* xp = xs + li * pitch + MX4_BLOCK * g;
  const bool live = li < p.M;  // padding columns of B: zeros, nothing read
  const bf16x8 zero = {};
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  const int steps = klen / DL4_KSTEP, trips = steps / DL4_UNROLL;  // trips <= 4: wave wid takes trip wid
  const bool trip = wid < trips;
  // the slice's last steps, fewer than a trip: one each to the waves after the last trip's
  const int ls = trips * DL4_UNROLL + ((wid - trips) & (DL_WAVES - 1));
  const bool lone = ls < steps;
  constexpr int STEP_BYTES = DL4_KSTEP / 2, STEP_BLOCKS = DL4_KSTEP / MX4_BLOCK;

  // one K step: the load's four dwords against x at k0 + 32 g + 8 u, the block's scale in the conversion
  auto step_mfma = [&](int step, const u32x4& a0, const u32x4& a1, float s0, float s1) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bf16x8 b = live ? *reinterpret_cast<const bf16x8*>(xp + step * DL4_KSTEP + 8 * u) : zero;
      acc[0] = mfma16(dl4_operand(a0[u], s0), b, acc[0]);
      acc[1] = mfma16(dl4_operand(a1[u], s1), b, acc[1]);
    }
  };

  u32x4 a[2][DL4_UNROLL], la[2];
  unsigned sd[2] = {0u, 0u}, lb[2] = {0u, 0u};
  if (trip) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int u = 0; u < DL4_UNROLL; ++u)
        a[b][u] = __builtin_nontemporal_load(
            reinterpret_cast<const u32x4*>(wp[b] + (wid * DL4_UNROLL + u) * STEP_BYTES));
      sd[b] = *reinterpret_cast<const unsigned*>(sp[b] + wid * DL4_UNROLL * STEP_BLOCKS + 4 * g);
    }
  }
  if (lone) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      la[b] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[b] + ls * STEP_BYTES));
      lb[b] = sp[b][ls * STEP_BLOCKS + g];
    }
  }
  if (trip) {
#pragma unroll
    for (int u = 0; u < DL4_UNROLL; ++u) {  // load u holds block 4 u + g: byte g of lane (li, u)'s dword
      const unsigned d0 = (unsigned)__builtin_amdgcn_ds_bpermute(4 * (li + 16 * u), (int)sd[0]);
      const unsigned d1 = (unsigned)__builtin_amdgcn_ds_bpermute(4 * (li + 16 * u), (int)sd[1]);
      step_mfma(wid * DL4_UNROLL + u, a[0][u], a[1][u], dl4_scale(d0 >> (8 * g)), dl4_scale(d1 >> (8 * g)));
    }
  }
  if (lone) step_mfma(ls, la[0], la[1], dl4_scale(lb[0]), dl4_scale(lb[1]));

  // ---- the waves' accumulators, added in wave order
  red[(wid * 2 + 0) * 64 + lane] = acc[0];
  red[(wid * 2 + 1) * 64 + lane] = acc[1];
  __syncthreads();
  if (wid != 0 || !live) return;
  f32x4 sum[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    sum[b] = red[b * 64 + lane];
#pragma unroll
    for (int w = 1; w < DL_WAVES; ++w) {
      const f32x4 v = red[(w * 2 + b) * 64 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[b][r] += v[r];
    }
  }

  // ---- lane l holds outputs (row li of y, 4 consecutive columns 4 g .. 4 g + 3 of each row block)
  const int m = li;
  if constexpr (EPI == DL_EPI_SWIGLU) {
    const int inter = p.N / 2, j = out0 + 4 * g;
    if (j >= inter) return;
    if (split) {
      float* pr = p.part + ((int64_t)blockIdx.y * p.M + m) * p.N;
      *reinterpret_cast<f32x4*>(pr + j) = sum[0];
      *reinterpret_cast<f32x4*>(pr + inter + j) = sum[1];
      return;
    }
    u16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gf = bf2f(f2bf(sum[0][r])), uf = bf2f(f2bf(sum[1][r]));
      o[r] = f2bf(gf * sigmoidf_(gf) * uf);
    }
    *reinterpret_cast<u16x4*>((bf16_t*)p.y + (int64_t)m * p.ldy + j) = o;
  } else {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int n = out0 + 16 * b + 4 * g;
      if (n >= p.N) continue;
      if (split) {
        *reinterpret_cast<f32x4*>(p.part + ((int64_t)blockIdx.y * p.M + m) * p.N + n) = sum[b];
        continue;
      }
      if constexpr (EPI == DL_EPI_F32) {
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = bf2f(f2bf(sum[b][r]));
        *reinterpret_cast<f32x4*>((float*)p.y + (int64_t)m * p.ldy + n) = o;
      } else {
        u16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2bf(sum[b][r]);
        *reinterpret_cast<u16x4*>((bf16_t*)p.y + (int64_t)m * p.ldy + n) = o;
      }
    }
  }
}

// The finishing launch of a K split: one thread per output, the slices' partials added in slice order, then the
// epilogue. part is [nsplit][M][N] fp32.
template <int EPI>
__global__ __launch_bounds__(256) void decode_linear_mxfp4_finish_kernel(const float* __restrict__ part,
                                                                         void* __restrict__ y, int64_t ldy, int M,
                                                                         int N, int nsplit) {
  const int outs = EPI == DL_EPI_SWIGLU ? N / 2 : N;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * outs) return;
  const int m = idx / outs, j = idx - m * outs;
  const int64_t plane = (int64_t)M * N;
  const float* p0 = part + (int64_t)m * N + j;
  float s0 = 0.f, s1 = 0.f;
#pragma unroll 4
  for (int s = 0; s < nsplit; ++s) {
    s0 += p0[s * plane];
    if constexpr (EPI == DL_EPI_SWIGLU) s1 += p0[s * plane + outs];
  }
  if constexpr (EPI == DL_EPI_SWIGLU) {
    const float gf = bf2f(f2bf(s0)), uf = bf2f(f2bf(s1));
    ((bf16_t*)y)[(int64_t)m * ldy + j] = f2bf(gf * sigmoidf_(gf) * uf);
  } else if constexpr (EPI == DL_EPI_F32) {
    ((float*)y)[(int64_t)m * ldy + j] = bf2f(f2bf(s0));
  } else {
    ((bf16_t*)y)[(int64_t)m * ldy + j] = f2bf(s0);
  }
}

int dl4_check_shape(int64_t m, int64_t n, int64_t k, int epilogue, int64_t split_k) {
  PICO_REQUIRE(epilogue == DL_EPI_BF16 || epilogue == DL_EPI_F32 || epilogue == DL_EPI_SWIGLU,
               "pico_decode_linear_mxfp4: unknown epilogue %d", epilogue);
  PICO_REQUIRE(m >= 0 && m <= DL_MAX_M, "pico_decode_linear_mxfp4: m=%lld rows; 1..%d are supported", (long long)m,
               DL_MAX_M);
  PICO_REQUIRE(k > 0 && k % DL4_KSTEP == 0 && k <= (1 << 20),
               "pico_decode_linear_mxfp4: k=%lld must be a multiple of %d", (long long)k, DL4_KSTEP);
  PICO_REQUIRE(n > 0 && n % 8 == 0 && n <= (1 << 24), "pico_decode_linear_mxfp4: n=%lld must be a multiple of 8",
               (long long)n);
  PICO_REQUIRE(epilogue != DL_EPI_SWIGLU || n % 16 == 0,
               "pico_decode_linear_mxfp4: SWIGLU takes the stacked gate|up matrix, n=%lld must be a multiple of 16",
               (long long)n);
  PICO_REQUIRE(split_k <= (1 << 20), "pico_decode_linear_mxfp4: bad split_k %lld", (long long)split_k);
  return 0;
}

int dl4_check_plan(const DecodeLinearPlan& p) {
  PICO_REQUIRE(p.k_slice <= DL4_MAX_SLICE,
               "pico_decode_linear_mxfp4: split_k leaves slices of %lld columns; at most %d fit the workgroup's LDS",
               (long long)p.k_slice, DL4_MAX_SLICE);
  PICO_REQUIRE(p.blocks <= 0x7fffffff && p.split_k <= 65535, "pico_decode_linear_mxfp4: grid too large");
  return 0;
}

bool dl4_overlap(const void* a, int64_t a_elems, const void* b, int64_t b_elems) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + 2 * (uintptr_t)b_elems && b0 < a0 + 2 * (uintptr_t)a_elems;
}

template <int EPI>
int dl4_launch(const DecodeLinearPlan& pl, const DL4Params& p, bool norm, int64_t ldy, hipStream_t s) {
  const unsigned lds = (unsigned)decode_linear_lds_bytes(p.M, pl.k_slice);
  const dim3 grid((unsigned)pl.blocks, (unsigned)pl.split_k);
  auto k = norm ? decode_linear_mxfp4_kernel<EPI, true> : decode_linear_mxfp4_kernel<EPI, false>;
  if (lds > 64 * 1024) {  // once per kernel and device: the largest request any plan makes
    static bool raised[2][64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!raised[norm][dev]) {
      const int most = (int)decode_linear_lds_bytes(DL_MAX_M, DL4_MAX_SLICE);
      const hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, most);
      if (e != hipSuccess) return pico_set_error("pico_decode_linear_mxfp4: cannot set LDS size (%d)", (int)e);
      raised[norm][dev] = true;
    }
  }
  PICO_TRY(pico_launch(PICO_K_DECODE_LINEAR, "decode_linear_mxfp4", k, grid, dim3(DL_THREADS), lds, s, p));
  if (pl.split_k > 1) {
    const int64_t outs = EPI == DL_EPI_SWIGLU ? p.N / 2 : p.N;
    PICO_TRY(pico_launch(PICO_K_DECODE_LINEAR, "decode_linear_mxfp4_finish", decode_linear_mxfp4_finish_kernel<EPI>,
                         dim3((unsigned)pico_cdiv(p.M * outs, 256)), dim3(256), 0, s, p.part, p.y, ldy, p.M, p.N,
                         (int)pl.split_k));
  }
  return 0;
}

}  // namespace

extern "C" int pico_quantize_rows_mxfp4(const void* w, int64_t ldw, void* codes, int64_t ldc, void* scales,
                                        int64_t lds, int64_t n, int64_t k, void* stream) {
  PICO_REQUIRE(n >= 0 && n <= (1 << 24) && k > 0 && k % MX4_BLOCK == 0 && k <= (1 << 20),
               "pico_quantize_rows_mxfp4: n=%lld rows of k=%lld columns; k must be a multiple of %d", (long long)n,
               (long long)k, MX4_BLOCK);
  if (n == 0) return 0;
  PICO_REQUIRE(w && codes && scales, "pico_quantize_rows_mxfp4: null pointer");
  PICO_REQUIRE(ldw % 8 == 0 && ldw >= k && ldc % 4 == 0 && ldc >= k / 2 && lds >= k / MX4_BLOCK,
               "pico_quantize_rows_mxfp4: row strides must cover a row (w: a multiple of 8 elements, codes: of 4 "
               "bytes)");
  PICO_REQUIRE((uintptr_t)w % 16 == 0 && (uintptr_t)codes % 4 == 0,
               "pico_quantize_rows_mxfp4: w must be 16-byte and codes 4-byte aligned");
  return pico_launch(PICO_K_CAST, "quantize_rows_mxfp4", quantize_rows_mxfp4_kernel,
                     dim3((unsigned)pico_cdiv(n * (k / 8), 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)w, ldw, (uint8_t*)codes, ldc, (uint8_t*)scales, lds, (int)n, (int)k);
}

extern "C" int64_t pico_decode_linear_mxfp4_args_size(void) {
  return (int64_t)sizeof(pico_decode_linear_mxfp4_args);
}

extern "C" int pico_decode_linear_mxfp4_plan(int64_t m, int64_t n, int64_t k, int epilogue, int64_t split_k, int cus,
                                             int64_t* plan) {
  PICO_REQUIRE(plan, "pico_decode_linear_mxfp4_plan: null pointer");
  PICO_TRY(dl4_check_shape(m, n, k, epilogue, split_k));
  const DecodeLinearPlan p = decode_linear_mxfp4_plan(m, n, k, epilogue, split_k, cus > 0 ? cus : pico_num_cus());
  PICO_TRY(dl4_check_plan(p));
  plan[0] = p.blocks, plan[1] = p.split_k, plan[2] = p.k_slice, plan[3] = p.bytes;
  return 0;
}

extern "C" int pico_decode_linear_mxfp4(const pico_decode_linear_mxfp4_args* a, void* stream) {
  PICO_REQUIRE(a && a->x && a->weight && a->weight_scale && a->y, "pico_decode_linear_mxfp4: null pointer");
  PICO_TRY(dl4_check_shape(a->m, a->n, a->k, a->epilogue, a->split_k));
  const int64_t outs = a->epilogue == DL_EPI_SWIGLU ? a->n / 2 : a->n;
  PICO_REQUIRE(a->ldx % 8 == 0 && a->ldw % 16 == 0 && a->lds % 4 == 0 && a->ldy % 8 == 0 && a->ldx >= a->k &&
                   a->ldw >= a->k / 2 && a->lds >= a->k / MX4_BLOCK && a->ldy >= outs,
               "pico_decode_linear_mxfp4: row strides must be multiples of 8 elements (codes: 16 bytes, scales: 4 "
               "bytes) and cover a row");
  PICO_REQUIRE(((uintptr_t)a->x | (uintptr_t)a->weight | (uintptr_t)a->y | (uintptr_t)a->norm_weight |
                (uintptr_t)a->residual | (uintptr_t)a->residual_out | (uintptr_t)a->workspace) % 16 == 0 &&
                   (uintptr_t)a->weight_scale % 4 == 0,
               "pico_decode_linear_mxfp4: pointers must be 16-byte aligned (weight_scale: 4-byte)");
  const bool norm = a->norm_weight != nullptr;
  PICO_REQUIRE(norm || (!a->residual && !a->residual_out),
               "pico_decode_linear_mxfp4: residual / residual_out belong to the norm prologue (norm_weight is null)");
  if (a->residual)
    PICO_REQUIRE(a->ldr % 8 == 0 && a->ldr >= a->k, "pico_decode_linear_mxfp4: bad residual row stride %lld",
                 (long long)a->ldr);
  if (a->residual_out) {
    PICO_REQUIRE(a->ldro % 8 == 0 && a->ldro >= a->k, "pico_decode_linear_mxfp4: bad residual_out row stride %lld",
                 (long long)a->ldro);
    const int64_t rows = a->m > 0 ? a->m - 1 : 0;
    const int64_t ro = rows * a->ldro + a->k;
    PICO_REQUIRE(!dl4_overlap(a->residual_out, ro, a->x, rows * a->ldx + a->k) &&
                     !(a->residual && dl4_overlap(a->residual_out, ro, a->residual, rows * a->ldr + a->k)),
                 "pico_decode_linear_mxfp4: residual_out must not alias x or residual (other workgroups still read "
                 "them)");
  }
  const DecodeLinearPlan pl = decode_linear_mxfp4_plan(a->m, a->n, a->k, a->epilogue, a->split_k, pico_num_cus());
  PICO_TRY(dl4_check_plan(pl));
  PICO_REQUIRE(pl.split_k == 1 || a->workspace, "pico_decode_linear_mxfp4: a K split needs the workspace");
  if (a->m == 0) return 0;
  DL4Params p{};
  p.x = (const bf16_t*)a->x;
  p.res = (const bf16_t*)a->residual;
  p.nw = (const bf16_t*)a->norm_weight;
  p.res_out = (bf16_t*)a->residual_out;
  p.w = (const uint8_t*)a->weight;
  p.sc = (const uint8_t*)a->weight_scale;
  p.y = a->y;
  p.part = (float*)a->workspace;
  p.ldx = a->ldx, p.ldr = a->ldr, p.ldro = a->ldro, p.ldw = a->ldw, p.lds = a->lds, p.ldy = a->ldy;
  p.M = (int)a->m, p.N = (int)a->n, p.K = (int)a->k, p.k_slice = (int)pl.k_slice;
  p.eps = a->eps;
  hipStream_t s = (hipStream_t)stream;
  switch (a->epilogue) {
    case DL_EPI_BF16: return dl4_launch<DL_EPI_BF16>(pl, p, norm, a->ldy, s);
    case DL_EPI_F32: return dl4_launch<DL_EPI_F32>(pl, p, norm, a->ldy, s);
    default: return dl4_launch<DL_EPI_SWIGLU>(pl, p, norm, a->ldy, s);
  }
}
