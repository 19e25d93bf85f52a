// FP8 (OCP e4m3) weight-only skinny linear for decode steps, and the row quantiser that makes its weights.
//
//   format       codes [N, K], one e4m3 byte each (finite codes only), and scale [N] fp32, one per output row: the
//                value of element (n, k) is scale[n] * e4m3(codes[n, k]). Per-row scales make stacking (q|k|v,
//                gate|up) a concatenation and leave a split-K partial without a scale.
//   quantiser    pico_quantize_rows_fp8: a wave per row of the bf16 matrix. Pass 1 takes the exact absmax (an integer
//                max over the magnitudes' bits); scale = absmax / 448 (correctly rounded division; a row of zeros:
//                1). Pass 2 re-reads the row (from L2), q = clamp(w / scale, -448, 448) (correctly rounded), and
//                v_cvt_pk_fp8_f32 rounds to nearest even; the clamp keeps the result out of the instruction's
//                overflow mode. Eight codes per lane and store.
//   stream       pico_decode_linear_fp8: y[M, N] = epilogue(scale[n] * (prologue(x)[M, K] . e4m3(codes)[N, K]^T)), 1
//                <= M <= 16. pico_decode_linear's workgroup (decode_linear.hip: 4 waves, 32 rows of W, the K slice's
//                steps dealt to the waves a trip at a time, accumulators added through LDS in wave order, K slices
//                across workgroups finished by a second launch in slice order) with another operand mapping:
//   W            lane l's 16-byte non-temporal load holds 16 consecutive codes of row n0 + (l & 15): columns k0 + 16 g
//                .. + 15, g = l >> 4. A wave's load covers 64 contiguous bytes of 16 rows, 64 columns: one K step.
//                Its low and high 8 bytes are the A operands of two v_mfma_f32_16x16x32_bf16: MFMA u of the pair
//                takes, from lane group g, columns k0 + 16 g + 8 u .. + 7, a permutation of the instruction's own K
//                order (8 g + j) that the B operand repeats. v_cvt_scalef32_pk_bf16_fp8 (scale 1.0) turns a dword's
//                half into two bf16, exactly: two per dword, eight per load. A trip is 4 loads per row block, 256
//                columns; two trips are in flight per wave, 64 KiB per workgroup. Every product bf16 x e4m3 is exact
//                in fp32, as bf16 x bf16 is.
//   x            staged in LDS as bf16, as in the bf16 kernel (row pitch k_slice + 8 elements: 16 bytes past a
//                multiple of 128, so the 16 rows of one lane group's ds_read_b128 fall on 16 different 16-byte bank
//                groups of the 256-byte bank row; lane group g reads 32 g + 16 u bytes into its row). MFMA u reads
//                x[m][k0 + 16 g + 8 u ..]. Padding columns take zeros from a register.
//   scale        one fp32 multiply scale[n] * acc by wave 0 after the wave reduction, or by the finishing launch
//                after the slice sum, before the epilogue's first rounding. Partials are written unscaled.
//   prologue, epilogue: pico_decode_linear's, rounding point for rounding point, on scale * acc.
#include "attn_common.h"
#include "common.h"
#include "decode_linear_fp8_plan.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

constexpr float E4M3_MAX = 448.f;

// ------------------------------------------------------------------------------------------------
// Row quantiser
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(const bf16_t* __restrict__ w, int64_t ldw,
                                                                uint8_t* __restrict__ codes, int64_t ldc,
                                                                float* __restrict__ scale, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const bf16_t* row = w + (int64_t)n * ldw;
  unsigned top = 0;  // the largest magnitude's bits: |a| <= |b| <=> bits(|a|) <= bits(|b|) for finite bf16
  for (int c = lane * 8; c < K; c += 512) {
    const u16x8 v = *reinterpret_cast<const u16x8*>(row + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) top = max(top, (unsigned)(v[j] & 0x7fffu));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) top = max(top, (unsigned)__shfl_xor((int)top, o));
  const float s = top ? __fdiv_rn(bf2f((unsigned short)top), E4M3_MAX) : 1.f;
  if (lane == 0) scale[n] = s;
  for (int c = lane * 8; c < K; c += 512) {
    const u16x8 v = *reinterpret_cast<const u16x8*>(row + c);
    float q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = fminf(fmaxf(__fdiv_rn(bf2f(v[j]), s), -E4M3_MAX), E4M3_MAX);
    u32x2 o;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      int pk = __builtin_amdgcn_cvt_pk_fp8_f32(q[4 * d], q[4 * d + 1], 0, false);
      pk = __builtin_amdgcn_cvt_pk_fp8_f32(q[4 * d + 2], q[4 * d + 3], pk, true);
      o[d] = (unsigned)pk;
    }
    *reinterpret_cast<u32x2*>(codes + (int64_t)n * ldc + c) = o;
  }
}

// ------------------------------------------------------------------------------------------------
// Stream kernel
// ------------------------------------------------------------------------------------------------
struct DL8Params {
  const bf16_t* x;
  const bf16_t* res;
  const bf16_t* nw;
  bf16_t* res_out;
  const uint8_t* w;
  const float* ws;
  void* y;
  float* part;
  int64_t ldx, ldr, ldro, ldw, ldy;
  int M, N, K, k_slice;
  float eps;
};

PICO_DEV void dl8_load8(const bf16_t* p, float* f) {
  const u16x8 v = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = bf2f(v[j]);
}

PICO_DEV u16x8 dl8_pack8(const float* f) {
  u16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = f2bf(f[j]);
  return v;
}

// xe = bf16(x + residual) (x itself without a residual), 8 elements of row m at column c
PICO_DEV void dl8_xe8(const DL8Params& p, int m, int c, float* v) {
  dl8_load8(p.x + (int64_t)m * p.ldx + c, v);
  if (p.res) {
    float r[8];
    dl8_load8(p.res + (int64_t)m * p.ldr + c, r);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf2f(f2bf(v[j] + r[j]));
  }
}

// 8 e4m3 codes (two dwords, ascending K) -> the bf16x8 MFMA operand, exactly
PICO_DEV bf16x8 dl8_operand(unsigned d0, unsigned d1) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, false);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, true);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, false);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, true);
  const bf16x4 lo = __builtin_shufflevector(a, b, 0, 1, 2, 3), hi = __builtin_shufflevector(c, d, 0, 1, 2, 3);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int EPI, bool NORM>
__global__ __launch_bounds__(DL_THREADS) void decode_linear_fp8_kernel(const DL8Params p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dl8_smem[];
  f32x4* red = reinterpret_cast<f32x4*>(dl8_smem);                  // [wave][row block][lane]
  bf16_t* xs = reinterpret_cast<bf16_t*>(dl8_smem + DL_RED_BYTES);  // [M][pitch]
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
        dl8_xe8(p, m, c, v);
        if (writer) *reinterpret_cast<u16x8*>(p.res_out + (int64_t)m * p.ldro + c) = dl8_pack8(v);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
      }
      rs = rsqrtf(wave_sum_dpp(ss) / (float)p.K + p.eps);
    }
    for (int c = lane * 8; c < klen; c += 512) {
      if constexpr (NORM) {
        float v[8], wf[8];
        dl8_xe8(p, m, kbeg + c, v);
        dl8_load8(p.nw + kbeg + c, wf);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] * rs * wf[j];
        *reinterpret_cast<u16x8*>(xs + m * pitch + c) = dl8_pack8(v);
      } else {
        *reinterpret_cast<u16x8*>(xs + m * pitch + c) =
            *reinterpret_cast<const u16x8*>(p.x + (int64_t)m * p.ldx + kbeg + c);
      }
    }
  }
  __syncthreads();

  // ---- the stream: lane l reads 16 codes of row (l & 15) of both row blocks at K offset 16 (l >> 4) of every step
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
  const uint8_t* wp[2] = {p.w + (int64_t)row[0] * p.ldw + kbeg + 16 * g, p.w + (int64_t)row[1] * p.ldw + kbeg + 16 * g};
  const bf16_t* xp = xs + li * pitch + 16 * g;
  const bool live = li < p.M;  // padding columns of B: zeros, nothing read
  const bf16x8 zero = {};
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  const int steps = klen / DL8_KSTEP, trips = steps / DL8_UNROLL;

  auto load_w = [&](int step, u32x4(&a)[2][DL8_UNROLL]) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int u = 0; u < DL8_UNROLL; ++u)
        a[b][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[b] + (step + u) * DL8_KSTEP));
  };
  // one K step: the load's two halves against x at k0 + 16 g + 8 u
  auto step_mfma = [&](int step, const u32x4& a0, const u32x4& a1) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bf16x8 b = live ? *reinterpret_cast<const bf16x8*>(xp + step * DL8_KSTEP + 8 * u) : zero;
      acc[0] = mfma16(dl8_operand(a0[2 * u], a0[2 * u + 1]), b, acc[0]);
      acc[1] = mfma16(dl8_operand(a1[2 * u], a1[2 * u + 1]), b, acc[1]);
    }
  };

  u32x4 a[2][DL8_UNROLL], nx[2][DL8_UNROLL];
  int t = wid;
  if (t < trips) load_w(t * DL8_UNROLL, a);
  for (; t < trips; t += DL_WAVES) {
    const bool more = t + DL_WAVES < trips;
    if (more) load_w((t + DL_WAVES) * DL8_UNROLL, nx);
#pragma unroll
    for (int u = 0; u < DL8_UNROLL; ++u) step_mfma(t * DL8_UNROLL + u, a[0][u], a[1][u]);
    if (more) {
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int u = 0; u < DL8_UNROLL; ++u) a[b][u] = nx[b][u];
    }
  }
  for (int s = trips * DL8_UNROLL + wid; s < steps; s += DL_WAVES)  // the slice's last steps, fewer than a trip
    step_mfma(s, *reinterpret_cast<const u32x4*>(wp[0] + s * DL8_KSTEP),
              *reinterpret_cast<const u32x4*>(wp[1] + s * DL8_KSTEP));

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
    const f32x4 sg = *reinterpret_cast<const f32x4*>(p.ws + j), su = *reinterpret_cast<const f32x4*>(p.ws + inter + j);
    u16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gf = bf2f(f2bf(sg[r] * sum[0][r])), uf = bf2f(f2bf(su[r] * sum[1][r]));
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
      const f32x4 sc = *reinterpret_cast<const f32x4*>(p.ws + n);
      if constexpr (EPI == DL_EPI_F32) {
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = bf2f(f2bf(sc[r] * sum[b][r]));
        *reinterpret_cast<f32x4*>((float*)p.y + (int64_t)m * p.ldy + n) = o;
      } else {
        u16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2bf(sc[r] * sum[b][r]);
        *reinterpret_cast<u16x4*>((bf16_t*)p.y + (int64_t)m * p.ldy + n) = o;
      }
    }
  }
}

// The finishing launch of a K split: one thread per output, the slices' partials added in slice order, the row's
// scale, then the epilogue. part is [nsplit][M][N] fp32.
template <int EPI>
__global__ __launch_bounds__(256) void decode_linear_fp8_finish_kernel(const float* __restrict__ part,
                                                                       const float* __restrict__ ws,
                                                                       void* __restrict__ y, int64_t ldy, int M, int N,
                                                                       int nsplit) {
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
  s0 *= ws[j];
  if constexpr (EPI == DL_EPI_SWIGLU) {
    s1 *= ws[outs + j];
    const float gf = bf2f(f2bf(s0)), uf = bf2f(f2bf(s1));
    ((bf16_t*)y)[(int64_t)m * ldy + j] = f2bf(gf * sigmoidf_(gf) * uf);
  } else if constexpr (EPI == DL_EPI_F32) {
    ((float*)y)[(int64_t)m * ldy + j] = bf2f(f2bf(s0));
  } else {
    ((bf16_t*)y)[(int64_t)m * ldy + j] = f2bf(s0);
  }
}

int dl8_check_shape(int64_t m, int64_t n, int64_t k, int epilogue, int64_t split_k) {
  PICO_REQUIRE(epilogue == DL_EPI_BF16 || epilogue == DL_EPI_F32 || epilogue == DL_EPI_SWIGLU,
               "pico_decode_linear_fp8: unknown epilogue %d", epilogue);
  PICO_REQUIRE(m >= 0 && m <= DL_MAX_M, "pico_decode_linear_fp8: m=%lld rows; 1..%d are supported", (long long)m,
               DL_MAX_M);
  PICO_REQUIRE(k > 0 && k % DL8_KSTEP == 0 && k <= (1 << 20),
               "pico_decode_linear_fp8: k=%lld must be a multiple of %d", (long long)k, DL8_KSTEP);
  PICO_REQUIRE(n > 0 && n % 8 == 0 && n <= (1 << 24), "pico_decode_linear_fp8: n=%lld must be a multiple of 8",
               (long long)n);
  PICO_REQUIRE(epilogue != DL_EPI_SWIGLU || n % 16 == 0,
               "pico_decode_linear_fp8: SWIGLU takes the stacked gate|up matrix, n=%lld must be a multiple of 16",
               (long long)n);
  PICO_REQUIRE(split_k <= (1 << 20), "pico_decode_linear_fp8: bad split_k %lld", (long long)split_k);
  return 0;
}

int dl8_check_plan(const DecodeLinearPlan& p) {
  PICO_REQUIRE(p.k_slice <= DL8_MAX_SLICE,
               "pico_decode_linear_fp8: split_k leaves slices of %lld columns; at most %d fit the workgroup's LDS",
               (long long)p.k_slice, DL8_MAX_SLICE);
  PICO_REQUIRE(p.blocks <= 0x7fffffff && p.split_k <= 65535, "pico_decode_linear_fp8: grid too large");
  return 0;
}

bool dl8_overlap(const void* a, int64_t a_elems, const void* b, int64_t b_elems) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + 2 * (uintptr_t)b_elems && b0 < a0 + 2 * (uintptr_t)a_elems;
}

template <int EPI>
int dl8_launch(const DecodeLinearPlan& pl, const DL8Params& p, bool norm, int64_t ldy, hipStream_t s) {
  const unsigned lds = (unsigned)decode_linear_lds_bytes(p.M, pl.k_slice);
  const dim3 grid((unsigned)pl.blocks, (unsigned)pl.split_k);
  auto k = norm ? decode_linear_fp8_kernel<EPI, true> : decode_linear_fp8_kernel<EPI, false>;
  if (lds > 64 * 1024) {  // once per kernel and device: the largest request any plan makes
    static bool raised[2][64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!raised[norm][dev]) {
      const int most = (int)decode_linear_lds_bytes(DL_MAX_M, DL8_MAX_SLICE);
      const hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, most);
      if (e != hipSuccess) return pico_set_error("pico_decode_linear_fp8: cannot set LDS size (%d)", (int)e);
      raised[norm][dev] = true;
    }
  }
  PICO_TRY(pico_launch(PICO_K_DECODE_LINEAR, "decode_linear_fp8", k, grid, dim3(DL_THREADS), lds, s, p));
  if (pl.split_k > 1) {
    const int64_t outs = EPI == DL_EPI_SWIGLU ? p.N / 2 : p.N;
    PICO_TRY(pico_launch(PICO_K_DECODE_LINEAR, "decode_linear_fp8_finish", decode_linear_fp8_finish_kernel<EPI>,
                         dim3((unsigned)pico_cdiv(p.M * outs, 256)), dim3(256), 0, s, p.part, p.ws, p.y, ldy, p.M, p.N,
                         (int)pl.split_k));
  }
  return 0;
}

}  // namespace

extern "C" int pico_quantize_rows_fp8(const void* w, int64_t ldw, void* codes, int64_t ldc, float* scale, int64_t n,
                                      int64_t k, void* stream) {
  PICO_REQUIRE(n >= 0 && n <= (1 << 24) && k > 0 && k % 8 == 0 && k <= (1 << 20),
               "pico_quantize_rows_fp8: n=%lld rows of k=%lld columns; k must be a multiple of 8", (long long)n,
               (long long)k);
  if (n == 0) return 0;
  PICO_REQUIRE(w && codes && scale, "pico_quantize_rows_fp8: null pointer");
  PICO_REQUIRE(ldw % 8 == 0 && ldw >= k && ldc % 8 == 0 && ldc >= k,
               "pico_quantize_rows_fp8: row strides must be multiples of 8 and cover a row");
  PICO_REQUIRE((uintptr_t)w % 16 == 0 && (uintptr_t)codes % 8 == 0 && (uintptr_t)scale % 4 == 0,
               "pico_quantize_rows_fp8: w must be 16-byte, codes 8-byte and scale 4-byte aligned");
  return pico_launch(PICO_K_CAST, "quantize_rows_fp8", quantize_rows_fp8_kernel, dim3((unsigned)pico_cdiv(n, 4)),
                     dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, ldw, (uint8_t*)codes, ldc, scale, (int)n,
                     (int)k);
}

extern "C" int64_t pico_decode_linear_fp8_args_size(void) { return (int64_t)sizeof(pico_decode_linear_fp8_args); }

extern "C" int pico_decode_linear_fp8_plan(int64_t m, int64_t n, int64_t k, int epilogue, int64_t split_k, int cus,
                                           int64_t* plan) {
  PICO_REQUIRE(plan, "pico_decode_linear_fp8_plan: null pointer");
  PICO_TRY(dl8_check_shape(m, n, k, epilogue, split_k));
  const DecodeLinearPlan p = decode_linear_fp8_plan(m, n, k, epilogue, split_k, cus > 0 ? cus : pico_num_cus());
  PICO_TRY(dl8_check_plan(p));
  plan[0] = p.blocks, plan[1] = p.split_k, plan[2] = p.k_slice, plan[3] = p.bytes;
  return 0;
}

extern "C" int pico_decode_linear_fp8(const pico_decode_linear_fp8_args* a, void* stream) {
  PICO_REQUIRE(a && a->x && a->weight && a->weight_scale && a->y, "pico_decode_linear_fp8: null pointer");
  PICO_TRY(dl8_check_shape(a->m, a->n, a->k, a->epilogue, a->split_k));
  const int64_t outs = a->epilogue == DL_EPI_SWIGLU ? a->n / 2 : a->n;
  PICO_REQUIRE(a->ldx % 8 == 0 && a->ldw % 16 == 0 && a->ldy % 8 == 0 && a->ldx >= a->k && a->ldw >= a->k &&
                   a->ldy >= outs,
               "pico_decode_linear_fp8: row strides must be multiples of 8 elements (weight: 16 bytes) and cover a row");
  PICO_REQUIRE(((uintptr_t)a->x | (uintptr_t)a->weight | (uintptr_t)a->weight_scale | (uintptr_t)a->y |
                (uintptr_t)a->norm_weight | (uintptr_t)a->residual | (uintptr_t)a->residual_out |
                (uintptr_t)a->workspace) % 16 == 0,
               "pico_decode_linear_fp8: pointers must be 16-byte aligned");
  const bool norm = a->norm_weight != nullptr;
  PICO_REQUIRE(norm || (!a->residual && !a->residual_out),
               "pico_decode_linear_fp8: residual / residual_out belong to the norm prologue (norm_weight is null)");
  if (a->residual)
    PICO_REQUIRE(a->ldr % 8 == 0 && a->ldr >= a->k, "pico_decode_linear_fp8: bad residual row stride %lld",
                 (long long)a->ldr);
  if (a->residual_out) {
    PICO_REQUIRE(a->ldro % 8 == 0 && a->ldro >= a->k, "pico_decode_linear_fp8: bad residual_out row stride %lld",
                 (long long)a->ldro);
    const int64_t rows = a->m > 0 ? a->m - 1 : 0;
    const int64_t ro = rows * a->ldro + a->k;
    PICO_REQUIRE(!dl8_overlap(a->residual_out, ro, a->x, rows * a->ldx + a->k) &&
                     !(a->residual && dl8_overlap(a->residual_out, ro, a->residual, rows * a->ldr + a->k)),
                 "pico_decode_linear_fp8: residual_out must not alias x or residual (other workgroups still read "
                 "them)");
  }
  const DecodeLinearPlan pl = decode_linear_fp8_plan(a->m, a->n, a->k, a->epilogue, a->split_k, pico_num_cus());
  PICO_TRY(dl8_check_plan(pl));
  PICO_REQUIRE(pl.split_k == 1 || a->workspace, "pico_decode_linear_fp8: a K split needs the workspace");
  if (a->m == 0) return 0;
  DL8Params p{};
  p.x = (const bf16_t*)a->x;
  p.res = (const bf16_t*)a->residual;
  p.nw = (const bf16_t*)a->norm_weight;
  p.res_out = (bf16_t*)a->residual_out;
  p.w = (const uint8_t*)a->weight;
  p.ws = a->weight_scale;
  p.y = a->y;
  p.part = (float*)a->workspace;
  p.ldx = a->ldx, p.ldr = a->ldr, p.ldro = a->ldro, p.ldw = a->ldw, p.ldy = a->ldy;
  p.M = (int)a->m, p.N = (int)a->n, p.K = (int)a->k, p.k_slice = (int)pl.k_slice;
  p.eps = a->eps;
  hipStream_t s = (hipStream_t)stream;
  switch (a->epilogue) {
    case DL_EPI_BF16: return dl8_launch<DL_EPI_BF16>(pl, p, norm, a->ldy, s);
    case DL_EPI_F32: return dl8_launch<DL_EPI_F32>(pl, p, norm, a->ldy, s);
    default: return dl8_launch<DL_EPI_SWIGLU>(pl, p, norm, a->ldy, s);
  }
}
