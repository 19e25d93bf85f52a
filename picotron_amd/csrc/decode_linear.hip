// Skinny weight-streaming linear for decode steps: y[M, N] = epilogue(prologue(x)[M, K] . W[N, K]^T), 1 <= M <= 16.
//
// At M <= 16 a projection is one pass over W; everything else is small. The layout follows from that:
//
//   work split   A workgroup (4 waves) owns 32 rows of W (SWIGLU: 16 gate rows and the 16 up rows of the same
//                columns) over one K slice (decode_linear_plan.h). Its waves take the slice's K steps in turn, four
//                steps per trip, and add their accumulators through LDS in wave order. Where the column blocks
//                alone leave CUs idle the plan cuts K into slices across workgroups: each writes an fp32 partial
//                [M, N] to the workspace and a finishing launch adds the slices in slice order and applies the
//                epilogue. No atomics, no workgroup waits for another: the same shape and split give the same bits.
//   W            v_mfma_f32_16x16x32_bf16 with W as the A operand: lane l's 16-byte load of W[n0 + (l & 15)][k0 +
//                8 (l >> 4) ..] is the operand as it stands (no unpack, no shuffle); a wave's load covers 64
//                contiguous bytes of 16 rows and its next three the rest of the rows' 256 bytes. Two trips are in
//                flight per wave (the next trip's 8 loads are issued before the current trip's MFMAs): 64 KiB per
//                workgroup. Each element of W is read once.
//   x            The B operand: x^T padded to 16 columns. The workgroup stages its K slice of the M real rows in
//                LDS once (row pitch k_slice + 8: the 16 rows of a ds_read_b128 fall on different banks); lanes of
//                the padding columns take zeros from a register and read nothing. Column m of the result depends
//                on column m of B alone: a row's bits do not depend on the other rows, nor on M.
//   prologue     NORM: every workgroup recomputes rstd of every row over the whole K (a wave per row, x from L2)
//                and stages h = bf16(xe rstd w) for its slice, xe = bf16(x + residual): pico_rmsnorm_fwd's
//                arithmetic and rounding points. Workgroup (0, 0) alone writes residual_out.
//   epilogue     wave 0, after the reduction: BF16 y = bf16(acc); F32 y = float(bf16(acc)); SWIGLU act =
//                bf16(silu(g) u) on g = bf16(acc_g), u = bf16(acc_u) (pico_swiglu_fwd's arithmetic).
#include "attn_common.h"
#include "common.h"
#include "decode_linear_plan.h"

namespace {

struct DLParams {
  const bf16_t* x;
  const bf16_t* res;
  const bf16_t* nw;
  bf16_t* res_out;
  const bf16_t* w;
  void* y;
  float* part;
  int64_t ldx, ldr, ldro, ldw, ldy;
  int M, N, K, k_slice;
  float eps;
};

PICO_DEV void dl_load8(const bf16_t* p, float* f) {
  const u16x8 v = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = bf2f(v[j]);
}

PICO_DEV u16x8 dl_pack8(const float* f) {
  u16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = f2bf(f[j]);
  return v;
}

// xe = bf16(x + residual) (x itself without a residual), 8 elements of row m at column c
PICO_DEV void dl_xe8(const DLParams& p, int m, int c, float* v) {
  dl_load8(p.x + (int64_t)m * p.ldx + c, v);
  if (p.res) {
    float r[8];
    dl_load8(p.res + (int64_t)m * p.ldr + c, r);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf2f(f2bf(v[j] + r[j]));
  }
}

template <int EPI, bool NORM>
__global__ __launch_bounds__(DL_THREADS) void decode_linear_kernel(const DLParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dl_smem[];
  f32x4* red = reinterpret_cast<f32x4*>(dl_smem);                  // [wave][row block][lane]
  bf16_t* xs = reinterpret_cast<bf16_t*>(dl_smem + DL_RED_BYTES);  // [M][pitch]
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
        dl_xe8(p, m, c, v);
        if (writer) *reinterpret_cast<u16x8*>(p.res_out + (int64_t)m * p.ldro + c) = dl_pack8(v);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
      }
      rs = rsqrtf(wave_sum_dpp(ss) / (float)p.K + p.eps);
    }
    for (int c = lane * 8; c < klen; c += 512) {
      if constexpr (NORM) {
        float v[8], wf[8];
        dl_xe8(p, m, kbeg + c, v);
        dl_load8(p.nw + kbeg + c, wf);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] * rs * wf[j];
        *reinterpret_cast<u16x8*>(xs + m * pitch + c) = dl_pack8(v);
      } else {
        *reinterpret_cast<u16x8*>(xs + m * pitch + c) =
            *reinterpret_cast<const u16x8*>(p.x + (int64_t)m * p.ldx + kbeg + c);
      }
    }
  }
  __syncthreads();

  // ---- the stream: lane l reads row (l & 15) of both row blocks at K offset 8 (l >> 4) of every step
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
  const bf16_t* wp[2] = {p.w + (int64_t)row[0] * p.ldw + kbeg + 8 * g, p.w + (int64_t)row[1] * p.ldw + kbeg + 8 * g};
  const bf16_t* xp = xs + li * pitch + 8 * g;
  const bool live = li < p.M;  // padding columns of B: zeros, nothing read
  const bf16x8 zero = {};
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  const int steps = klen / DL_KSTEP, trips = steps / DL_UNROLL;

  auto load_w = [&](int step, bf16x8(&a)[2][DL_UNROLL]) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int u = 0; u < DL_UNROLL; ++u)
        a[b][u] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp[b] + (step + u) * DL_KSTEP));
  };
  auto load_x = [&](int step) {
    return live ? *reinterpret_cast<const bf16x8*>(xp + step * DL_KSTEP) : zero;
  };

  bf16x8 a[2][DL_UNROLL], nx[2][DL_UNROLL];
  int t = wid;
  if (t < trips) load_w(t * DL_UNROLL, a);
  for (; t < trips; t += DL_WAVES) {
    const bool more = t + DL_WAVES < trips;
    if (more) load_w((t + DL_WAVES) * DL_UNROLL, nx);
#pragma unroll
    for (int u = 0; u < DL_UNROLL; ++u) {
      const bf16x8 b = load_x(t * DL_UNROLL + u);
      acc[0] = mfma16(a[0][u], b, acc[0]);
      acc[1] = mfma16(a[1][u], b, acc[1]);
    }
    if (more) {
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int u = 0; u < DL_UNROLL; ++u) a[b][u] = nx[b][u];
    }
  }
  for (int s = trips * DL_UNROLL + wid; s < steps; s += DL_WAVES) {  // the slice's last steps, fewer than a trip
    const bf16x8 b = load_x(s);
    acc[0] = mfma16(*reinterpret_cast<const bf16x8*>(wp[0] + s * DL_KSTEP), b, acc[0]);
    acc[1] = mfma16(*reinterpret_cast<const bf16x8*>(wp[1] + s * DL_KSTEP), b, acc[1]);
  }

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
      } else if constexpr (EPI == DL_EPI_F32) {
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
__global__ __launch_bounds__(256) void decode_linear_finish_kernel(const float* __restrict__ part, void* __restrict__ y,
                                                                   int64_t ldy, int M, int N, int nsplit) {
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

int dl_check_shape(int64_t m, int64_t n, int64_t k, int epilogue, int64_t split_k) {
  PICO_REQUIRE(epilogue == DL_EPI_BF16 || epilogue == DL_EPI_F32 || epilogue == DL_EPI_SWIGLU,
               "pico_decode_linear: unknown epilogue %d", epilogue);
  PICO_REQUIRE(m >= 0 && m <= DL_MAX_M, "pico_decode_linear: m=%lld rows; 1..%d are supported", (long long)m,
               DL_MAX_M);
  PICO_REQUIRE(k > 0 && k % DL_KSTEP == 0 && k <= (1 << 20), "pico_decode_linear: k=%lld must be a multiple of %d",
               (long long)k, DL_KSTEP);
  PICO_REQUIRE(n > 0 && n % 8 == 0 && n <= (1 << 24), "pico_decode_linear: n=%lld must be a multiple of 8",
               (long long)n);
  PICO_REQUIRE(epilogue != DL_EPI_SWIGLU || n % 16 == 0,
               "pico_decode_linear: SWIGLU takes the stacked gate|up matrix, n=%lld must be a multiple of 16",
               (long long)n);
  PICO_REQUIRE(split_k <= (1 << 20), "pico_decode_linear: bad split_k %lld", (long long)split_k);
  return 0;
}

int dl_check_plan(const DecodeLinearPlan& p) {
  PICO_REQUIRE(p.k_slice <= DL_MAX_SLICE,
               "pico_decode_linear: split_k leaves slices of %lld columns; at most %d fit the workgroup's LDS",
               (long long)p.k_slice, DL_MAX_SLICE);
  PICO_REQUIRE(p.blocks <= 0x7fffffff && p.split_k <= 65535, "pico_decode_linear: grid too large");
  return 0;
}

bool dl_overlap(const void* a, int64_t a_elems, const void* b, int64_t b_elems) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + 2 * (uintptr_t)b_elems && b0 < a0 + 2 * (uintptr_t)a_elems;
}

template <int EPI>
int dl_launch(const DecodeLinearPlan& pl, const DLParams& p, bool norm, int64_t ldy, hipStream_t s) {
  const unsigned lds = (unsigned)decode_linear_lds_bytes(p.M, pl.k_slice);
  const dim3 grid((unsigned)pl.blocks, (unsigned)pl.split_k);
  auto k = norm ? decode_linear_kernel<EPI, true> : decode_linear_kernel<EPI, false>;
  if (lds > 64 * 1024) {  // once per kernel and device: the largest request any plan makes
    static bool raised[2][64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!raised[norm][dev]) {
      const int most = (int)decode_linear_lds_bytes(DL_MAX_M, DL_MAX_SLICE);
      const hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, most);
      if (e != hipSuccess) return pico_set_error("pico_decode_linear: cannot set LDS size (%d)", (int)e);
      raised[norm][dev] = true;
    }
  }
  PICO_TRY(pico_launch(PICO_K_DECODE_LINEAR, "decode_linear", k, grid, dim3(DL_THREADS), lds, s, p));
  if (pl.split_k > 1) {
    const int64_t outs = EPI == DL_EPI_SWIGLU ? p.N / 2 : p.N;
    PICO_TRY(pico_launch(PICO_K_DECODE_LINEAR, "decode_linear_finish", decode_linear_finish_kernel<EPI>,
                         dim3((unsigned)pico_cdiv(p.M * outs, 256)), dim3(256), 0, s, p.part, p.y, ldy, p.M, p.N,
                         (int)pl.split_k));
  }
  return 0;
}

}  // namespace

extern "C" int64_t pico_decode_linear_args_size(void) { return (int64_t)sizeof(pico_decode_linear_args); }

extern "C" int64_t pico_decode_linear_split_k(int64_t n, int64_t k, int epilogue) {
  if (dl_check_shape(1, n, k, epilogue, 0)) return -1;
  return decode_linear_plan(1, n, k, epilogue, 0, pico_num_cus()).split_k;
}

extern "C" int64_t pico_decode_linear_workspace_bytes(int64_t m, int64_t n, int64_t k, int epilogue,
                                                      int64_t split_k) {
  if (dl_check_shape(m, n, k, epilogue, split_k)) return -1;
  const DecodeLinearPlan p = decode_linear_plan(m, n, k, epilogue, split_k, pico_num_cus());
  if (dl_check_plan(p)) return -1;
  return p.bytes;
}

extern "C" int pico_decode_linear(const pico_decode_linear_args* a, void* stream) {
  PICO_REQUIRE(a && a->x && a->weight && a->y, "pico_decode_linear: null pointer");
  PICO_TRY(dl_check_shape(a->m, a->n, a->k, a->epilogue, a->split_k));
  const int64_t outs = a->epilogue == DL_EPI_SWIGLU ? a->n / 2 : a->n;
  PICO_REQUIRE(a->ldx % 8 == 0 && a->ldw % 8 == 0 && a->ldy % 8 == 0 && a->ldx >= a->k && a->ldw >= a->k &&
                   a->ldy >= outs,
               "pico_decode_linear: row strides must be multiples of 8 elements and cover a row");
  PICO_REQUIRE(((uintptr_t)a->x | (uintptr_t)a->weight | (uintptr_t)a->y | (uintptr_t)a->norm_weight |
                (uintptr_t)a->residual | (uintptr_t)a->residual_out | (uintptr_t)a->workspace) % 16 == 0,
               "pico_decode_linear: pointers must be 16-byte aligned");
  const bool norm = a->norm_weight != nullptr;
  PICO_REQUIRE(norm || (!a->residual && !a->residual_out),
               "pico_decode_linear: residual / residual_out belong to the norm prologue (norm_weight is null)");
  if (a->residual)
    PICO_REQUIRE(a->ldr % 8 == 0 && a->ldr >= a->k, "pico_decode_linear: bad residual row stride %lld",
                 (long long)a->ldr);
  if (a->residual_out) {
    PICO_REQUIRE(a->ldro % 8 == 0 && a->ldro >= a->k, "pico_decode_linear: bad residual_out row stride %lld",
                 (long long)a->ldro);
    const int64_t rows = a->m > 0 ? a->m - 1 : 0;
    const int64_t ro = rows * a->ldro + a->k;
    PICO_REQUIRE(!dl_overlap(a->residual_out, ro, a->x, rows * a->ldx + a->k) &&
                     !(a->residual && dl_overlap(a->residual_out, ro, a->residual, rows * a->ldr + a->k)),
                 "pico_decode_linear: residual_out must not alias x or residual (other workgroups still read them)");
  }
  const DecodeLinearPlan pl = decode_linear_plan(a->m, a->n, a->k, a->epilogue, a->split_k, pico_num_cus());
  PICO_TRY(dl_check_plan(pl));
  PICO_REQUIRE(pl.split_k == 1 || a->workspace, "pico_decode_linear: a K split needs the workspace");
  if (a->m == 0) return 0;
  DLParams p{};
  p.x = (const bf16_t*)a->x;
  p.res = (const bf16_t*)a->residual;
  p.nw = (const bf16_t*)a->norm_weight;
  p.res_out = (bf16_t*)a->residual_out;
  p.w = (const bf16_t*)a->weight;
  p.y = a->y;
  p.part = (float*)a->workspace;
  p.ldx = a->ldx, p.ldr = a->ldr, p.ldro = a->ldro, p.ldw = a->ldw, p.ldy = a->ldy;
  p.M = (int)a->m, p.N = (int)a->n, p.K = (int)a->k, p.k_slice = (int)pl.k_slice;
  p.eps = a->eps;
  hipStream_t s = (hipStream_t)stream;
  switch (a->epilogue) {
    case DL_EPI_BF16: return dl_launch<DL_EPI_BF16>(pl, p, norm, a->ldy, s);
    case DL_EPI_F32: return dl_launch<DL_EPI_F32>(pl, p, norm, a->ldy, s);
    default: return dl_launch<DL_EPI_SWIGLU>(pl, p, norm, a->ldy, s);
  }
}
