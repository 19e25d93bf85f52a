/*
 * picotron_hip.h — C ABI of the MI355X (gfx950) hot-path kernels of picotron_amd.
 *
 * The reference (rkinas/picotron) is pure Python; its native arithmetic lives in
 * flash-attn 2.5.0 (CUDA + Triton) and torch ATen/NCCL. Each entry point below replaces one
 * of those third-party calls made from the reference's model / data-parallel code:
 *
 *   pico_rmsnorm_fwd / _bwd   <- flash_attn.ops.triton.layer_norm.layer_norm_fn(is_rms_norm=True)
 *                                 called by TritonRMSNorm.forward   (ref picotron/model.py:50-64)
 *                                 eager oracle LlamaRMSNorm          (ref picotron/model.py:66-85)
 *   pico_rope                 <- flash_attn.layers.rotary.apply_rotary_emb(x, cos, sin, interleaved=False)
 *                                 called by Attention.forward         (ref picotron/model.py:135-136)
 *                                 (conjugate=1 is its backward: rotation by -theta)
 *   pico_swiglu_fwd / _bwd    <- F.silu(gate(x)) * up(x)             (ref picotron/model.py:185)
 *   pico_attn_fwd / _bwd      <- flash_attn_func(q, k, v, causal)     (ref picotron/model.py:32-36,153)
 *                                 and the ring-attention block fwd/bwd
 *                                 (ref picotron/context_parallel/context_parallel.py:112-155)
 *   pico_attn_merge           <- update_out_and_lse                  (ref .../context_parallel.py:157-187)
 *   pico_grad_accum           <- param.main_grad.add_(param.grad)    (ref picotron/data_parallel/data_parallel.py:131)
 *                                 fused with Bucket.sync_gradient's grad_data /= W
 *                                                                      (ref picotron/data_parallel/bucket.py:30)
 *   pico_cast_f32_bf16        <- p.grad = p.main_grad.to(p.dtype)    (ref picotron/data_parallel/data_parallel.py:165)
 *   pico_scale_f32            <- grad_data /= process_group_size     (ref picotron/data_parallel/bucket.py:30)
 *   pico_cross_entropy_fwd/_bwd <- F.cross_entropy(logits, target, reduction='mean')
 *                                 (ref train.py:46-49, picotron/pipeline_parallel/pipeline_parallel.py:68,98)
 *   pico_ce_vp_partial / _combine / _grad
 *                             <- the same loss under tensor parallelism on each rank's vocabulary shard of the
 *                                 logits, instead of the LM head's all-gather followed by the full-vocabulary loss
 *                                 (ref picotron/tensor_parallel/tensor_parallel.py:50, gather_output=True)
 *   pico_adamw_bf16           <- torch.optim.AdamW(..., fused=True).step() (ref train.py:204-209,235)
 *   pico_grad_sqnorm / _clip_coef / _scale, pico_adamw_bf16_clip
 *                             <- torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm): no reference call
 *                                 (the reference trains unclipped); what a Llama pre-training recipe adds between
 *                                 the last backward and optimizer.step() (ref train.py:235)
 *   pico_adamw_master         <- the same step on fp32 master weights and fp32 moments (mixed-precision recipes'
 *                                 optimizer; no reference call: the reference's AdamW steps the bf16 tensors)
 *   pico_adamw_bf16_sr, pico_sr_round_bf16
 *                             <- the bf16 step with stochastically rounded stores (torchao / optimi
 *                                 bf16_stochastic_round; no reference call), and the rounding alone
 *   pico_muon_momentum / _normalize / _update
 *                             <- the elementwise half of torch.optim.Muon's step (no reference call: the
 *                                 reference trains with AdamW alone)
 *   pico_sort_ids             <- the stable id sort inside F.embedding's backward (ref picotron/model.py:223-224)
 *   pico_embedding_bwd        <- backward of F.embedding (ref picotron/model.py:223-224) + the micro-batch
 *                                 gradient accumulation (data_parallel.py:131 / autograd's grad += dW)
 *   pico_transpose_bf16       <- no reference call: lays out x^T / W^T for the faster hipBLASLt forms of
 *                                 the nn.Linear wgrad / dgrad GEMMs (ref picotron/model.py nn.Linear)
 *   pico_kv_append, pico_attn_decode
 *                             <- no reference call: KV-cache generation (picotron_amd/generate.py)
 *   pico_sample               <- no reference call: the fused next-token sampler of generation (temperature,
 *                                 top-k, top-p, counter-based draw; all per-step state on the device)
 *
 * Conventions: all pointers are device pointers allocated by the caller (kernels never
 * allocate); bf16 tensors are passed as raw 16-bit storage; `stream` is a hipStream_t
 * (the caller's current stream). Every function returns 0 on success or a non-zero
 * status (hipError_t value, or PICO_EINVAL for argument errors); pico_last_error()
 * returns the message for the calling thread. No C++ exception crosses the ABI.
 */
#ifndef PICOTRON_HIP_H
#define PICOTRON_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PICO_ABI_VERSION 2
#define PICO_EINVAL 1000

/* kernel ids for the optional event timer (pico_prof_*) */
enum {
  PICO_K_RMSNORM_FWD = 1,
  PICO_K_RMSNORM_BWD = 2,
  PICO_K_RMSNORM_DW = 3,
  PICO_K_ROPE = 4,
  PICO_K_SWIGLU_FWD = 5,
  PICO_K_SWIGLU_BWD = 6,
  PICO_K_ATTN_FWD = 7,
  PICO_K_ATTN_BWD_PRE = 8, /* 8-10: retired with round 1's fused backward (kept so later ids stay stable) */
  PICO_K_ATTN_BWD = 9,
  PICO_K_ATTN_BWD_DQ = 10,
  PICO_K_GRAD_ACCUM = 11,
  PICO_K_CAST = 12,
  PICO_K_SCALE = 13,
  PICO_K_ATTN_MERGE = 14,
  PICO_K_EMBEDDING_BWD = 15,
  PICO_K_CE_FWD = 16,
  PICO_K_CE_BWD = 17,
  PICO_K_TRANSPOSE = 18,
  PICO_K_ATTN_BWD_DKV = 19,
  PICO_K_SORT_IDS = 20,
  PICO_K_ADAMW = 21,
  PICO_K_ATTN_BWD_KV = 22, /* split backward: dK/dV key-major kernel */
  PICO_K_ATTN_BWD_Q = 23,  /* split backward: dQ query-major kernel (+ delta, LSE*log2e) */
  PICO_K_GRAD_SQNORM = 24, /* global gradient norm: the per-chunk sum-of-squares kernel */
  PICO_K_GRAD_SCALE = 25,  /* standalone gradient clip (pico_adamw_bf16_clip is timed under PICO_K_ADAMW) */
  PICO_K_COUNT = 26
};

int pico_abi_version(void);
const char* pico_last_error(void);

/* ---- event timer: times every launch of the enabled kernel ids on the stream each is launched on ----
 * pico_prof_enable(id, capacity) enables id (up to `capacity` timed launches); id <= 0 disables all.
 * pico_prof_collect(id, ...) synchronises the recorded events, returns their summed duration and
 * count, and resets that id's pool. */
int pico_prof_enable(int kernel_id, int capacity);
int pico_prof_collect(int kernel_id, double* total_ms, int64_t* launches);

/* ---- kernel selection (A/B switches; process-wide, read by every later launch) ----
 * Each knob starts at its shipped default (PICO_SEL_AUTO = the library's shape rule), overridden ONCE, when the
 * library is loaded, by the environment variable named beside it; pico_select(knob, value) sets it afterwards
 * (value PICO_SEL_AUTO restores the rule). Returns the previous value, or -2 for an unknown knob. No launch reads
 * the environment. */
#define PICO_SEL_AUTO (-1)
enum {
  PICO_SEL_ATTN_KVP = 0,    /* PICO_ATTN_KVP: dK/dV kernel, 1 = 64-row (attn_bwd_kvp_kernel at D=64,
                               attn_bwd_kvp128_kernel at D=128), 0 = 32-row kernel */
  PICO_SEL_KVP_WAVES = 1,   /* PICO_KVP_WAVES: waves per attn_bwd_kvp_kernel workgroup, 4 or 8 */
  PICO_SEL_ATTN_GROUPS = 2, /* PICO_ATTN_GROUPS: one-round block groups of the causal dK/dV grid, 1 on / 0 off */
  PICO_SEL_ATTN_FWD = 3,    /* PICO_ATTN_FWD: 1 = the persistent 64-row-per-wave forward (opt-in, measured slower) */
  PICO_SEL_COUNT = 4
};
int pico_select(int knob, int value);

/* ---- RMSNorm: y = x * rsqrt(mean(x^2) + eps) * w, fp32 math, one bf16 rounding ----
 * x, y: [rows, cols] bf16 row-major (row stride = cols); w: [cols] bf16; rstd: [rows] fp32 (saved
 * for backward). residual (optional, may be NULL): x_eff = bf16(x + residual), written to
 * residual_out when residual_out != NULL (layer_norm_fn(prenorm=True) semantics). */
/* pico_rmsnorm_fwd that also writes y^T ([cols, rows], row stride ld_t): the x^T the next projection's
 * weight-gradient GEMM reads. cols 1024 or 2048, rows multiple of 32, 16-byte aligned pointers. */
int pico_rmsnorm_fwd_t(const void* x, const void* residual, const void* weight, void* y, void* residual_out,
                       float* rstd, void* y_t, int64_t ld_t, int64_t rows, int64_t cols, float eps, void* stream);
int pico_rmsnorm_fwd(const void* x, const void* residual, const void* weight, void* y,
                     void* residual_out, float* rstd, int64_t rows, int64_t cols, float eps,
                     void* stream);
int64_t pico_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t cols);
/* dx: [rows, cols] bf16; dweight: [cols] bf16; workspace >= pico_rmsnorm_bwd_workspace_bytes.
 * dresidual (optional, may be NULL): added into dx (gradient flowing through residual_out). */
int pico_rmsnorm_bwd(const void* dy, const void* dresidual, const void* x, const void* weight,
                     const float* rstd, void* dx, void* dweight, void* workspace, int64_t rows,
                     int64_t cols, void* stream);
/* As pico_rmsnorm_bwd, with the weight gradient's micro-batch accumulation folded in (the
 * reference's AccumulateGrad `grad += dw` at DP = 1 / DataParallelBucket's `main_grad += grad`,
 * ref picotron/data_parallel/data_parallel.py:131, and the bucket's /W, bucket.py:30):
 *   dw_mode 0: dweight (bf16)  = sum                      (== pico_rmsnorm_bwd)
 *   dw_mode 1: dweight (bf16)  = bf16(dweight + sum)       (one rounding)
 *   dw_mode 2: dweight (fp32)  = (dweight + sum) * dw_scale */
int pico_rmsnorm_bwd_acc(const void* dy, const void* dresidual, const void* x, const void* weight,
                         const float* rstd, void* dx, void* dweight, int dw_mode, float dw_scale,
                         void* workspace, int64_t rows, int64_t cols, void* stream);
/* Chained form (one launch per norm instead of two): as pico_rmsnorm_bwd_acc, but
 *   reduce_own = 0 leaves this call's dw partial rows (pico_rmsnorm_bwd_partial_rows of them, [nb][cols]
 *     fp32) in `workspace` for a later call to reduce (dweight / dw_mode / dw_scale unused);
 *   prev_part != NULL: the same launch also reduces a previous call's partial rows ([prev_nb][prev_cols],
 *     still alive in the caller's memory) into prev_dweight with prev_mode / prev_scale.
 * pico_rmsnorm_dw_reduce does that reduction alone (the last norm of a backward pass). Deterministic: every
 * dw sum runs in a fixed order. */
int pico_rmsnorm_bwd_chain(const void* dy, const void* dresidual, const void* x, const void* weight,
                           const float* rstd, void* dx, void* dweight, int dw_mode, float dw_scale,
                           void* workspace, int64_t rows, int64_t cols, int reduce_own,
                           const float* prev_part, int64_t prev_nb, int64_t prev_cols, void* prev_dweight,
                           int prev_mode, float prev_scale, void* stream);
int64_t pico_rmsnorm_bwd_partial_rows(int64_t rows, int64_t cols);
int pico_rmsnorm_dw_reduce(const float* part, int64_t nb, int64_t cols, void* dweight, int dw_mode,
                           float dw_scale, void* stream);

/* ---- RoPE, rotate-half (non-interleaved) layout ----
 * x, out: [batch, seqlen, heads, head_dim] bf16 with element strides (batch, seq, head) and
 * unit last-dim stride (out may alias x). cos/sin: [seqlen, >= head_dim/2] bf16 tables with
 * row stride cs_stride (elements); element i < head_dim/2 of row s is cos(s * theta_i).
 * out[..., i]       = x[i] * c - x[i + D/2] * s
 * out[..., i + D/2] = x[i + D/2] * c + x[i] * s        (conjugate: s -> -s, the backward) */
int pico_rope(const void* x, void* out, const void* cos, const void* sin, int64_t batch,
              int64_t seqlen, int64_t heads, int64_t head_dim, const int64_t* x_strides,
              const int64_t* out_strides, int64_t cs_stride, int conjugate, void* stream);

/* ---- SwiGLU epilogue: h = silu(g) * u on [rows, cols] bf16 ----
 * gate/up (and dgate/dup) rows at element stride in_stride (they may be the two column halves of one
 * fused gate|up GEMM output, in_stride = 2*cols); out/dout rows at out_stride. */
/* pico_swiglu_fwd that also writes out^T ([cols, rows], row stride t_stride): the down projection's
 * x^T for its weight-gradient GEMM. rows, cols multiples of 64; strides multiples of 8. */
int pico_swiglu_fwd_t(const void* gate, const void* up, void* out, void* out_t, int64_t rows, int64_t cols,
                      int64_t in_stride, int64_t out_stride, int64_t t_stride, void* stream);
int pico_swiglu_fwd(const void* gate, const void* up, void* out, int64_t rows, int64_t cols,
                    int64_t in_stride, int64_t out_stride, void* stream);
int pico_swiglu_bwd(const void* dout, const void* gate, const void* up, void* dgate, void* dup,
                    int64_t rows, int64_t cols, int64_t in_stride, int64_t out_stride, void* stream);

/* ---- Flash attention (bf16 MFMA, online softmax, fp32 LSE) ----
 * Layouts: q/o/do/dq [B, Sq, Hq, D], k/v/dk/dv [B, Sk, Hkv, D] with element strides
 * (batch, seq, head) and unit last-dim stride; lse [B, Hq, Sq] fp32 contiguous (natural log,
 * lse = log sum_j exp(scale * q.k_j)). Hq % Hkv == 0 (GQA: query head h uses kv head h/(Hq/Hkv)).
 * head_dim in {64, 128}. causal requires Sq == Sk (top-left aligned mask j <= i). */
typedef struct pico_attn_args {
  const void* q;
  const void* k;
  const void* v;
  void* o;          /* fwd output / bwd input */
  float* lse;       /* fwd output / bwd input */
  const void* dout; /* bwd */
  void* dq;         /* bwd out (bf16, or fp32 accumulate with PICO_ATTN_DQ_F32_ACCUM) */
  void* dk;         /* bwd out bf16 */
  void* dv;         /* bwd out bf16 */
  void* workspace;  /* bwd: >= pico_attn_bwd_workspace_bytes */
  int64_t batch, seqlen_q, seqlen_k, heads_q, heads_kv, head_dim;
  int64_t q_strides[3], k_strides[3], v_strides[3], o_strides[3];
  int64_t do_strides[3], dq_strides[3], dk_strides[3], dv_strides[3];
  float softmax_scale;
  int causal;
  int flags;
  /* PICO_ATTN_ROPE_BWD: bf16 rotate-half tables [>= S, D/2] (row stride rope_stride elements) */
  const void* rope_cos;
  const void* rope_sin;
  int64_t rope_stride;
  /* fwd, optional (NULL: off): O also written transposed, o_t[hq * D + d][b * Sq + q] with row stride
   * o_t_ld elements — the [Hq*D, tokens] layout of the out-projection input that its weight-gradient
   * GEMM reads fastest (x^T), written from the accumulator layout at no extra pass */
  void* o_t;
  int64_t o_t_ld;
} pico_attn_args;

#define PICO_ATTN_DQ_F32_ACCUM 1 /* dq is fp32 [B,Sq,Hq,D] (dq_strides) and is ADDED into */
/* bwd: q and k were rotated (RoPE, rotate-half, position = sequence index) before attention; dq and dk
 * are returned rotated back by -theta (the RoPE backward, ref picotron/model.py:135-136), fused into
 * the dQ slab sum and the dK epilogue. Not combinable with PICO_ATTN_DQ_F32_ACCUM. */
#define PICO_ATTN_ROPE_BWD 2
/* fwd: q holds UNROTATED queries; each row is rotated (RoPE, rotate-half, position = sequence index,
 * tables as for ROPE_BWD) in registers before use, and the rotated rows are written to dq (dq_strides;
 * dq may alias q) for the backward. Replaces the query half of the separate pico_rope launch. */
#define PICO_ATTN_ROPE_Q_FWD 4

int64_t pico_attn_args_size(void); /* sizeof(pico_attn_args), for FFI layout checks */
int pico_attn_fwd(const pico_attn_args* args, void* stream);
int64_t pico_attn_bwd_workspace_bytes(const pico_attn_args* args);
int pico_attn_bwd(const pico_attn_args* args, void* stream);

/* ---- ring-attention block merge (update_out_and_lse) ----
 * ref picotron/context_parallel/context_parallel.py:157-187:
 *   first != 0: out = float(block_out), lse = block_lse
 *   otherwise:  out -= sigmoid(block_lse - lse) * (out - block_out); lse -= logsigmoid(lse - block_lse)
 * Every operand by element strides, so the reference's layout (out [B, H, S, D] fp32 and lse [B, H, S, 1],
 * or slices of them, ref :183-186) and the ring's internal [B, S, H, D] one use the same entry point:
 * out fp32, strides (batch, seq, head), unit head_dim stride; lse fp32, strides (batch, head, seq);
 * block_out bf16 (block_out_f32 == 0) or fp32, strides (batch, seq, head), unit head_dim stride;
 * block_lse fp32, strides (batch, head, seq). out and block_out rows 16-byte aligned. head_dim: any multiple
 * of 8 up to 256; batch * seqlen < 2^31. */
int pico_attn_merge(float* out, const int64_t* out_strides, float* lse, const int64_t* lse_strides,
                    const void* block_out, const int64_t* block_out_strides, int block_out_f32,
                    const float* block_lse, const int64_t* block_lse_strides, int64_t batch, int64_t seqlen,
                    int64_t heads, int64_t head_dim, int first, void* stream);

/* ---- DP gradient buckets ---- */
/* main_grad[i] = (main_grad[i] + float(grad[i])) * (1.0f / divide_by)   (divide_by == 1: no scaling).
 * The fp32 reciprocal product is what ATen computes for the reference's `grad_data /= W` on a GPU. */
int pico_grad_accum(float* main_grad, const void* grad, int64_t n, float divide_by, void* stream);
/* buf[i] = buf[i] * (1.0f / divide_by) */
int pico_scale_f32(float* buf, int64_t n, float divide_by, void* stream);
/* dst[i] = bf16(src[i]) (round to nearest even) */
int pico_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream);

/* ---- token embedding backward (deterministic, graph-safe) ----
 * sorted_ids / sorted_pos: the n_tokens token ids stable-sorted ascending and their positions
 * (int64, device). dy: [n_tokens, dim] bf16. grad: [vocab, dim] bf16 (grad_is_f32 = 0) or fp32;
 * for every id present: grad[id] = (grad[id] + sum of its dy rows in position order) * scale. */
int pico_embedding_bwd(const int64_t* sorted_ids, const int64_t* sorted_pos, const void* dy, void* grad,
                       int64_t n_tokens, int64_t dim, int grad_is_f32, float scale, void* stream);
/* Stable ascending sort of n <= 8192 token ids in [0, vocab), vocab <= 2^19 (int64, device) with their
 * positions: the input pico_embedding_bwd wants, bit-identical to torch.sort(ids, stable=True)
 * (which the reference's F.embedding backward does inside ATen). One workgroup, LDS bitonic sort of
 * (id << 13 | position) keys. */
int pico_sort_ids(const int64_t* ids, int64_t n, int64_t vocab, int64_t* sorted_ids, int64_t* sorted_pos,
                  void* stream);

/* ---- AdamW step over a whole parameter list (one launch) ----
 * Replaces torch.optim.AdamW(params, lr, fused=True).step() (ref train.py:13,204-209,235) for bf16
 * parameters with bf16 exp_avg / exp_avg_sq (torch keeps the states in the parameter dtype).
 * tensors: device int64 [n_tensors][5] = (param, grad, exp_avg, exp_avg_sq addresses, grad_is_f32);
 * grad_is_f32 != 0: grad is an fp32 buffer (DataParallelBucket's averaged main_grad with the bf16 .grad
 * cast deferred, ref picotron/data_parallel/data_parallel.py:165), rounded to bf16 in register exactly as
 * pico_cast_f32_bf16 stores it — bit-identical to cast-then-step; sizes: device int64 [n_tensors] numel; chunks: device int64 [n_chunks][2] = (tensor index, first element), one
 * per pico_adamw_chunk_elems() elements of each tensor. step: the step number after increment (>= 1).
 * Same expression order and types as ATen's fused AdamW (decoupled weight decay). */
int64_t pico_adamw_chunk_elems(void);
int pico_adamw_bf16(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks, int64_t n_chunks,
                    double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                    void* stream);

/* ---- global L2 gradient norm and clip over a whole parameter list, on pico_adamw_bf16's device tables ----
 * Replaces torch.nn.utils.clip_grad_norm_(params, max_norm) (norm_type 2). Only the grad and grad_is_f32 columns
 * of `tensors` are read; an fp32 main_grad element counts as bf16(g), the value the deferred cast would store.
 * pico_grad_sqnorm: one launch writes one fp32 partial sum of squares per chunk into workspace
 * (>= pico_grad_sqnorm_workspace_bytes(n_chunks)), a second adds them in index order in double and stores
 * *sumsq (device double). No atomics: the same tables and data give the same bits on every run. n_chunks = 0
 * stores 0. The caller may all-reduce *sumsq over its model-parallel groups before pico_grad_clip_coef. */
int64_t pico_grad_sqnorm_workspace_bytes(int64_t n_chunks);
int pico_grad_sqnorm(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks, int64_t n_chunks,
                     void* workspace, double* sumsq, void* stream);
/* norm_coef (device float[2]): [0] = (float)sqrt(*sumsq), the total norm; [1] = fminf(1, (float)max_norm /
 * ([0] + 1e-6f)), torch's clip coefficient. max_norm >= 0 (NaN is rejected). */
int pico_grad_clip_coef(const double* sumsq, double max_norm, float* norm_coef, void* stream);
/* The standalone clip, in place: bf16 g = bf16(float(g) * coef); fp32 main_grad g32 = float(bf16(float(bf16(g32))
 * * coef)), the value the bf16 form would hold, so a later deferred-cast step rounds it to the same bits. Nothing
 * is written when coef == 1 (the stored bf16 values would not change) or when the norm is not finite. */
int pico_grad_scale(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks, int64_t n_chunks,
                    const float* norm_coef, void* stream);
/* pico_adamw_bf16 with g replaced by bf16(g * norm_coef[1]) in register: bit-identical to pico_grad_scale followed
 * by pico_adamw_bf16 without the gradient write and re-read, and to pico_adamw_bf16 itself when the coefficient
 * is 1. If norm_coef[0] is not finite (an inf / NaN gradient) the kernel writes nothing: parameters and both
 * moments stay as they were. The host never reads the norm, so the caller's step counter still advances. */
int pico_adamw_bf16_clip(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks, int64_t n_chunks,
                         double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                         const float* norm_coef, void* stream);

/* ---- AdamW on fp32 master weights and fp32 moments under the bf16 model parameters, one launch ----
 * The Megatron / DeepSpeed / torch-AMP arrangement (no reference call: the reference steps bf16 tensors). `tensors`
 * keeps pico_adamw_bf16's [n_tensors][5] layout (pico_grad_sqnorm / pico_grad_scale work on it unchanged), but its
 * exp_avg / exp_avg_sq columns point at FP32 buffers and its param column at the bf16 model parameter, which is
 * written as bf16(master), round to nearest even, and never read. masters: device int64 [n_tensors], the fp32
 * master parameter addresses. The gradient value is the bf16 kernels' (bf16 .grad, or bf16(main_grad) when
 * grad_is_f32); the update is ATen's fused AdamW on fp32 tensors (double hyper-parameters, same expression order);
 * master and both moments are stored as fp32. norm_coef NULL: no clip; else as pico_adamw_bf16_clip (g = bf16(g *
 * norm_coef[1]); nothing is written when norm_coef[0] is not finite). 28 bytes per element (30 with an fp32
 * main_grad). Timed under PICO_K_ADAMW. */
int pico_adamw_master(const int64_t* tensors, const int64_t* masters, const int64_t* sizes, const int64_t* chunks,
                      int64_t n_chunks, double lr, double beta1, double beta2, double eps, double weight_decay,
                      int64_t step, const float* norm_coef, void* stream);

/* ---- the bf16 AdamW step with stochastic rounding of the parameter and both moments, one launch ----
 * pico_adamw_bf16 (same tables, same 14 bytes per element, bf16 state), but each of the three stores rounds the
 * fp32 result x (bit pattern u) to one of its two bf16 neighbours with probability proportional to distance
 * ("Revisiting BFloat16 Training"; torchao / optimi bf16_stochastic_round): inf / NaN store bf16(x) as before;
 * otherwise t = u + r with 16 random bits r, t = u if that carried a finite value to inf, and t >> 16 is stored.
 * The magnitude rounds up with probability (u & 0xFFFF) / 65536: the expectation is x and a value exact in bf16
 * never changes, so updates below half an ulp and slow decays survive on average.
 * r comes from Philox4x32-10 evaluated in registers (no generator state in memory): key = (seed low, seed high
 * 32 bits), counter = (uint32(i >> 3), uint32(ids[tensor]), uint32(step), q) for element i of the tensor and
 * quantity q (0 parameter, 1 exp_avg, 2 exp_avg_sq); the four output words w hold the values of elements i & ~7 ..
 * i | 7, element j = i & 7 taking (w[j >> 1] >> (16 * (j & 1))) & 0xFFFF. A step is a pure function of (seed,
 * step, id, element): the same bits on the vector and the scalar path, under any chunking, graph replay and after
 * a checkpoint resume. ids: device int64 [n_tensors], the generator's tensor ids (the caller keeps them distinct
 * and stable). step < 2^32; tensors of fewer than 2^35 elements (the caller's duty: sizes live on the device).
 * norm_coef NULL: no clip; else as pico_adamw_bf16_clip. Timed under PICO_K_ADAMW. */
int pico_adamw_bf16_sr(const int64_t* tensors, const int64_t* ids, const int64_t* sizes, const int64_t* chunks,
                       int64_t n_chunks, double lr, double beta1, double beta2, double eps, double weight_decay,
                       int64_t step, const float* norm_coef, uint64_t seed, void* stream);
/* The rounding of pico_adamw_bf16_sr alone: dst[i] (bf16) = the stochastic rounding of src[i] (fp32) with the bits
 * of (seed, step, id, quantity, i), e.g. to convert an fp32 checkpoint. 8 elements per lane when src is 32-byte
 * and dst 16-byte aligned (then a scalar tail of n % 8), one element per lane otherwise: the same bits either way.
 * n < 2^35, 0 <= step, id < 2^32, quantity 0..2. Timed under PICO_K_CAST. */
int pico_sr_round_bf16(const float* src, void* dst, int64_t n, uint64_t seed, int64_t step, int64_t id, int quantity,
                       void* stream);

/* ---- Muon's elementwise passes over a whole list of bf16 matrices, on pico_adamw_bf16's device tables ----
 * torch.optim.Muon's rounding points (fp32 arithmetic, each named result rounded once to bf16, nearest even); the
 * Newton-Schulz GEMMs between pico_muon_normalize and pico_muon_update are the caller's (hipBLASLt).
 * tensors: device int64 [n_tensors][5] = (param, grad, momentum_buffer, work addresses, grad_is_f32), so
 * pico_grad_sqnorm / pico_grad_scale work on it unchanged; work: the tensor's bf16 slice of the Newton-Schulz input
 * buffer. sizes / chunks as pico_adamw_bf16. The gradient value g is the AdamW kernels' (bf16 .grad, or
 * bf16(main_grad) when grad_is_f32). lerp(a, b, w) is ATen's: |w| < 0.5 ? a + w (b - a) : b - (b - a)(1 - w), w
 * cast to fp32. No atomics: the same inputs give the same bits on every run. All timed under PICO_K_ADAMW.
 * pico_muon_momentum: m' = bf16(lerp(m, g, 1 - momentum)) -> momentum_buffer; u = bf16(lerp(g, m', momentum)) when
 * nesterov, else m', -> work; partials[c] (device float [n_chunks]) = the fp32 sum of squares of the bf16 u values
 * of chunk c, in pico_grad_sqnorm's summation order. 8 bytes per element (10 with an fp32 main_grad). */
int pico_muon_momentum(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks, int64_t n_chunks,
                       double momentum, int nesterov, float* partials, void* stream);
/* Two launches. norms[t] (device float [n_tensors]) = max(float(bf16(sqrt(s_t))), (float)eps), s_t = partials[
 * chunk_start[t] .. chunk_start[t + 1]) added in index order in double: torch's bf16 norm().clamp(min=eps).
 * chunk_start: device int64 [n_tensors + 1], the first chunk of each tensor (chunks holds each tensor's chunks
 * together, tensors in order). Then work = bf16(work / norms[t]) in place, a true division. 4 bytes per element. */
int pico_muon_normalize(const int64_t* tensors, const int64_t* sizes, const int64_t* chunks, int64_t n_chunks,
                        const int64_t* chunk_start, int64_t n_tensors, const float* partials, double eps,
                        float* norms, void* stream);
/* p = bf16(p * (float)(1 - lr * weight_decay)), then p = bf16(p + (float)(-(lr * ratios[t])) * O): torch's mul_
 * followed by add_(O, alpha=-adjusted_lr), two roundings, the scalars formed in double. out_ptrs: device int64
 * [n_tensors], the address of each tensor's O (bf16, contiguous, the parameter's shape); ratios: device double
 * [n_tensors], torch's _adjust_lr ratio of each shape. 6 bytes per element. */
int pico_muon_update(const int64_t* tensors, const int64_t* out_ptrs, const int64_t* sizes, const int64_t* chunks,
                     int64_t n_chunks, double lr, double weight_decay, const double* ratios, void* stream);

/* ---- softmax cross-entropy (mean over non-ignored rows) ----
 * logits: [rows, vocab] bf16, row stride ld (elements); target: [rows] int64.
 * fwd: lse[i] = log sum_j exp(logits[i][j]) (fp32), loss[i] = lse[i] - logits[i][target[i]] (0 for
 *      target == ignore_index). The caller sums loss[] and divides by the non-ignored count.
 * bwd: dlogits[i][j] = (exp(logits[i][j] - lse[i]) - [j == target[i]]) * (*grad_scale) (0 rows for
 *      ignored targets); grad_scale is a DEVICE fp32 scalar (grad_out / n_valid), row stride ldd. */
int pico_cross_entropy_fwd(const void* logits, int64_t ld, const int64_t* target, float* lse, float* loss,
                           int64_t rows, int64_t vocab, int64_t ignore_index, void* stream);
/* fused forward + gradient: as pico_cross_entropy_fwd, and the logits are overwritten IN PLACE with
 * (softmax - onehot) * (*grad_scale) (device fp32 scalar; 0 rows for ignored targets) — the gradient of
 * mean CE for a unit upstream gradient, which the caller scales after the LM-head GEMMs. */
int pico_cross_entropy_fwd_grad(void* logits, int64_t ld, const int64_t* target, float* lse, float* loss,
                                const float* grad_scale, int64_t rows, int64_t vocab, int64_t ignore_index,
                                void* stream);
/* The mean's scalars around pico_cross_entropy_fwd_grad, one launch each (instead of the ATen scalar ops of
 * F.cross_entropy(reduction='mean')'s host code): pico_ce_count writes stats[0] = #(target != ignore_index),
 * stats[1] = grad_scale / stats[0] (pass stats + 1 as fwd_grad's grad_scale); pico_ce_mean writes
 * grad_scale * sum(loss_rows) / stats[0] to *out (bf16, or fp32 when out_f32), summed in a fixed order,
 * and when acc is non-null adds the stored value to *acc (fp32): the training loop's per-step loss sum
 * (ref train.py:53 `loss_acc += loss.item()`), kept on the device without a separate launch. */
int pico_ce_count(const int64_t* target, int64_t n, int64_t ignore_index, float grad_scale, float* stats,
                  void* stream);
int pico_ce_mean(const float* loss_rows, int64_t n, const float* stats, float grad_scale, void* out, int out_f32,
                 float* acc, void* stream);
/* backward of the fused LM-head CE: dx (bf16, contiguous, n elements) *= *upstream (the loss's upstream
 * gradient, a device 0-dim bf16 tensor, or fp32 when upstream_f32, rounded to bf16 first as ATen does),
 * fp32 product, one bf16 rounding.
 * Replaces autograd's scaling of the reference's logits gradient (ref picotron/model.py:269, train.py:46-49).
 * nonunit (optional, device int): set to 1 if the upstream gradient is not exactly 1 (the chunked LM-head CE
 * accumulated its weight gradient in the forward for a unit upstream; the host checks the flag later). */
int pico_ce_scale_grad(void* dx, int64_t n, const void* upstream, int upstream_f32, int* nonunit, void* stream);
int pico_cross_entropy_bwd(const void* logits, int64_t ld, const int64_t* target, const float* lse,
                           const float* grad_scale, void* dlogits, int64_t ldd, int64_t rows, int64_t vocab,
                           int64_t ignore_index, void* stream);

/* ---- vocab-parallel softmax cross-entropy (tensor parallelism) ----
 * Every tp rank holds the columns [vocab_start, vocab_start + vocab_local) of the [rows, vocab_total] logits:
 * logits is this rank's [rows, vocab_local] bf16 shard, row stride ld (elements); target: [rows] int64 on the
 * GLOBAL vocabulary. The softmax statistics are split across the shards, so the caller all-gathers three fp32
 * numbers per row between partial and combine instead of the logits.
 * All three: vocab_local, vocab_start, ld (and ldd) multiples of 8, ld (ldd) >= vocab_local, vocab_start +
 * vocab_local <= vocab_total, 16-byte aligned logits / dlogits; rows == 0 returns 0 before the pointers are read.
 * partial: one read of the shard. part: fp32 [3][rows] — part[0][i] = m_i = max_j x_ij, part[1][i] = s_i =
 *          sum_j exp(x_ij - m_i), part[2][i] = x_i[t_i - vocab_start] when the target lives on this shard, else 0.
 *          A shard row of -inf only gives m = -inf, s = 0 (no NaN). ignore_index is accepted for symmetry; the
 *          skip rule is applied by combine and grad.
 * combine: parts: fp32 [tp][3][rows], the gathered planes in rank order. M = max_r m_r, S = sum_r s_r exp(m_r - M)
 *          added in rank order (a term with m_r = -inf counts 0), lse[i] = M + log S, loss[i] = lse[i] - sum_r xt_r,
 *          and loss[i] = 0 when t == ignore_index || t < 0 || t >= vocab_total (the skip rule of
 *          pico_cross_entropy_fwd on the global vocabulary). Fixed order: every rank computes the same bits from
 *          the same planes. The caller sums loss[] and divides by the non-ignored count (pico_ce_count / _mean).
 * grad:    dlogits[i][j] = (exp(x_ij - lse[i]) - [j + vocab_start == t_i]) * (*grad_scale), row stride ldd;
 *          grad_scale is a DEVICE fp32 scalar as in pico_cross_entropy_bwd; skipped rows are written as zeros. A row
 *          whose target lives on another shard still gets its softmax term (which a shifted target passed to
 *          pico_cross_entropy_bwd would skip). dlogits may be logits itself (in place) when ldd == ld: each lane
 *          reads its 16-byte chunks before it writes them. */
int pico_ce_vp_partial(const void* logits, int64_t ld, const int64_t* target, float* part, int64_t rows,
                       int64_t vocab_local, int64_t vocab_start, int64_t vocab_total, int64_t ignore_index,
                       void* stream);
int pico_ce_vp_combine(const float* parts, int64_t tp, const int64_t* target, int64_t rows, int64_t vocab_total,
                       int64_t ignore_index, float* lse, float* loss, void* stream);
int pico_ce_vp_grad(const void* logits, int64_t ld, const int64_t* target, const float* lse, const float* grad_scale,
                    void* dlogits, int64_t ldd, int64_t rows, int64_t vocab_local, int64_t vocab_start,
                    int64_t vocab_total, int64_t ignore_index, void* stream);

/* ---- 2-D transpose ----
 * dst[c][r] = src[r][c] for a [rows, cols] bf16 matrix with row stride ld_src into [cols, rows] with row
 * stride ld_dst (elements). rows, cols, ld_src, ld_dst multiples of 8; pointers 16-byte aligned. */
int pico_transpose_bf16(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int64_t cols,
                        void* stream);

/* ---- Generation: fused RoPE + KV-cache append, split-KV decode attention (no reference call: the reference
 * has no sampling path) ----
 * Caches are bf16 views [batch, heads_kv, s_max, head_dim] with unit last stride; k_strides / v_strides are their
 * element strides {batch, head, position} (slices of a larger [layers, ...] allocation are fine). head_dim is 64 or
 * 128, heads_q a multiple of heads_kv, every stride a multiple of 8 elements, every pointer 16-byte aligned; a
 * violation returns PICO_EINVAL with a message.
 *
 * pico_kv_append: qkv is the fused q|k|v projection output, token (b, t) at qkv + b * batch_stride + t *
 *   token_stride, holding heads_q q heads, heads_kv k heads and heads_kv v heads of head_dim elements. With p =
 *   pos[b] + t (pos: DEVICE int32 [batch]): q is rotated in place with row p of the cos / sin tables ([table_rows,
 *   >= head_dim / 2] bf16, row stride cs_stride), k is rotated with row p and stored at k_cache[b, :, p, :], v is
 *   copied to v_cache[b, :, p, :]. The rotation is pico_rope's arithmetic bit for bit. A token with p outside
 *   [0, min(s_max, table_rows)) is skipped whole (no q write, no cache write). Timed under PICO_K_ROPE.
 *
 * pico_attn_decode: one query per sequence. q[b, h] at q + b * q_strides[0] + h * q_strides[1] (head_dim bf16,
 *   already rotated), seqlens DEVICE int32 [batch] -> o [batch, heads_q, head_dim] bf16 and lse [batch, heads_q]
 *   fp32 (natural log), both contiguous, of softmax(softmax_scale q K^T) V over keys [0, min(seqlens[b], s_max)).
 *   seqlens[b] <= 0 gives o = 0, lse = -inf; cache contents at or beyond the length are never read. One workgroup
 *   serves the heads_q / heads_kv (at most 8; more is refused) query heads of a kv head over a chunk of split_keys
 *   keys and writes an fp32 partial to the workspace; a second kernel combines a row's chunks in chunk order. No
 *   atomics, no inter-workgroup waiting: the same inputs and split_keys give the same bits, and a row's result does
 *   not depend on the other rows. split_keys <= 0 selects pico_attn_decode_split_keys (a host rule on the shape
 *   and the CU count, never on the device lengths). workspace: pico_attn_decode_workspace_bytes for the same
 *   arguments (-1 for bad arguments). Timed under PICO_K_ATTN_FWD (chunks) and PICO_K_ATTN_MERGE (combine). */
int pico_kv_append(void* qkv, int64_t batch_stride, int64_t token_stride, const void* cos, const void* sin,
                   int64_t cs_stride, int64_t table_rows, const int32_t* pos, void* k_cache, const int64_t* k_strides,
                   void* v_cache, const int64_t* v_strides, int64_t batch, int64_t tokens, int64_t heads_q,
                   int64_t heads_kv, int64_t s_max, int64_t head_dim, void* stream);
int64_t pico_attn_decode_split_keys(int64_t batch, int64_t heads_kv, int64_t s_max, int64_t head_dim);
int64_t pico_attn_decode_workspace_bytes(int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t s_max,
                                         int64_t head_dim, int64_t split_keys);
int pico_attn_decode(const void* q, const int64_t* q_strides, const void* k_cache, const int64_t* k_strides,
                     const void* v_cache, const int64_t* v_strides, const int32_t* seqlens, void* o, float* lse,
                     void* workspace, int64_t batch, int64_t heads_q, int64_t heads_kv, int64_t s_max,
                     int64_t head_dim, float softmax_scale, int64_t split_keys, void* stream);

/* ---- Generation: fused device sampler (no reference call: the reference has no sampling path) ----
 * pico_sample: one launch per decode step, one workgroup per row of logits [rows, vocab] (dtype PICO_SAMPLE_F32 or
 *   PICO_SAMPLE_BF16, row r at logits + r * row_stride elements, unit last stride, 1 <= vocab <= 2^20, no
 *   alignment beyond the element's). All per-step state is on the DEVICE, so a captured launch replays with the
 *   same arguments:
 *   params: 8 words {f32 temperature, f32 top_p (<= 0 or >= 1: off), i32 top_k (<= 0 or >= vocab: off), i32 eos
 *     (< 0: none), i32 pad, u32 seed low word, u32 seed high word, 0}, read at run time;
 *   draws int32 [rows]: row r reads its draw counter n = draws[r] and stores n + 1;
 *   done uint8 [rows] (may be NULL), tokens int64 [rows], out int64 [rows, out_cols] with row stride out_stride (may
 *     be NULL), kept int32 [rows] (may be NULL): the size of the set the token was drawn from.
 *   Per row, in fp32 (NaN counts as -inf, +inf as FLT_MAX): temperature <= 0 takes the maximum's lowest index (kept
 *   1). Otherwise masses exp((x - max x) / temperature); top-k keeps {x >= the k-th largest value} (ties kept);
 *   top-p then keeps {x >= t} within it for the largest t whose mass reaches top_p times the top-k set's mass (ties
 *   kept); the token is the first kept index in vocabulary order whose inclusive cumulative mass exceeds u times
 *   the kept mass, u = ((w[1] << 32) | w[0]) / 2^64 with w = Philox4x32-10(counter {r, n, 0, 0}, key {seed low,
 *   seed high}). A row with no finite logit gives token 0, kept 0. done[r] set: token = pad, kept 0. Then tokens[r]
 *   = token, out[r, n] = token if 0 <= n < out_cols, done[r] |= (token == eos) if eos >= 0, draws[r] = n + 1.
 *   Thresholds and the draw are integer arithmetic on fixed-point masses round(w 2^40): the same inputs give the
 *   same token on every run, whatever the other rows hold. rows == 0 is a no-op. Timed under PICO_K_CE_FWD. */
#define PICO_SAMPLE_F32 0
#define PICO_SAMPLE_BF16 1
int pico_sample(const void* logits, int dtype, int64_t row_stride, int64_t rows, int64_t vocab, const void* params,
                int32_t* draws, uint8_t* done, int64_t* tokens, int64_t* out, int64_t out_stride, int64_t out_cols,
                int32_t* kept, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PICOTRON_HIP_H */
