"""Vocab-parallel cross-entropy for tensor parallelism (Megatron's vocab_parallel_cross_entropy with
F.cross_entropy(reduction='mean') semantics): every tp rank keeps its [N, V/tp] column shard of the LM-head
logits and reduces only that shard; three fp32 numbers per token (the shard's row maximum, its sum of
exponentials, the target's logit) cross the wire instead of V logits, and the full [N, V] logits never
exist on any rank.

    vocab_parallel_cross_entropy(local_logits, target)          - the loss from this rank's logits
    vocab_parallel_lm_head_cross_entropy(x, w_local, target)    - LM head + loss in one autograd node

bf16 tensors on a HIP device run the gfx950 kernels (pico_ce_vp_partial / _combine / _grad, picotron_amd.ops);
anything else (CPU, fp32) runs the plain-torch restatement below: fp32 math, the same two collectives, the same
skip rule. The loss is bit-identical on every tp rank: each rank combines the same gathered planes in rank order.

apply_tensor_parallel(model, vocab_parallel_loss=True) builds the LM head for this (no gather); the caller takes
the loss from one of the two functions (train.train_step is not routed through them yet).
"""
import torch
import torch.distributed as dist

from .. import ops
from .. import process_group_manager as pgm
from .. import wgrad_operands
from .tp_communications import all_reduce_


def _tp(group):
    """(group, this rank's index in it, its size); group=None: the process group manager's tp group."""
    if group is None:
        m = pgm.process_group_manager
        if m is None:
            return None, 0, 1
        return m.tp_group, m.tp_rank, m.tp_world_size
    return group, dist.get_rank(group), dist.get_world_size(group)


def _targets(target):
    t = target.reshape(-1)
    if t.dtype != torch.int64:
        t = t.long()
    return t.contiguous()


def _gather_parts(part, group, world):
    """[3, N] fp32 planes of every rank -> [tp, 3, N], in rank order (one all-gather)."""
    if world == 1:
        return part.unsqueeze(0)
    parts = torch.empty((world,) + tuple(part.shape), dtype=part.dtype, device=part.device)
    dist.all_gather(list(parts.unbind(0)), part, group=group)
    return parts


def _on_kernels(*tensors):
    return all(t.is_cuda and t.dtype == torch.bfloat16 for t in tensors)


def _skipped(t, vocab_total, ignore_index):
    return (t == ignore_index) | (t < 0) | (t >= vocab_total)


# --------------------------------------------------------------------------------------------
# The plain-torch path: what the kernels compute, restated
# --------------------------------------------------------------------------------------------
def _torch_stats(x, t, start, vocab_total, ignore_index, group, world):
    """(lse, loss_rows) of the global vocabulary from this rank's shard x [N, V/tp] (fp32 or fp64)."""
    vl = x.shape[1]
    m = x.max(dim=1).values
    dead = m == float("-inf")  # a shard row of -inf only: s = 0, not NaN
    s = torch.where(dead, torch.zeros_like(m), torch.exp(x - torch.where(dead, torch.zeros_like(m), m)[:, None]).sum(1))
    tl = t - start
    here = (tl >= 0) & (tl < vl)
    xt = torch.where(here, x.gather(1, tl.clamp(0, vl - 1)[:, None])[:, 0], torch.zeros_like(m))
    parts = _gather_parts(torch.stack([m, s, xt]), group, world)
    M = parts[:, 0].max(dim=0).values
    S = torch.zeros_like(M)
    xts = torch.zeros_like(M)
    for r in range(world):  # rank order: the same bits on every rank
        mr, sr = parts[r, 0], parts[r, 1]
        S = S + torch.where(mr == float("-inf"), torch.zeros_like(sr), sr * torch.exp(mr - M))
        xts = xts + parts[r, 2]
    lse = M + torch.log(S)
    loss_rows = torch.where(_skipped(t, vocab_total, ignore_index), torch.zeros_like(lse), lse - xts)
    return lse, loss_rows


def _torch_grad(x, t, lse, scale, start, vocab_total, ignore_index):
    """(softmax - onehot) * scale on this rank's shard; zeros on skipped rows."""
    vl = x.shape[1]
    p = torch.exp(x - lse[:, None])
    tl = t - start
    rows = ((tl >= 0) & (tl < vl)).nonzero().flatten()
    p[rows, tl[rows]] -= 1.0
    p = p * scale
    p[_skipped(t, vocab_total, ignore_index)] = 0.0
    return p


def _math_dtype(t):
    return torch.float64 if t.dtype == torch.float64 else torch.float32


class _VocabParallelCETorchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, t, ignore_index, group):
        group, rank, world = _tp(group)
        vl = logits.shape[1]
        x = logits.to(_math_dtype(logits))
        lse, loss_rows = _torch_stats(x, t, rank * vl, world * vl, ignore_index, group, world)
        n_valid = (t != ignore_index).sum().to(x.dtype)
        ctx.save_for_backward(logits, t, lse, n_valid)
        ctx.args = (rank * vl, world * vl, int(ignore_index))
        return (loss_rows.sum() / n_valid).to(logits.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        logits, t, lse, n_valid = ctx.saved_tensors
        x = logits.to(lse.dtype)
        return _torch_grad(x, t, lse, grad_out.to(lse.dtype) / n_valid, *ctx.args).to(logits.dtype), None, None, None


class _VocabParallelLMHeadCETorchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, t, ignore_index, group):
        group, rank, world = _tp(group)
        vl = w.shape[0]
        ct = _math_dtype(x)
        x2 = x.reshape(-1, x.shape[-1]).to(ct)
        logits = x2 @ w.to(ct).t()
        lse, loss_rows = _torch_stats(logits, t, rank * vl, world * vl, ignore_index, group, world)
        n_valid = (t != ignore_index).sum().to(ct)
        dlogits = _torch_grad(logits, t, lse, 1.0 / n_valid, rank * vl, world * vl, int(ignore_index))
        ctx.save_for_backward(dlogits, x2, w)
        ctx.group, ctx.world, ctx.xshape = group, world, x.shape
        return (loss_rows.sum() / n_valid).to(x.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        dlogits, x2, w = ctx.saved_tensors
        g = grad_out.to(dlogits.dtype)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = dlogits @ w.to(dlogits.dtype)
            if ctx.world > 1:
                all_reduce_(dx, ctx.group)
            dx = (dx * g).to(w.dtype).view(ctx.xshape)
        if ctx.needs_input_grad[1]:
            dw = (dlogits.t() @ (x2 * g)).to(w.dtype)
        return dx, dw, None, None, None


# --------------------------------------------------------------------------------------------
# The gfx950 path
# --------------------------------------------------------------------------------------------
def _kernel_stats(logits, t, start, vocab_total, ignore_index, group, world):
    """partial kernel -> all-gather of the [3, N] planes -> combine kernel: (lse, loss_rows)."""
    part = ops.ce_vp_partial(logits, t, start, vocab_total, ignore_index)
    return ops.ce_vp_combine(_gather_parts(part, group, world), t, vocab_total, ignore_index)


class _VocabParallelCEFn(torch.autograd.Function):
    """One read of the shard forward (pico_ce_vp_partial), one read + one write backward (pico_ce_vp_grad),
    grad_out / n_valid read on the device: no host sync."""

    @staticmethod
    def forward(ctx, logits, t, ignore_index, group):
        group, rank, world = _tp(group)
        if logits.stride(1) != 1:
            logits = logits.contiguous()
        vl = logits.shape[1]
        lse, loss_rows = _kernel_stats(logits, t, rank * vl, world * vl, ignore_index, group, world)
        stats = ops.ce_count(t, ignore_index)
        ctx.save_for_backward(logits, t, lse, stats)
        ctx.args = (rank * vl, world * vl, int(ignore_index))
        return ops.ce_mean(loss_rows, stats, logits.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        logits, t, lse, stats = ctx.saved_tensors
        gscale = (grad_out.to(torch.float32) / stats[0]).reshape(1)
        return ops.ce_vp_grad(logits, t, lse, gscale, *ctx.args), None, None, None


class _VocabParallelLMHeadCEFn(torch.autograd.Function):
    """ops._LMHeadCEFn on a vocabulary shard: logits_local = x W_local^T into one buffer, its statistics combined
    over the tp group, then pico_ce_vp_grad turns the buffer in place into dlogits_local for a unit upstream. The
    backward runs the two LM-head GEMMs on it, sums dx over the tp group (the f region's all-reduce) and scales
    by the upstream gradient: exact for any upstream."""

    @staticmethod
    def forward(ctx, x, w, t, ignore_index, group):
        group, rank, world = _tp(group)
        x2 = x.reshape(-1, x.shape[-1])
        vl = w.shape[0]
        logits = torch.nn.functional.linear(x2, w)  # [T, V/tp] bf16, becomes dlogits in place below
        lse, loss_rows = _kernel_stats(logits, t, rank * vl, world * vl, ignore_index, group, world)
        stats = ops.ce_count(t, ignore_index)  # [n_valid, 1 / n_valid]
        ops.ce_vp_grad(logits, t, lse, stats[1:], rank * vl, world * vl, ignore_index, out=logits)
        ctx.save_for_backward(logits, wgrad_operands.saved_input(x2, vl, x), w)
        ctx.group, ctx.world, ctx.xshape = group, world, x.shape
        return ops.ce_mean(loss_rows, stats, x.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        dlogits, xin, w = ctx.saved_tensors
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = ops.dgrad(dlogits, w, (w,))
            if ctx.world > 1:
                all_reduce_(dx, ctx.group)
            dx = ops._scale_by_upstream(dx, grad_out).view(ctx.xshape)
        if ctx.needs_input_grad[1]:
            dw = ops.wgrad_accumulate((w,), dlogits, xin * grad_out.to(torch.float32))[0]
        return dx, dw, None, None, None


def vocab_parallel_cross_entropy(local_logits, target, ignore_index=-100, group=None):
    """Mean cross-entropy over the global vocabulary from this rank's logits [N, V/tp] (rank r holds the columns
    [r V/tp, (r + 1) V/tp)); target: [N] indices into the global vocabulary. F.cross_entropy(reduction='mean')
    semantics: rows whose target is ignore_index count neither in the sum nor in the mean's divisor. Returns the
    loss in the logits' dtype, bit-identical on every rank of `group` (default: the tp group). The gradient
    reaches this rank's logits only."""
    if local_logits.dim() != 2:
        local_logits = local_logits.reshape(-1, local_logits.shape[-1])
    t = _targets(target)
    fn = _VocabParallelCEFn if _on_kernels(local_logits) else _VocabParallelCETorchFn
    return fn.apply(local_logits, t, int(ignore_index), group)


def vocab_parallel_lm_head_cross_entropy(x, w_local, target, ignore_index=-100, group=None):
    """mean F.cross_entropy(x W^T, target) with W's rows (the vocabulary) split over the tp group, w_local
    [V/tp, H] this rank's rows, in one autograd node. x (the replicated hidden state, [..., H]) receives the
    gradient summed over the tp group, w_local its own rows' gradient (accumulated through
    ops.wgrad_accumulate, as the unsharded LM head's). Not chunked over tokens (the local logits are already
    1 / tp of the size), and not capturable into a HIP graph: the all-gather between its kernels and the
    all-reduce of dx run on the process group's own stream."""
    t = _targets(target)
    fn = _VocabParallelLMHeadCEFn if _on_kernels(x, w_local) else _VocabParallelLMHeadCETorchFn
    return fn.apply(x, w_local, t, int(ignore_index), group)
