"""Where the two operands of a projection's weight-gradient GEMM live: its input x (kept as x^T) and its output
gradient dy. The counterpart of grad_sink (where dW lands): the one rule every producer and consumer in ops and
model shares, on top of wgrad_pair's group buffers.

Who produces which operand of which projection (`Proj`):
  RMSNorm     y^T -> x^T of qkv, gate|up and the LM head;   dx        -> dy of out / down (it reads their output)
  attention   O^T -> x^T of out;                            dq|dk|dv  -> dy of qkv
  SwiGLU      h^T -> x^T of down;                           dgate|dup -> dy of gate|up
  LM head                                                   dlogits   -> its own dy

x^T, decided in the producer's forward (xt_sink), first matching rule wins:
  1. the producer's kernel cannot write it (`eligible`), or PICO_XT_WGRAD=0      -> None: the plain kernel
  2. pairing active, reader is a Proj, reader.K == K, T % 8 == 0                 -> the reader's group slot
  3. otherwise                                                                   -> a fresh [K, T]
The producer attaches what it wrote to its output (attach_t); the reading projection's forward picks it up
(saved_input), or transposes x itself where the K-major GEMM form pays for that (n_out >= 3 K).

dy, decided in the producer's backward; None means a fresh tensor, and neither rule ever creates group buffers:
  dy_sink_of_input   a projection's own backward (qkv, gate|up, LM head): the slot only when this micro-batch's
                     saved x^T IS the slot view, by pointer -- the forward paired it;
  dy_sink_of_output  a norm backward, whose dx is the dy of the projection before it: it holds no saved x of that
                     projection to compare by pointer, so the slot when that projection's buffers exist with this
                     shape (its forward's x^T producer created them) and writer.N == N.
wgrad_pair.plan verifies both operands by pointer per GEMM: a wrong answer here costs a copy or a GEMM per
micro-batch, never a wrong gradient.
"""
import os
from typing import Any, NamedTuple

import torch

from . import wgrad_pair as WP


class Proj(NamedTuple):
    """A projection y = x W^T, W [N, K]; `weight` (the first of row-stacked weights) keys its group buffers."""
    weight: Any
    N: int
    K: int

    @classmethod
    def of(cls, *weights):
        """Of one nn.Linear weight, or of several stacked by rows (q|k|v, gate|up)."""
        return cls(weights[0], sum(w.shape[0] for w in weights), weights[0].shape[1])


def xt_enabled():
    return os.getenv("PICO_XT_WGRAD", "1") != "0"


def xt_sink(reader, K, T, like, eligible=True):
    """Where a producer writes its [T, K] output transposed ([K, T], unit column stride) for the Proj `reader`, or
    None (rules 1-3 above). `eligible`: the producer's own kernel constraints."""
    if not eligible or not xt_enabled():
        return None
    t = None
    if reader is not None and reader[2] == K and T % 8 == 0:
        t = WP.xt_out(reader[0], reader[1], K, T, like.dtype, like.device)
    return t if t is not None else torch.empty((K, T), dtype=like.dtype, device=like.device)


def attach_t(out, xt):
    """Hand `xt`, the x^T a producer wrote beside `out` (or None), to the projection that reads `out`."""
    if xt is not None:
        out._pico_t = xt
    return out


def transposed_of(x, rows, cols):
    """The x^T attached to x, seen as [rows, cols], or None (none attached, or one of another shape)."""
    xt = getattr(x, "_pico_t", None)
    return xt if xt is not None and tuple(xt.shape) == (cols, rows) else None


def saved_input(x2, n_out, x=None):
    """What the backward keeps of a projection's input x2 [T, K] (a view of x) for its wgrad: x2 itself, or x2^T as a
    transposed view -- the producer's by-product, or a contiguous [K, T] copy where hipBLASLt's "TT" wgrad form saves
    more than the transpose costs (output width >= 3 K: qkv, gate|up, LM head; gemm_layout_probe.py --wgrad)."""
    if not xt_enabled() or not x2.is_cuda:
        return x2
    xt = transposed_of(x, *x2.shape)
    if xt is not None:
        return xt.t()
    if n_out >= 3 * x2.shape[1]:
        from . import ops  # (ops imports this module)
        return ops.transpose_2d(x2).t()
    return x2


def dy_sink_of_output(writer, T, N, like):
    """The [T, N] dy group slot of `writer`, the Proj whose output the caller differentiates, or None."""
    if writer is None or writer[1] != N:
        return None
    return WP.dy_out_existing(writer[0], N, writer[2], T, like.dtype, like.device)


def dy_sink_of_input(weight, saved_x, N, K, T, like):
    """The [T, N] dy group slot of the projection `weight` [N, K] whose backward saved `saved_x`, or None."""
    return WP.dy_out_if_paired(weight, saved_x, N, K, T, like.dtype, like.device)
