"""Where a fused weight-gradient producer puts a parameter's gradient: the one decision every producer in ops
shares (wgrad GEMMs, RMSNorm dw, embedding backward, chunked LM-head CE). Plain Python, no kernel calls.

Micro-batch accumulation happens inside the producers, into one of three places:
  * "main"  DataParallelBucket's fp32 main_grad, with the bucket's 1/W folded into the syncing micro-batch; the
            producer then calls the readiness callback;
  * "grad"  the parameter's own .grad, in place;
  * "fresh" no .grad yet: the producer's output becomes the .grad;
and "autograd" is everything else: a plain gradient handed back to autograd, which accumulates it.

The other half of the contract is DataParallelBucket (data_parallel/data_parallel.py), which installs on every
parameter `main_grad`, `_pico_wgrad_sync() -> (syncing, W)` and `_pico_wgrad_ready()`.

resolve(p, grad_dtype), first matching rule wins:
  1. p is None, or PICO_WGRAD_FUSION=0                                          -> autograd
  2. main_grad and _pico_wgrad_ready: main_grad fp32, contiguous, p's shape     -> main (scale 1/W if syncing)
                                      otherwise                                 -> autograd
  3. main_grad without a readiness callback                                     -> autograd
  4. no main_grad, no hooks on p, p.dtype == grad_dtype: .grad is None          -> fresh
                                      .grad contiguous, p's dtype and shape     -> grad
                                      any other .grad                           -> autograd
  5. anything else (hooks, a gradient of another dtype)                         -> autograd
"""
import os
from typing import Any, Callable, NamedTuple, Optional

import torch


class Sink(NamedTuple):
    kind: str                       # "main" | "grad" | "fresh" | "autograd"
    buf: Any = None                 # main: main_grad; grad: p.grad; else None
    scale: float = 1.0              # main on the syncing micro-batch: 1/W
    ready: Optional[Callable] = None  # main: p._pico_wgrad_ready, to be called once the gradient is in buf


AUTOGRAD = Sink("autograd")


def wgrad_fusion_enabled():
    """PICO_WGRAD_FUSION=0 restores the reference's two-step accumulation (for bitwise tests)."""
    return os.getenv("PICO_WGRAD_FUSION", "1") != "0"


def _has_hooks(p):
    hooks = getattr(p, "_post_accumulate_grad_hooks", None)
    return bool(hooks) or bool(getattr(p, "_backward_hooks", None))


def resolve(p, grad_dtype):
    """The Sink of parameter `p` for a gradient of dtype `grad_dtype` (rule table above). No side effects: the
    readiness callback is returned, never called."""
    if p is None or not wgrad_fusion_enabled():
        return AUTOGRAD
    mg = getattr(p, "main_grad", None)
    if mg is not None:
        ready = getattr(p, "_pico_wgrad_ready", None)
        if ready is None or mg.dtype != torch.float32 or not mg.is_contiguous() or mg.shape != p.shape:
            return AUTOGRAD
        sync, world = p._pico_wgrad_sync()
        return Sink("main", mg, 1.0 / world if sync else 1.0, ready)
    if _has_hooks(p) or p.dtype != grad_dtype:
        return AUTOGRAD
    g = p.grad
    if g is None:
        return Sink("fresh")
    if g.is_contiguous() and g.dtype == p.dtype and g.shape == p.shape:
        return Sink("grad", g)
    return AUTOGRAD


def mark_produced(p):
    """Tell DataParallelBucket that a fused producer handled `p` in this backward pass without writing a gradient
    now (a deferred micro-batch of wgrad_pair), whatever resolve() says: the bucket's post-accumulate hook would
    otherwise add a stale persistent .grad."""
    ready = getattr(p, "_pico_wgrad_ready", None)
    if ready is not None and getattr(p, "main_grad", None) is not None:
        ready()
