"""The gradient-sink decision (picotron_amd/grad_sink.py) and its two CPU-runnable consumers, without a device.

The DataParallelBucket half of the contract is faked with its three attributes on the parameter: `main_grad`,
`_pico_wgrad_sync() -> (syncing, W)` and `_pico_wgrad_ready()`.
"""
import pytest
import torch

from picotron_amd import grad_sink, ops

BF16 = torch.bfloat16


def _param(shape=(8, 4), dtype=BF16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.Parameter(torch.randn(*shape, generator=g).to(dtype))


def _fake_dp(p, main_grad, sync, world=4, ready=True):
    """DataParallelBucket's attributes on p; returns the list the readiness callback appends to."""
    calls = []
    p.main_grad = main_grad
    p._pico_wgrad_sync = lambda: (sync, world)
    if ready:
        p._pico_wgrad_ready = lambda: calls.append(p)
    return calls


# ---------------------------------------------------------------------------------------------------------
# resolve: one row per parameter state -> (kind, which buffer, scale)
# ---------------------------------------------------------------------------------------------------------
def _st_no_grad():
    return _param(), BF16, None


def _st_good_grad():
    p = _param()
    p.grad = torch.zeros_like(p)
    return p, BF16, None


def _st_grad_wrong_dtype():
    p = _param()
    p.grad = torch.zeros_like(p)
    p.data = p.data.float()  # the parameter moved to fp32 under its bf16 .grad
    assert p.grad.dtype != p.dtype
    return p, torch.float32, None


def _st_grad_noncontig():
    p = _param()
    p.grad = torch.zeros(4, 8, dtype=BF16).t()
    assert not p.grad.is_contiguous()
    return p, BF16, None


def _st_grad_wrong_shape():
    p = _param()
    p.grad = torch.zeros_like(p)
    p.data = torch.zeros(4, 4, dtype=BF16)
    assert p.grad.shape != p.shape
    return p, BF16, None


def _st_post_acc_hook():
    p = _param()
    p.register_post_accumulate_grad_hook(lambda q: None)
    return p, BF16, None


def _st_backward_hook():
    p = _param()
    p.register_hook(lambda g: g)
    return p, BF16, None


def _st_main_no_ready():
    p = _param()
    return p, BF16, _fake_dp(p, torch.zeros(8, 4), True, ready=False)


def _st_main_sync():
    p = _param()
    return p, BF16, _fake_dp(p, torch.zeros(8, 4), True)


def _st_main_nosync():
    p = _param()
    return p, BF16, _fake_dp(p, torch.zeros(8, 4), False)


def _st_main_bf16():
    p = _param()
    return p, BF16, _fake_dp(p, torch.zeros(8, 4, dtype=BF16), True)


def _st_main_noncontig():
    p = _param()
    return p, BF16, _fake_dp(p, torch.zeros(4, 8).t(), True)


def _st_main_wrong_shape():
    p = _param()
    return p, BF16, _fake_dp(p, torch.zeros(32), True)


def _st_dtype_mismatch():
    return _param(), torch.float32, None


def _st_dtype_mismatch_with_grad():
    p = _param()
    p.grad = torch.zeros_like(p)
    return p, torch.float32, None


def _st_none():
    return None, BF16, None


# state, fusion on?, kind, buffer ("main_grad" / "grad" / None), scale
RESOLVE_TABLE = [
    (_st_no_grad, True, "fresh", None, 1.0),
    (_st_good_grad, True, "grad", "grad", 1.0),
    (_st_grad_wrong_dtype, True, "autograd", None, 1.0),
    (_st_grad_noncontig, True, "autograd", None, 1.0),
    (_st_grad_wrong_shape, True, "autograd", None, 1.0),
    (_st_post_acc_hook, True, "autograd", None, 1.0),
    (_st_backward_hook, True, "autograd", None, 1.0),
    (_st_main_no_ready, True, "autograd", None, 1.0),
    (_st_main_sync, True, "main", "main_grad", 0.25),
    (_st_main_nosync, True, "main", "main_grad", 1.0),
    (_st_main_bf16, True, "autograd", None, 1.0),
    (_st_main_noncontig, True, "autograd", None, 1.0),
    (_st_main_wrong_shape, True, "autograd", None, 1.0),
    (_st_dtype_mismatch, True, "autograd", None, 1.0),
    (_st_dtype_mismatch_with_grad, True, "autograd", None, 1.0),
    (_st_none, True, "autograd", None, 1.0),
    (_st_no_grad, False, "autograd", None, 1.0),
    (_st_good_grad, False, "autograd", None, 1.0),
    (_st_main_sync, False, "autograd", None, 1.0),
]


@pytest.mark.parametrize("state,fusion,kind,buf,scale", RESOLVE_TABLE,
                         ids=[f"{r[0].__name__[4:]}-{'on' if r[1] else 'off'}" for r in RESOLVE_TABLE])
def test_resolve_table(monkeypatch, state, fusion, kind, buf, scale):
    monkeypatch.setenv("PICO_WGRAD_FUSION", "1" if fusion else "0")
    p, grad_dtype, calls = state()
    s = grad_sink.resolve(p, grad_dtype)
    assert s.kind == kind
    assert s.buf is (getattr(p, buf) if buf else None)
    assert s.scale == scale
    if kind == "main":
        assert s.ready is p._pico_wgrad_ready
    else:
        assert s.ready is None
    assert not calls  # resolve never fires the readiness callback
    with pytest.raises(AttributeError):  # an immutable record
        s.kind = "grad"


def test_fusion_switch_is_reexported(monkeypatch):
    assert ops.wgrad_fusion_enabled is grad_sink.wgrad_fusion_enabled
    monkeypatch.setenv("PICO_WGRAD_FUSION", "0")
    assert not ops.wgrad_fusion_enabled()
    monkeypatch.delenv("PICO_WGRAD_FUSION")
    assert ops.wgrad_fusion_enabled()


# ---------------------------------------------------------------------------------------------------------
# mark_produced
# ---------------------------------------------------------------------------------------------------------
def test_mark_produced_fires_whatever_the_sink():
    p, _, calls = _st_main_bf16()
    assert grad_sink.resolve(p, BF16).kind == "autograd"
    grad_sink.mark_produced(p)
    assert calls == [p]
    p, _, calls = _st_main_nosync()
    grad_sink.mark_produced(p)
    assert calls == [p]


def test_mark_produced_needs_main_grad():
    p = _param()
    calls = []
    p._pico_wgrad_ready = lambda: calls.append(p)  # a callback alone: not a DP-wrapped parameter
    grad_sink.mark_produced(p)
    grad_sink.mark_produced(_param())
    p2, _, calls2 = _st_main_no_ready()
    grad_sink.mark_produced(p2)
    assert calls == [] and calls2 == []


# ---------------------------------------------------------------------------------------------------------
# _norm_grad_target: the sink as the RMSNorm backward's (dw_mode, buffer, scale, ready)
# ---------------------------------------------------------------------------------------------------------
def _norm_param():
    return _param((16,))


def test_norm_target_modes_without_dp(monkeypatch):
    monkeypatch.setenv("PICO_WGRAD_FUSION", "1")
    p = _norm_param()
    mode, buf, scale, ready = ops._norm_grad_target(p, p.detach())  # no .grad yet: a fresh dw for autograd
    assert (mode, scale, ready) == (0, 1.0, None)
    assert buf.shape == p.shape and buf.dtype == p.dtype and buf is not p.grad
    p.grad = torch.zeros_like(p)
    mode, buf, scale, ready = ops._norm_grad_target(p, p.detach())
    assert (mode, scale, ready) == (1, 1.0, None) and buf is p.grad
    for bad in (lambda q: q.register_hook(lambda g: g), lambda q: q.register_post_accumulate_grad_hook(lambda r: None)):
        q = _norm_param()
        q.grad = torch.zeros_like(q)
        bad(q)
        mode, buf, scale, ready = ops._norm_grad_target(q, q.detach())
        assert (mode, scale, ready) == (0, 1.0, None) and buf is not q.grad
    mode, buf, scale, ready = ops._norm_grad_target(None, p.detach())
    assert (mode, scale, ready) == (0, 1.0, None) and buf.shape == p.shape
    monkeypatch.setenv("PICO_WGRAD_FUSION", "0")
    mode, buf, scale, ready = ops._norm_grad_target(p, p.detach())
    assert (mode, scale, ready) == (0, 1.0, None) and buf is not p.grad


def test_norm_target_noncontiguous_param(monkeypatch):
    monkeypatch.setenv("PICO_WGRAD_FUSION", "1")
    p = torch.nn.Parameter(torch.zeros(16, 2, dtype=BF16)[:, 0])
    assert not p.is_contiguous()
    w = p.detach().contiguous()
    calls = _fake_dp(p, torch.zeros(16), True)
    mode, buf, scale, ready = ops._norm_grad_target(p, w)
    assert (mode, scale, ready) == (0, 1.0, None) and buf.is_contiguous() and not calls


@pytest.mark.parametrize("chain", ["1", "0"])
def test_norm_target_modes_with_dp(monkeypatch, chain):
    monkeypatch.setenv("PICO_WGRAD_FUSION", "1")
    monkeypatch.setenv("PICO_NORM_DW_CHAIN", chain)
    p = _norm_param()
    calls = _fake_dp(p, torch.zeros(16), True)
    mode, buf, scale, ready = ops._norm_grad_target(p, p.detach())  # syncing: the callback is handed out, not called
    assert (mode, scale) == (2, 0.25) and buf is p.main_grad and ready is p._pico_wgrad_ready and not calls
    p = _norm_param()
    calls = _fake_dp(p, torch.zeros(16), False)
    mode, buf, scale, ready = ops._norm_grad_target(p, p.detach())
    assert (mode, scale) == (2, 1.0) and buf is p.main_grad
    if chain == "1":  # non-syncing and chained: recorded as produced at once, nothing left to call later
        assert ready is None and calls == [p]
    else:
        assert ready is p._pico_wgrad_ready and not calls
    for mg in (torch.zeros(16, dtype=BF16), torch.zeros(16, 2)[:, 0], torch.zeros(4, 4)):
        p = _norm_param()
        calls = _fake_dp(p, mg, False)
        mode, buf, scale, ready = ops._norm_grad_target(p, p.detach())
        assert (mode, scale, ready) == (0, 1.0, None) and buf is not mg and not calls
    p = _norm_param()
    calls = _fake_dp(p, torch.zeros(16), True, ready=False)
    assert ops._norm_grad_target(p, p.detach())[0] == 0


# ---------------------------------------------------------------------------------------------------------
# wgrad_accumulate on CPU bf16: two row-stacked [8, 4] parameters, dy [16, 16], x [16, 4]
# ---------------------------------------------------------------------------------------------------------
def _operands(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(16, 16, generator=g).to(BF16), torch.randn(16, 4, generator=g).to(BF16)


def _stacked():
    return _param(seed=1), _param(seed=2)


def test_wgrad_fresh_then_adjacent_in_place(monkeypatch):
    monkeypatch.setenv("PICO_WGRAD_FUSION", "1")
    a, b = _stacked()
    dy, x = _operands(3)
    assert ops.wgrad_accumulate((a, b), dy, x) == (None, None)
    dW = torch.mm(dy.t(), x)
    assert torch.equal(a.grad, dW[:8]) and torch.equal(b.grad, dW[8:])
    # one buffer, b's rows right behind a's
    assert a.grad.untyped_storage().data_ptr() == b.grad.untyped_storage().data_ptr()
    assert b.grad.data_ptr() == a.grad.data_ptr() + 8 * 4 * a.grad.element_size()
    ga, gb = a.grad, b.grad
    dy2, x2 = _operands(4)
    assert ops.wgrad_accumulate((a, b), dy2, x2) == (None, None)  # second micro-batch: in place, one addmm
    assert a.grad is ga and b.grad is gb
    want = dW.clone()
    torch.addmm(want, dy2.t(), x2, out=want)
    assert torch.equal(a.grad, want[:8]) and torch.equal(b.grad, want[8:])
    assert not torch.equal(want, dW)


def test_wgrad_separately_allocated_grads(monkeypatch):
    monkeypatch.setenv("PICO_WGRAD_FUSION", "1")
    a, b = _stacked()
    a.grad, b.grad = torch.zeros_like(a), torch.zeros_like(b)
    ga, gb = a.grad, b.grad
    want = [g.clone() for g in (ga, gb)]
    for seed in (3, 4):
        dy, x = _operands(seed)
        assert ops.wgrad_accumulate((a, b), dy, x) == (None, None)
        dW = torch.mm(dy.t(), x)
        want[0].add_(dW[:8])
        want[1].add_(dW[8:])
    assert a.grad is ga and b.grad is gb
    assert torch.equal(ga, want[0]) and torch.equal(gb, want[1])


def _assert_plain(a, b, dy, x):
    before = [None if p.grad is None else p.grad.clone() for p in (a, b)]
    held = [p.grad for p in (a, b)]
    out = ops.wgrad_accumulate((a, b), dy, x)
    dW = torch.mm(dy.t(), x)
    assert torch.equal(out[0], dW[:8]) and torch.equal(out[1], dW[8:])
    for p, g, g0 in zip((a, b), held, before):
        assert p.grad is g
        assert g is None or torch.equal(g, g0)


def test_wgrad_mixed_and_hooked_fall_back_to_autograd(monkeypatch):
    monkeypatch.setenv("PICO_WGRAD_FUSION", "1")
    dy, x = _operands(3)
    a, b = _stacked()  # one parameter has a gradient, the other none
    b.grad = torch.ones_like(b)
    _assert_plain(a, b, dy, x)
    a, b = _stacked()  # a backward hook on one parameter
    b.register_hook(lambda g: g)
    _assert_plain(a, b, dy, x)
    a, b = _stacked()  # a post-accumulate hook, gradients present
    a.grad, b.grad = torch.ones_like(a), torch.ones_like(b)
    a.register_post_accumulate_grad_hook(lambda q: None)
    _assert_plain(a, b, dy, x)
    a, b = _stacked()  # a non-contiguous gradient: autograd's own `grad += dW`
    a.grad, b.grad = torch.ones(4, 8, dtype=BF16).t(), torch.ones_like(b)
    _assert_plain(a, b, dy, x)
    a, b = _stacked()  # a gradient of another dtype than the parameters'
    _assert_plain(a, b, dy.float(), x.float())
    a, b = _stacked()  # one DP-wrapped parameter beside an unwrapped one
    calls = _fake_dp(a, torch.zeros(8, 4), True)
    _assert_plain(a, b, dy, x)
    assert not calls and not a.main_grad.any()
    monkeypatch.setenv("PICO_WGRAD_FUSION", "0")
    a, b = _stacked()
    _assert_plain(a, b, dy, x)
