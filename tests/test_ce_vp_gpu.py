"""The vocab-parallel cross-entropy kernels (pico_ce_vp_partial / _combine / _grad) in one process: the tp shards
are column slices of one [rows, V] bf16 tensor (row stride V > vocab_local, in-place writes into slices), the
all-gather is a torch.stack of the shards' planes. Against fp64 on the same bf16 logits.

The bound on lse (and on the per-row loss): with e_ref the max abs error of the existing full-vocabulary kernel
(pico_cross_entropy_fwd) against the same fp64 values on the same logits, measured in the same test, the
vocab-parallel error of a row must be <= 2 e_ref + 4 fp32 ulps of |lse|: the margin covers the tp - 1 extra
exp / multiply-add roundings of the combine and a different summation order; nothing else differs."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROWS = 300


def _ulp32(x):
    """Spacing of fp32 at |x| (x: fp64 tensor)."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


def _full_fwd(logits, tgt):
    """(lse, loss_rows) of the existing full-vocabulary kernel."""
    from picotron_amd import _lib
    rows, V = logits.shape
    lse = torch.empty(rows, dtype=torch.float32, device=DEV)
    loss = torch.empty(rows, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().pico_cross_entropy_fwd(_lib.ptr(logits), logits.stride(0), _lib.ptr(tgt), _lib.ptr(lse),
                                                  _lib.ptr(loss), rows, V, -100, _lib.stream_of(logits)),
               "pico_cross_entropy_fwd")
    return lse, loss


def _vp_forward(logits, tgt, tp):
    from picotron_amd import ops
    V = logits.shape[1]
    vl = V // tp
    parts = torch.stack([ops.ce_vp_partial(logits[:, r * vl:(r + 1) * vl], tgt, r * vl, V) for r in range(tp)])
    lse, loss = ops.ce_vp_combine(parts, tgt, V)
    return parts, lse, loss


def _vp_grad_in_place(logits, tgt, lse, gscale, tp):
    """Every shard's dlogits written in place into its slice of a clone: the concatenated [rows, V] gradient."""
    from picotron_amd import ops
    V = logits.shape[1]
    vl = V // tp
    buf = logits.clone()
    for r in range(tp):
        sl = buf[:, r * vl:(r + 1) * vl]
        out = ops.ce_vp_grad(sl, tgt, lse, gscale, r * vl, V, out=sl)
        assert out.data_ptr() == sl.data_ptr()
    return buf


def _targets(V, tp, ignore, gen):
    vl = V // tp
    tgt = torch.randint(0, V, (ROWS,), generator=gen)
    if ignore:
        tgt[::7] = -100
    for r in range(tp):  # the first and the last index of every shard
        tgt[10 + 2 * r], tgt[11 + 2 * r] = r * vl, (r + 1) * vl - 1
    tgt[5] = V + 3  # out of range: skipped like an ignored row
    return tgt.to(DEV)


@pytest.mark.parametrize("V,tp,ignore", [(64, 8, False), (4000, 4, True), (32000, 4, False), (49152, 2, True),
                                         (512, 1, True)])
def test_vocab_parallel_kernels_match_fp64(V, tp, ignore):
    gen = torch.Generator().manual_seed(V + tp)
    logits = (torch.randn(ROWS, V, generator=gen) * 3).to(BF).to(DEV)
    tgt = _targets(V, tp, ignore, gen)
    vl = V // tp
    skip = (tgt == -100) | (tgt < 0) | (tgt >= V)
    assert bool(skip[5]) and (int(skip.sum()) > 30) == ignore
    x = logits.double()
    lse64 = torch.logsumexp(x, dim=1)
    loss64 = torch.where(skip, torch.zeros_like(lse64), lse64 - x.gather(1, tgt.clamp(0, V - 1)[:, None])[:, 0])

    lse_ref, loss_ref = _full_fwd(logits, tgt)
    e_ref = float((lse_ref.double() - lse64).abs().max())
    parts, lse, loss = _vp_forward(logits, tgt, tp)
    err = (lse.double() - lse64).abs()
    bound = 2 * e_ref + 4 * _ulp32(lse64)
    print(f"V={V} tp={tp}: e_ref={e_ref:.3e} vocab-parallel max err={float(err.max()):.3e} "
          f"(min bound {float(bound.min()):.3e})")
    assert bool((err <= bound).all()), (float(err.max()), e_ref)
    assert bool((loss[skip] == 0).all()) and bool((loss_ref[skip] == 0).all())
    lerr = (loss.double() - loss64).abs()
    assert bool((lerr <= bound).all()), (float(lerr.max()), e_ref)

    # dlogits: in place into the slices of a clone, against fp64 (softmax - onehot) * scale
    n_valid = int((~skip).sum())
    gscale = torch.tensor([0.25 / n_valid], dtype=torch.float32, device=DEV)
    dl = _vp_grad_in_place(logits, tgt, lse, gscale, tp)
    p = torch.softmax(x, dim=1)
    keep_rows = (~skip).nonzero().flatten()
    p[keep_rows, tgt[keep_rows]] -= 1
    p[skip] = 0
    p *= 0.25 / n_valid
    assert rel_l2(dl.cpu(), p.cpu()) < 8e-3
    assert float(dl[skip].float().abs().sum()) == 0.0 and not bool(torch.signbit(dl[skip].float()).any())
    # out of place into a fresh buffer (ldd = vocab_local): the same bits
    from picotron_amd import ops
    for r in range(tp):
        fresh = ops.ce_vp_grad(logits[:, r * vl:(r + 1) * vl], tgt, lse, gscale, r * vl, V)
        assert fresh.stride(0) == vl and torch.equal(fresh, dl[:, r * vl:(r + 1) * vl])

    # determinism
    parts2, lse2, loss2 = _vp_forward(logits, tgt, tp)
    assert torch.equal(parts2, parts) and torch.equal(lse2, lse) and torch.equal(loss2, loss)
    assert torch.equal(_vp_grad_in_place(logits, tgt, lse2, gscale, tp), dl)


def test_vocab_parallel_edge_rows():
    """A shard row of -inf only (m = -inf, s = 0: no NaN, lse = the other shard's own) and a shard 200 below the
    other (exp(m_r - M) underflows to 0)."""
    from picotron_amd import ops
    V, tp, vl = 64, 2, 32
    gen = torch.Generator().manual_seed(11)
    xf = torch.randn(4, V, generator=gen) * 3
    xf[1, :vl] = float("-inf")
    xf[2, :vl] = xf[2, vl:] - 200
    logits = xf.to(BF).to(DEV)
    tgt = torch.tensor([3, 40, 5, 63], device=DEV)  # row 1: on the live shard; row 2: on the underflowing shard
    x = logits.double()
    lse64 = torch.logsumexp(x, dim=1)
    loss64 = lse64 - x.gather(1, tgt[:, None])[:, 0]
    lse_ref, _ = _full_fwd(logits, tgt)
    e_ref = float((lse_ref.double() - lse64).abs().max())
    parts, lse, loss = _vp_forward(logits, tgt, tp)
    assert float(parts[0, 0, 1]) == float("-inf") and float(parts[0, 1, 1]) == 0.0 and float(parts[0, 2, 1]) == 0.0
    assert not bool(torch.isnan(parts).any())
    assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(loss).all())
    bound = 2 * e_ref + 4 * _ulp32(lse64)
    assert bool(((lse.double() - lse64).abs() <= bound).all())
    # loss = lse - x[t] is rounded once more, at |loss| (row 2: ~200, far above |lse|): half an ulp of it on top
    assert bool(((loss.double() - loss64).abs() <= bound + 0.5 * _ulp32(loss64)).all())
    # row 1: exactly what shard 1 alone gives (S = 0 + s_1 exp(0)), and shard 1's own logsumexp
    alone, _ = ops.ce_vp_combine(parts[1:2].contiguous(), tgt, V)
    assert float(lse[1]) == float(alone[1])
    assert abs(float(lse[1]) - float(torch.logsumexp(x[1, vl:], dim=0))) <= float(bound[1])
    gscale = torch.tensor([0.25], dtype=torch.float32, device=DEV)
    dl = _vp_grad_in_place(logits, tgt, lse, gscale, tp)
    assert not bool(torch.isnan(dl).any())
    assert float(dl[1, :vl].float().abs().sum()) == 0.0
    p = torch.softmax(x, dim=1)
    p[torch.arange(4, device=DEV), tgt] -= 1
    assert rel_l2(dl.cpu(), (p * 0.25).cpu()) < 8e-3


def test_vocab_parallel_autograd_single_shard():
    """The autograd nodes with a group of one (no collective): vocab_parallel_lm_head_cross_entropy against fp64 —
    loss, dx and dW accumulated onto an existing .grad, for a non-unit upstream — with
    test_lm_head_cross_entropy_fused's tolerances, and vocab_parallel_cross_entropy on the same logits."""
    from picotron_amd import ops
    from picotron_amd.tensor_parallel import vocab_parallel_loss as VPL
    torch.manual_seed(4000)
    T, H, V, g = 512, 256, 4000, 0.25
    x = (torch.randn(T, H, device=DEV) * 0.5).to(BF).requires_grad_(True)
    w = (torch.randn(V, H, device=DEV) * 0.05).to(BF).requires_grad_(True)
    w0 = (torch.randn(V, H, device=DEV) * 1e-5).to(BF)  # same scale as dW: accumulation visible in bf16
    w.grad = w0.clone()
    tgt = torch.randint(0, V, (T,), device=DEV)
    tgt[::5] = -100
    loss = VPL.vocab_parallel_lm_head_cross_entropy(x, w, tgt)
    (loss * g).backward()
    xd, wd = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(xd @ wd.t(), tgt)
    (ref * g).backward()
    assert loss.dtype == BF
    assert abs(float(loss.detach()) - float(ref.detach())) <= 8e-3 * abs(float(ref.detach())) + 1e-3
    assert rel_l2(x.grad.cpu(), xd.grad.cpu()) < 1.5e-2
    assert rel_l2((w.grad.double() - w0.double()).cpu(), wd.grad.cpu()) < 3e-2
    # the loss alone on the same logits, a negative upstream
    lg = ops.linear(x.detach(), w.detach()).requires_grad_(True)
    l2 = VPL.vocab_parallel_cross_entropy(lg, tgt)
    (l2 * -g).backward()
    ld = lg.detach().double().requires_grad_(True)
    ref2 = torch.nn.functional.cross_entropy(ld, tgt)
    (ref2 * -g).backward()
    assert l2.dtype == BF and abs(float(l2.detach()) - float(ref2.detach())) <= 8e-3 * abs(float(ref2.detach())) + 1e-3
    assert rel_l2(lg.grad.cpu(), ld.grad.cpu()) < 8e-3
