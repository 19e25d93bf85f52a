"""Document-masked causal attention (pico_attn_doc_fwd / _bwd) against plain torch in fp64 on the CPU,
with the bounds of the plain causal tests (test_kernels_gpu.py): O rel-L2 4e-3, LSE max-abs 2e-3, gradients 1e-2."""
import functools
import math

import pytest
import torch

from conftest import max_abs, rel_l2

pytestmark = pytest.mark.gpu
DEV, BF = "cuda", torch.bfloat16
CASES = {  # name: (Hq, Hkv, document lengths of each row), each the smallest shape with its hazard
    "edges": (2, 2, [[1, 63, 64, 65, 127]]),        # S 320: starts on, before and after a 64-key tile edge; odd first tile
    "rebase": (2, 1, [[300, 212]]),                 # S 512: the sweep of the last query block begins at tile 4
    "ragged": (8, 2, [[37, 190, 333, 95, 345]]),    # S 1000: partial last tile together with a start clamp, GQA 8 / 2
    "rows": (2, 2, [[448], [10, 54, 64, 100, 27, 129, 64]]),  # per-row bounds inside one launch
    "hsplit": (1, 1, [[100, 30, 126, 256, 512]]),   # S 1024, 8 key blocks x hsplit 8: lists of 5 tiles, empty shares
}
PARAMS = [(c, d) for c in ("edges", "rebase", "ragged") for d in (64, 128)] + [("rows", 64), ("hsplit", 128)]


def _reference(q, k, v, do, start, sc):  # fp64 O, dq, dk, dv [B, S, H, D] and LSE [B, H, S]
    qd, kd, vd = [t.double().cpu().transpose(1, 2).requires_grad_() for t in (q, k, v)]
    G, i = q.shape[2] // k.shape[2], torch.arange(q.shape[1])
    mask = (i[None, :] <= i[:, None])[None] & (i[None, None, :] >= start.cpu()[:, :, None].long())  # [B, Sq, Sk]
    s = ((qd @ kd.repeat_interleave(G, 1).transpose(-1, -2)) * sc).masked_fill(~mask[:, None], float("-inf"))
    o = torch.softmax(s, -1) @ vd.repeat_interleave(G, 1)
    grads = torch.autograd.grad(o, (qd, kd, vd), do.double().cpu().transpose(1, 2))
    return [t.detach().transpose(1, 2) for t in (o, *grads)] + [torch.logsumexp(s, -1).detach()]


@functools.lru_cache(maxsize=None)
def _run(case, D):
    """Inputs, the kernels' (o, lse, dq, dk, dv) and the reference of one case: computed once, never written."""
    from picotron_amd import ops
    Hq, Hkv, lengths = CASES[case]
    B, S = len(lengths), sum(lengths[0])
    g = torch.Generator("cpu").manual_seed(S + D)
    q, do, k, v = [torch.randn(B, S, h, D, generator=g).to(DEV, BF) for h in (Hq, Hq, Hkv, Hkv)]
    start = ops.doc_starts_from_lengths(lengths, S, check=True, device=DEV)
    bounds, sc = ops.doc_bounds(start), 1.0 / math.sqrt(D)
    o, lse = ops.attention_block_fwd(q, k, v, sc, True, doc_bounds=bounds)
    dq, dk, dv = ops.attention_block_bwd(do, q, k, v, o, lse, sc, True, doc_bounds=bounds)
    return (q, k, v, do, start, bounds, sc), (o, lse, dq, dk, dv), _reference(q, k, v, do, start, sc)


@pytest.mark.parametrize("case,D", PARAMS)
def test_matches_fp64_reference(case, D):
    _, (o, lse, dq, dk, dv), (O, dQ, dK, dV, L) = _run(case, D)
    errs = [rel_l2(o.cpu(), O), max_abs(lse.cpu(), L)] + [rel_l2(a.cpu(), b) for a, b in ((dq, dQ), (dk, dK), (dv, dV))]
    print(case, D, "O %.2e LSE %.2e dq %.2e dk %.2e dv %.2e" % tuple(errs))  # the figures, before the assertion
    assert errs[0] < 4e-3 and errs[1] < 2e-3 and max(errs[2:]) < 1e-2, errs


@pytest.mark.parametrize("D", [64, 128])
def test_bit_for_bit(D):
    """One document per row is the plain causal launch. No leak, with finite values (a masked p = 0 still multiplies V):
    new k / v in the document of tokens 128..192 change no other O or LSE; a dout confined to it gives zero elsewhere."""
    from picotron_amd import ops
    (q, k, v, do, start, bounds, sc), (o, lse, *_), _ = _run("edges", D)
    one = ops.attention_block_fwd(q, k, v, sc, True, doc_bounds=ops.doc_bounds(torch.zeros_like(start)))
    assert all(torch.equal(a, b) for a, b in zip(one, ops.attention_block_fwd(q, k, v, sc, True)))
    inside = start[0] == 128
    m = inside[None, :, None, None]
    o2, lse2 = ops.attention_block_fwd(q, torch.where(m, 3.0 * k + 1.0, k), torch.where(m, -2.0 * v, v), sc, True,
                                       doc_bounds=bounds)
    assert torch.equal(o2[:, ~inside], o[:, ~inside]) and torch.equal(lse2[..., ~inside], lse[..., ~inside])
    assert not torch.equal(o2[:, inside], o[:, inside])
    for g in ops.attention_block_bwd(torch.where(m, do, 0.0), q, k, v, o, lse, sc, True, doc_bounds=bounds):
        assert not bool(g[:, ~inside].any()) and bool(g[:, inside].any())


@pytest.mark.parametrize("D", [64, 128])
def test_fused_block_equals_rope_then_doc_attention(D):
    from picotron_amd import ops
    from picotron_amd.model import get_cos_sin
    B, S, nh, nkv, Hd = 2, 320, 4, 2, 256
    torch.manual_seed(D)
    bounds = ops.doc_bounds(ops.doc_starts_from_lengths([[1, 63, 64, 65, 127], [200, 120]], S, device=DEV))
    cos, sin = [t.to(DEV, BF) for t in get_cos_sin(S, D, base=10000.0)]
    x, dout, *ws = [(torch.randn(r, c, device=DEV) * std).to(BF) for r, c, std in (
        (B * S, Hd, 1.0), (B * S, nh * D, 1.0), (nh * D, Hd, Hd ** -0.5), (nkv * D, Hd, Hd ** -0.5), (nkv * D, Hd, Hd ** -0.5))]
    res = []
    for fused in (True, False):
        leaves = xx, wq, wk, wv = [t.clone().requires_grad_() for t in (x.view(B, S, Hd), *ws)]
        if fused:
            out = ops.qkv_rope_attention(xx, wq, wk, wv, cos, sin, nh, nkv, True, doc_bounds=bounds)
        else:
            q, k, v = [(xx @ w.t()).view(B, S, -1, D) for w in (wq, wk, wv)]
            q, k = [ops.apply_rotary_emb(t, cos[:, : D // 2], sin[:, : D // 2]) for t in (q, k)]
            out = ops.flash_attn_doc_func(q, k, v, bounds).reshape(B, S, nh * D)
        out.backward(dout.view(B, S, nh * D))
        res.append([out.detach()] + [t.grad for t in leaves])
    assert all(rel_l2(a, b) < tol for a, b, tol in zip(res[0], res[1], (4e-3, 1e-2, 1e-2, 1e-2, 1e-2)))


def test_model_masks_documents_in_every_layer():
    """Logits of the second document do not change with the first one's tokens; None is the call without it."""
    from picotron_amd.model import LlamaConfig, build_llama
    torch.manual_seed(0)
    model = build_llama(LlamaConfig(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_key_value_heads=1,
                                    num_hidden_layers=2, vocab_size=96, max_position_embeddings=192), device=DEV, dtype=BF)
    with torch.no_grad():
        model.final_proj.weight.normal_(std=0.05)  # build_llama leaves the head at zero
        ids = torch.randint(0, 96, (2, 192), device=DEV)
        ids2 = torch.cat(((ids[:, :70] + 1) % 96, ids[:, 70:]), 1)
        start = torch.where(torch.arange(192, device=DEV) < 70, 0, 70).to(torch.int32).expand(2, 192)
        a, b = model(ids, doc_start=start), model(ids2, doc_start=start)
        assert torch.equal(a[:, 70:], b[:, 70:]) and not torch.equal(a[:, :70], b[:, :70])
        assert torch.equal(model(ids, doc_start=None), model(ids))
