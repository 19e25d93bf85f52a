"""attention_extend's CPU restatement, extend_step's refusals and KVCache.rewind (picotron_amd/generate.py): no GPU."""
import math

import pytest
import torch

from picotron_amd import generate as G

BF, F64 = torch.bfloat16, torch.float64


def _inputs(T, G_, D=16, Hkv=2, S=50, lens=(0, 1, 3, 17, 33, 50, 54), seed=0):
    gen = torch.Generator().manual_seed(seed + 31 * T + G_)
    B = len(lens)
    q = torch.randn(B, T, Hkv * G_, D, generator=gen).to(BF)
    k, v = (torch.randn(B, Hkv, S, D, generator=gen).to(BF) for _ in range(2))
    for b, n in enumerate(lens):
        k[b, :, min(n, S):] = math.nan
        v[b, :, min(n, S):] = math.nan
    return q, k, v, torch.tensor(lens, dtype=torch.int32)


def _direct(q, k, v, lens, scale):
    """fp64 softmax under the mask itself, no chunks: O [B, T, Hq, D], LSE [B, T, Hq]."""
    B, T, Hq, D = q.shape
    S, g = k.shape[2], Hq // k.shape[1]
    kk, vv = (torch.nan_to_num(t.double()).repeat_interleave(g, 1) for t in (k, v))
    s = torch.einsum("bthd,bhsd->bths", q.double(), kk) * scale
    lim = (lens.long()[:, None] - (T - 1 - torch.arange(T))[None]).clamp(0, S)
    s = s.masked_fill((torch.arange(S)[None, None] >= lim[:, :, None])[:, :, None], -math.inf)
    lse = torch.logsumexp(s, -1)
    p = torch.nan_to_num(torch.exp(s - lse[..., None]))  # a row with no key: 0
    return torch.einsum("bths,bhsd->bthd", p, vv), lse


@pytest.mark.parametrize("T,G_", [(1, 1), (4, 3), (16, 8)])
def test_restatement_matches_direct_softmax(T, G_):
    q, k, v, lens = _inputs(T, G_)
    O, L = _direct(q, k, v, lens, 0.25)
    o64, l64 = G.attention_extend(q.double(), k.double(), v.double(), lens, 0.25, 7, True)
    assert torch.allclose(o64, O, rtol=0, atol=1e-12) and torch.equal(torch.isinf(l64), torch.isinf(L))
    assert torch.allclose(l64[~torch.isinf(L)], L[~torch.isinf(L)], rtol=0, atol=1e-12)
    o, l = G.attention_extend(q, k, v, lens, 0.25, 7, True)
    assert o.dtype == BF and l.dtype == torch.float32 and o.shape == q.shape and l.shape == q.shape[:3]
    # per query row: one bf16 rounding of O and of p (2^-9 each, relative to the row's largest |v| <= ||v||)
    err, bound = (o.double() - O).norm(dim=-1), 2.0 ** -8 * torch.nan_to_num(v.double()).abs().amax() * math.sqrt(16)
    assert bool((err <= bound).all()), float(err.max())
    empty = torch.isinf(L)
    assert bool(empty[0].all()) and bool((o[empty] == 0).all()) and bool((l[empty] == -math.inf).all())
    assert float((l[~empty] - L[~empty]).abs().max()) < 1e-5
    for split in (None, 1, 32, 50):  # independent of split_keys to fp32 rounding
        o2, l2 = G.attention_extend(q.float(), k.float(), v.float(), lens, 0.25, split, True)
        assert torch.allclose(o2.double(), O, rtol=0, atol=2e-5) and torch.equal(torch.isinf(l2), empty)
        assert float((l2[~empty] - L[~empty]).abs().max()) < 1e-5


def test_one_token_is_attention_decode():
    q, k, v, lens = _inputs(1, 3)
    q, k, v = q.double(), k.double(), v.double()
    for split in (None, 7):
        o, l = G.attention_extend(q, k, v, lens, 0.25, split, True)
        od, ld = G.attention_decode(q[:, 0], k, v, lens, 0.25, split, True)
        assert torch.allclose(o[:, 0], od, rtol=0, atol=1e-13) and torch.allclose(l[:, 0], ld, rtol=0, atol=1e-13)


def test_refusals(monkeypatch):
    q, k, v, lens = _inputs(4, 2)
    B = q.shape[0]
    for bad_q, msg in ((q[:, :0], "tokens"), (q.repeat(1, 5, 1, 1)[:, :17], "tokens"), (q.repeat(1, 1, 5, 1)[:, :, :18],
                                                                                        "at most 8")):
        with pytest.raises(ValueError, match=msg):
            G.attention_extend(bad_q, k, v, lens)
    with pytest.raises(ValueError, match="bf16 caches only"):
        G.attention_extend(q, torch.zeros(k.shape, dtype=torch.uint8).view(torch.float8_e4m3fn),
                           torch.zeros(k.shape, dtype=torch.uint8).view(torch.float8_e4m3fn), lens)
    for bad in (lens.long(), lens[:-1], lens.to("meta")):
        with pytest.raises(ValueError, match="seqlens"):
            G.attention_extend(q, k, v, bad)
    from picotron_amd.model import Llama, LlamaConfig
    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_key_value_heads=1,
                      num_hidden_layers=1, vocab_size=64, max_position_embeddings=32)
    monkeypatch.setenv("DEVICE", "cpu")
    monkeypatch.setenv("CONTEXT_PARALLEL", "0")
    with torch.device("meta"):
        m = Llama(cfg)
    tok = torch.zeros(1, 17, dtype=torch.int64)
    with pytest.raises(ValueError, match="batch x tokens"):
        G.extend_step(m, tok.view(17, 1), G.KVCache(m, 17, 8, device="cpu"), skinny_linear=True)
    for bad in (tok, tok[:, :0]):
        with pytest.raises(ValueError, match="1 to 16"):
            G.extend_step(m, bad, G.KVCache(m, 1, 8, device="cpu"))
    with pytest.raises(ValueError, match="FP8"):
        G.extend_step(m, tok[:, :4], G.KVCache(m, 1, 8, device="cpu", kv_dtype=torch.float8_e4m3fn))
    with pytest.raises(ValueError, match="shorter"):
        G.extend_step(m, tok[:, :4], G.KVCache(m, 1, 3, device="cpu"))


def test_rewind(monkeypatch):
    from types import SimpleNamespace
    c = SimpleNamespace(lens=torch.tensor([5, 1, 0], dtype=torch.int32), batch=3)
    G.KVCache.rewind(c, 2)
    assert c.lens.tolist() == [3, 0, 0] and c.lens.dtype == torch.int32
    G.KVCache.rewind(c, torch.tensor([1, 0, 4], dtype=torch.int32))
    assert c.lens.tolist() == [2, 0, 0]
    for bad in (-1, 1.5, torch.tensor([1, 0, 4]), torch.tensor([1], dtype=torch.int32)):
        with pytest.raises(ValueError, match="rewind"):
            G.KVCache.rewind(c, bad)
