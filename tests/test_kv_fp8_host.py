"""FP8 (e4m3) KV cache on the CPU: the plain-torch restatements of kv_cache_append and attention_decode for an FP8
cache, the model-level fp32 reference built on them, and what the two ops refuse."""
import math

import pytest
import torch

from oracle import hotpath as H

BF, E4 = torch.bfloat16, torch.float8_e4m3fn


def _caches(B, Hkv, S, D, fill=0x55):
    k, v = [torch.full((B, Hkv, S, D), fill, dtype=torch.uint8).view(E4) for _ in range(2)]
    ks, vs = [torch.full((B, Hkv, S), -7.0) for _ in range(2)]
    return k, v, ks, vs


@pytest.mark.parametrize("D", [64, 128])
def test_append_restatement_is_the_bf16_append_then_the_quantiser(D):
    from picotron_amd import generate as G
    from picotron_amd import ops
    B, T, Hq, Hkv, S = 3, 5, 4, 2, 16
    torch.manual_seed(D)
    qkv = torch.randn(B, T, (Hq + 2 * Hkv) * D).to(BF)
    qkv.view(B, T, -1, D)[0, 1, Hq] = 0  # an all-zero k vector: scale 1
    twin = qkv.clone()
    cos, sin = [t[:, : D // 2] for t in H.get_cos_sin(32, D, 10000.0)]
    pos = torch.tensor([0, 7, S - 2], dtype=torch.int32)  # the last row keeps 2 of its 5 tokens
    k, v, ks, vs = _caches(B, Hkv, S, D)
    kb, vb = torch.zeros(B, Hkv, S, D, dtype=BF), torch.zeros(B, Hkv, S, D, dtype=BF)
    q = G.kv_cache_append(qkv, cos, sin, pos, k, v, Hq, Hkv, k_scale=ks, v_scale=vs)
    q2 = G.kv_cache_append(twin, cos, sin, pos, kb, vb, Hq, Hkv)
    assert torch.equal(q, q2)
    x, x2 = qkv.view(B, T, -1, D), twin.view(B, T, -1, D)
    assert torch.equal(x[:, :, Hq + Hkv:], x2[:, :, Hq + Hkv:])  # v untouched
    for b, p0 in enumerate(pos.tolist()):
        n = min(T, S - p0)
        assert torch.equal(x[b, :n, Hq:Hq + Hkv], kb[b, :, p0:p0 + n].transpose(0, 1))  # k rotated in place
        assert torch.equal(x[b, n:, Hq:Hq + Hkv], x2[b, n:, Hq:Hq + Hkv])  # skipped tokens: as they were
        for codes, scales, src in ((k, ks, kb), (v, vs, vb)):
            want = ops.quantize_weight_fp8(src[b, :, p0:p0 + n].reshape(-1, D))
            assert torch.equal(codes[b, :, p0:p0 + n].reshape(-1, D).view(torch.uint8), want.codes.view(torch.uint8))
            assert torch.equal(scales[b, :, p0:p0 + n].reshape(-1), want.scale)
    assert ks[0, 0, 1] == 1.0 and (k[0, 0, 1].view(torch.uint8) == 0).all()


def test_decode_restatement_dequantises_and_drops_stale_rows():
    from picotron_amd import generate as G
    B, Hq, Hkv, S, D = 3, 4, 2, 40, 64
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, Hq, D, generator=g).to(BF)
    k, v = [torch.randint(0, 0x7F, (B, Hkv, S, D), generator=g, dtype=torch.uint8).view(E4) for _ in range(2)]
    ks, vs = [torch.rand(B, Hkv, S, generator=g) + 0.5 for _ in range(2)]
    lens = torch.tensor([0, 9, 40], dtype=torch.int32)
    want = G.attention_decode(q.double(), k.float().double() * ks.double()[..., None],
                              v.float().double() * vs.double()[..., None], lens, return_lse=True)
    for b, n in enumerate(lens.tolist()):  # NaN codes and NaN scales beyond the length
        k.view(torch.uint8)[b, :, n:] = 0x7F
        v.view(torch.uint8)[b, :, n:] = 0xFF
        ks[b, :, n:] = vs[b, :, n:] = float("nan")
    o, lse = G.attention_decode(q.double(), k, v, lens, return_lse=True, k_scale=ks, v_scale=vs)
    assert torch.equal(o, want[0]) and torch.equal(lse, want[1])
    assert (o[0] == 0).all() and (lse[0] == -math.inf).all()


def test_refusals():
    from picotron_amd import generate as G
    B, Hq, Hkv, S, D = 1, 2, 1, 8, 64
    q = torch.zeros(B, Hq, D, dtype=BF)
    qkv = torch.zeros(B, 1, (Hq + 2 * Hkv) * D, dtype=BF)
    cos, sin = [t[:, : D // 2] for t in H.get_cos_sin(16, D, 10000.0)]
    k, v, ks, vs = _caches(B, Hkv, S, D)
    kb = torch.zeros(B, Hkv, S, D, dtype=BF)
    one = torch.ones(B, dtype=torch.int32)
    bad = [dict(), dict(k_scale=ks), dict(k_scale=ks, v_scale=vs[:, :, :4]), dict(k_scale=ks, v_scale=vs.double()),
           dict(k_scale=ks, v_scale=vs.to("meta"))]
    for kw in bad:
        with pytest.raises(ValueError, match="scale"):
            G.attention_decode(q, k, v, one, **kw)
        with pytest.raises(ValueError, match="scale"):
            G.kv_cache_append(qkv, cos, sin, one, k, v, Hq, Hkv, **kw)
    with pytest.raises(ValueError, match="FP8"):  # scales with a bf16 cache
        G.attention_decode(q, kb, kb, one, k_scale=ks, v_scale=vs)
    with pytest.raises(ValueError, match="FP8"):
        G.kv_cache_append(qkv, cos, sin, one, kb, kb, Hq, Hkv, k_scale=ks, v_scale=vs)
    with pytest.raises(ValueError, match="v_cache"):  # one cache of each kind
        G.attention_decode(q, k, kb, one, k_scale=ks, v_scale=vs)


def test_reference_logits_is_the_oracle_and_moves_only_past_the_prompt(golden_loss):
    from oracle import model as omodel
    from picotron_amd import generate as G
    from picotron_amd.model import LlamaConfig
    cfg = LlamaConfig(**golden_loss["config"])
    torch.manual_seed(5)
    orc = omodel.build(cfg)
    toks = torch.randint(0, cfg.vocab_size, (12,))
    with torch.no_grad():
        orc.final_proj.weight.normal_(0.0, 0.02)
        want = orc(toks[None])[0]
    exact, quant = [G.reference_logits(orc, toks, 4, 2, p) for p in (None, 5)]
    assert float((exact - want).abs().max()) < 1e-5
    assert torch.equal(quant[:5], exact[:5]) and 0 < float((quant[5:] - exact[5:]).abs().max()) < 0.05
