"""Host half of KV-cache generation (picotron_amd/generate.py): the plain-torch restatements of the two kernels
against the fp64 oracle, the split handling, the capacity / length guards, sample_next, the host plan of the decode
kernel (csrc/attn_decode_plan.h, swept by tests/attn_decode_plan_check.cpp) and the argument errors of the new C
entry points. CPU only."""
import ctypes
import math
import os
import subprocess

import pytest
import torch

from oracle import hotpath as H
from picotron_amd import build
from picotron_amd import generate as G

F64 = torch.float64


def _decode_inputs(B=3, Hq=6, Hkv=2, S=40, D=16, seed=0, dtype=F64):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Hq, D, generator=g, dtype=F64).to(dtype)
    k = torch.randn(B, Hkv, S, D, generator=g, dtype=F64).to(dtype)
    v = torch.randn(B, Hkv, S, D, generator=g, dtype=F64).to(dtype)
    return q, k, v


def _oracle_decode(q, k, v, lens, scale):
    outs, lses = [], []
    for b, n in enumerate(lens):
        o, lse = H.attention_fwd(q[b:b + 1, :, None], k[b:b + 1, :, :n], v[b:b + 1, :, :n], scale, False)
        outs.append(o[0, :, 0])
        lses.append(lse[0, :, 0])
    return torch.stack(outs), torch.stack(lses)


@pytest.mark.parametrize("heads", [(4, 4), (6, 2), (8, 1)])
def test_attention_decode_reference_matches_oracle(heads):
    q, k, v = _decode_inputs(Hq=heads[0], Hkv=heads[1])
    lens = [1, 17, 40]
    scale = 0.3
    o, lse = G.attention_decode(q, k, v, torch.tensor(lens, dtype=torch.int32), softmax_scale=scale, return_lse=True)
    O, L = _oracle_decode(q, k, v, lens, scale)
    assert o.dtype == F64 and o.shape == q.shape and lse.shape == q.shape[:2]
    assert float((o - O).abs().max()) < 1e-12
    assert float((lse - L).abs().max()) < 1e-12


def test_attention_decode_default_scale():
    q, k, v = _decode_inputs()
    lens = torch.tensor([3, 9, 40], dtype=torch.int32)
    a = G.attention_decode(q, k, v, lens)
    b = G.attention_decode(q, k, v, lens, softmax_scale=1.0 / math.sqrt(q.shape[-1]))
    assert torch.equal(a, b)


def test_split_handling():
    """split_keys 16, 64 and the whole cache agree; lengths 1, 15, 16, 17 with split_keys = 16 cover a chunk that is
    partly live, exactly full, and chunks that are empty (which must contribute nothing, not a NaN)."""
    q, k, v = _decode_inputs(B=5, S=70)
    lens = [1, 15, 16, 17, 70]
    lt = torch.tensor(lens, dtype=torch.int32)
    O, L = _oracle_decode(q, k, v, lens, 0.25)
    for sk in (16, 64, None):
        o, lse = G.attention_decode(q, k, v, lt, softmax_scale=0.25, split_keys=sk, return_lse=True)
        assert torch.isfinite(o).all() and torch.isfinite(lse).all()
        assert float((o - O).abs().max()) < 1e-12, sk
        assert float((lse - L).abs().max()) < 1e-12, sk


def test_zero_length_and_stale_cache():
    q, k, v = _decode_inputs(B=3, S=40)
    lens = torch.tensor([0, 5, 40], dtype=torch.int32)
    o, lse = G.attention_decode(q, k, v, lens, split_keys=16, return_lse=True)
    assert torch.equal(o[0], torch.zeros_like(o[0]))
    assert torch.isinf(lse[0]).all() and (lse[0] < 0).all()
    # contents at or beyond the length never reach the result
    k2, v2 = k.clone(), v.clone()
    for b, n in enumerate(lens.tolist()):
        k2[b, :, n:] = float("nan")
        v2[b, :, n:] = float("nan")
    o2, lse2 = G.attention_decode(q, k2, v2, lens, split_keys=16, return_lse=True)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    # a length beyond the cache is the whole cache
    o3 = G.attention_decode(q, k, v, torch.tensor([0, 5, 99], dtype=torch.int32), split_keys=16)
    assert torch.equal(o3, o)


def test_attention_decode_bf16_rounds_once():
    """Given bf16, the restatement computes in fp32 on the bf16 values and rounds O once."""
    q, k, v = _decode_inputs(dtype=torch.bfloat16)
    lens = torch.tensor([2, 20, 40], dtype=torch.int32)
    o, lse = G.attention_decode(q, k, v, lens, return_lse=True)
    o32, lse32 = G.attention_decode(q.float(), k.float(), v.float(), lens, return_lse=True)
    assert o.dtype == torch.bfloat16 and lse.dtype == torch.float32
    assert torch.equal(o, o32.to(torch.bfloat16)) and torch.equal(lse, lse32)


def test_attention_decode_refusals():
    q, k, v = _decode_inputs(Hq=9, Hkv=1)
    lens = torch.ones(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="at most 8"):
        G.attention_decode(q, k, v, lens)
    q, k, v = _decode_inputs(Hq=6, Hkv=4)
    with pytest.raises(ValueError, match="multiple"):
        G.attention_decode(q, k, v, lens)
    q, k, v = _decode_inputs()
    with pytest.raises(ValueError, match="int32"):
        G.attention_decode(q, k, v, lens.long())
    with pytest.raises(ValueError, match="split_keys"):
        G.attention_decode(q, k, v, lens, split_keys=0)


def _append_inputs(B, T, Hq, Hkv, D, S, dtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, (Hq + 2 * Hkv) * D, generator=g, dtype=F64).to(dtype)
    cos, sin = H.get_cos_sin(S + 8, D, 10000.0, dtype=dtype)
    kc = torch.full((B, Hkv, S, D), -7.0, dtype=dtype)
    vc = torch.full((B, Hkv, S, D), -7.0, dtype=dtype)
    return qkv, cos, sin, kc, vc


@pytest.mark.parametrize("dtype", [F64, torch.bfloat16])
def test_kv_cache_append_matches_oracle_rope(dtype):
    B, T, Hq, Hkv, D, S = 3, 5, 4, 2, 16, 32
    qkv, cos, sin, kc, vc = _append_inputs(B, T, Hq, Hkv, D, S, dtype)
    src = qkv.clone().view(B, T, Hq + 2 * Hkv, D)
    pos = [0, 5, S - T]
    q = G.kv_cache_append(qkv, cos[:, : D // 2], sin[:, : D // 2], torch.tensor(pos, dtype=torch.int32), kc, vc, Hq,
                          Hkv)
    assert q.shape == (B, T, Hq, D) and q.data_ptr() == qkv.data_ptr()
    for b, p0 in enumerate(pos):
        want = H.rope_fused(src[b:b + 1, :, : Hq + Hkv], cos[p0:], sin[p0:])[0]
        assert torch.equal(q[b], want[:, :Hq])
        assert torch.equal(kc[b, :, p0:p0 + T], want[:, Hq:].transpose(0, 1))
        assert torch.equal(vc[b, :, p0:p0 + T], src[b, :, Hq + Hkv:].transpose(0, 1))
        # nothing else was written
        untouched = torch.ones(S, dtype=torch.bool)
        untouched[p0:p0 + T] = False
        assert (kc[b][:, untouched] == -7.0).all() and (vc[b][:, untouched] == -7.0).all()
    # the v part of qkv is not modified
    assert torch.equal(qkv.view(B, T, Hq + 2 * Hkv, D)[:, :, Hq:][:, :, Hkv:], src[:, :, Hq + Hkv:])


def test_kv_cache_append_drops_overflow_tokens():
    """pos + T > S_max: the tokens past the cache are skipped whole (no cache write, q left unrotated); so are
    tokens whose table row does not exist."""
    B, T, Hq, Hkv, D, S = 2, 4, 2, 1, 16, 8
    qkv, cos, sin, kc, vc = _append_inputs(B, T, Hq, Hkv, D, S, F64)
    src = qkv.clone().view(B, T, Hq + 2 * Hkv, D)
    G.kv_cache_append(qkv, cos[:, : D // 2], sin[:, : D // 2], torch.tensor([S - 2, S], dtype=torch.int32), kc, vc,
                      Hq, Hkv)
    x = qkv.view(B, T, Hq + 2 * Hkv, D)
    want = H.rope_fused(src[0:1, :2, : Hq + Hkv], cos[S - 2:], sin[S - 2:])[0]
    assert torch.equal(x[0, :2, :Hq], want[:, :Hq]) and torch.equal(kc[0, :, S - 2:], want[:, Hq:].transpose(0, 1))
    assert torch.equal(x[0, 2:], src[0, 2:]) and torch.equal(x[1], src[1])
    assert (kc[0, :, : S - 2] == -7.0).all() and (kc[1] == -7.0).all() and (vc[1] == -7.0).all()
    # a short table bounds the positions the same way
    qkv2, cos, sin, kc2, vc2 = _append_inputs(B, T, Hq, Hkv, D, S, F64)
    G.kv_cache_append(qkv2, cos[:3, : D // 2], sin[:3, : D // 2], torch.tensor([1, 3], dtype=torch.int32), kc2, vc2,
                      Hq, Hkv)
    assert (kc2[0, :, 1:3] != -7.0).all() and (kc2[0, :, 3:] == -7.0).all() and (kc2[1] == -7.0).all()


def test_sample_next_greedy_and_top_k():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(64, 50, generator=g)
    am = logits.argmax(-1)
    assert torch.equal(G.sample_next(logits), am)
    assert torch.equal(G.sample_next(logits, temperature=0.7, top_k=1, generator=g), am)
    top5 = torch.topk(logits, 5, dim=-1).indices
    for _ in range(20):
        t = G.sample_next(logits, temperature=1.5, top_k=5, generator=g)
        assert (top5 == t[:, None]).any(-1).all()
    a = G.sample_next(logits, temperature=1.0, top_k=10, generator=torch.Generator().manual_seed(11))
    b = G.sample_next(logits, temperature=1.0, top_k=10, generator=torch.Generator().manual_seed(11))
    assert a.dtype == torch.int64 and a.shape == (64,) and torch.equal(a, b)
    with pytest.raises(ValueError):
        G.sample_next(logits, temperature=-1.0)
    with pytest.raises(ValueError):
        G.sample_next(logits, temperature=1.0, top_k=0)


@pytest.mark.parametrize("top_k", [None, 8, 5])
def test_sample_next_frequencies(top_k):
    """4096 identical rows of an 8-way distribution: every empirical frequency lies within 5 binomial standard
    deviations, 5 sqrt(p (1 - p) / 4096), of its softmax probability (a derived bound: a 5-sigma miss of one of 8
    cells has probability < 5e-6)."""
    n, temp = 4096, 0.8
    row = torch.tensor([0.3, -1.2, 2.0, 0.0, 1.1, -0.4, 0.9, -2.5])
    x = row / temp
    if top_k is not None and top_k < 8:
        kept = torch.topk(x, top_k).indices
        masked = torch.full_like(x, float("-inf"))
        masked[kept] = x[kept]
        x = masked
    p = torch.softmax(x.double(), -1)
    draws = G.sample_next(row.expand(n, 8).contiguous(), temperature=temp, top_k=top_k,
                          generator=torch.Generator().manual_seed(5))
    freq = torch.bincount(draws, minlength=8).double() / n
    bound = 5.0 * torch.sqrt(p * (1 - p) / n)
    assert (freq - p).abs().le(bound).all(), (freq, p, bound)


def test_decode_plan_sweep(tmp_path):
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_decode_plan_check.cpp")
    exe = str(tmp_path / "attn_decode_plan_check")
    # host only: the plan header must compile without the HIP headers
    subprocess.run([build.HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-nogpuinc", "-nogpulib",
                    "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout


@pytest.fixture(scope="module")
def lib():
    from picotron_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def _decode_call(lib, q=64, k=64, v=64, lens=64, o=64, lse=64, ws=64, B=2, Hq=4, Hkv=2, S=128, D=64, qs=(256, 64),
                 ks=(16384, 8192, 64), vs=(16384, 8192, 64)):
    from picotron_amd import _lib
    vp = ctypes.c_void_p
    return lib.pico_attn_decode(vp(q), (_lib.c_i64 * 2)(*qs), vp(k), _lib.i64x3(ks), vp(v), _lib.i64x3(vs), vp(lens),
                                vp(o), vp(lse), vp(ws), B, Hq, Hkv, S, D, 0.125, 0, None)


def _append_call(lib, qkv=64, cos=64, sin=64, pos=64, k=64, v=64, B=2, T=1, Hq=4, Hkv=2, S=128, D=64, bs=512, ts=512,
                 ks=(16384, 8192, 64), vs=(16384, 8192, 64)):
    from picotron_amd import _lib
    vp = ctypes.c_void_p
    return lib.pico_kv_append(vp(qkv), bs, ts, vp(cos), vp(sin), 32, 128, vp(pos), vp(k), _lib.i64x3(ks), vp(v),
                              _lib.i64x3(vs), B, T, Hq, Hkv, S, D, None)


def test_abi_argument_errors(lib):
    """Each argument error returns PICO_EINVAL (1000) with its message; no kernel is launched (the pointers are
    never dereferenced)."""
    err = lib.pico_last_error
    assert _decode_call(lib, q=None) == 1000 and b"null" in err()
    assert _decode_call(lib, lens=None) == 1000 and b"null" in err()
    assert _decode_call(lib, ws=None) == 1000 and b"null" in err()
    assert _decode_call(lib, D=96) == 1000 and b"head_dim" in err()
    assert _decode_call(lib, Hq=5) == 1000 and b"multiple of heads_kv" in err()
    assert _decode_call(lib, Hq=18) == 1000 and b"at most 8" in err()
    assert _decode_call(lib, ks=(16384, 8192, 68)) == 1000 and b"multiples of 8" in err()
    assert _decode_call(lib, vs=(16380, 8192, 64)) == 1000 and b"multiples of 8" in err()
    assert _decode_call(lib, qs=(252, 64)) == 1000 and b"multiples of 8" in err()
    assert lib.pico_attn_decode_workspace_bytes(2, 18, 2, 128, 64, 0) == -1 and b"at most 8" in err()
    assert lib.pico_attn_decode_workspace_bytes(2, 4, 2, 128, 96, 0) == -1 and b"head_dim" in err()
    assert _append_call(lib, qkv=None) == 1000 and b"null" in err()
    assert _append_call(lib, pos=None) == 1000 and b"null" in err()
    assert _append_call(lib, D=96) == 1000 and b"head_dim" in err()
    assert _append_call(lib, Hq=5) == 1000 and b"multiple of heads_kv" in err()
    assert _append_call(lib, ks=(16384, 8190, 64)) == 1000 and b"multiples of 8" in err()
    assert _append_call(lib, ts=516) == 1000 and b"multiples of 8" in err()


def test_workspace_follows_the_plan(lib):
    """m | l | o for B * Hq * nsplit partials, each region padded to 256 bytes; the default split is the host rule
    for the device's CU count (256 without a device) and never depends on lengths."""
    sk = lib.pico_attn_decode_split_keys(1, 32, 8192, 64)
    assert sk >= 256 and sk % 128 == 0 and 32 * -(-8192 // sk) >= 2 * 256
    assert lib.pico_attn_decode_split_keys(32, 32, 1024, 64) == 1024  # 1024 workgroups already: no split
    assert lib.pico_attn_decode_split_keys(1, 1, 512, 128) == 256  # never below the minimum chunk
    n = -(-160 // 32)
    parts = 5 * 6 * n
    pad = lambda x: -(-x // 256) * 256  # noqa: E731
    assert lib.pico_attn_decode_workspace_bytes(5, 6, 2, 160, 128, 32) == 2 * pad(parts * 4) + pad(parts * 128 * 4)


def test_model_refusals_host(monkeypatch):
    from types import SimpleNamespace
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.model import Llama, LlamaConfig
    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_key_value_heads=1,
                      num_hidden_layers=1, vocab_size=64, max_position_embeddings=32)
    monkeypatch.setenv("DEVICE", "cpu")
    monkeypatch.setenv("CONTEXT_PARALLEL", "0")  # another test of the process may have left it at 1
    with torch.device("meta"):
        m = Llama(cfg)
    with pytest.raises(ValueError, match="RoPE table"):
        G.KVCache(m, 1, 33, device="cpu")
    c = G.KVCache(m, 2, 16, device="cpu")
    assert c.k.shape == (1, 2, 1, 16, 64) and c.k.dtype == torch.bfloat16 and c.lens.dtype == torch.int32
    c.lens += 3
    c.reset()
    assert int(c.lens.sum()) == 0
    ids = torch.zeros(2, 10, dtype=torch.int64)
    with pytest.raises(ValueError, match="exceed"):
        G.generate(m, ids, 7, cache=c)
    with pytest.raises(ValueError, match="exceed"):
        G.generate(m, ids, 23)
    with pytest.raises(TypeError, match="plain"):
        G.generate(torch.nn.Sequential(m), ids, 2)
    monkeypatch.setattr(pgm, "process_group_manager",
                        SimpleNamespace(tp_world_size=2, pp_world_size=1, cp_world_size=1))
    with pytest.raises(RuntimeError, match="parallel"):
        G.generate(m, ids, 2)
