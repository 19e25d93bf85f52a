"""KV-cache generation on the GPU (picotron_amd/generate.py): pico_kv_append bit for bit against pico_rope,
pico_attn_decode against the fp64 restatement on the bf16 inputs, and prefill / decode_step / generate against the
fp32 CPU oracle model, with the error of the existing training forward on the same tokens as the yardstick."""
import dataclasses
import math

import pytest
import torch

from conftest import max_abs, rel_l2
from oracle import hotpath as H
from oracle import model as omodel

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"
O_REL, LSE_ABS = 4e-3, 2e-3  # the attention forward's bounds in tests/test_kernels_gpu.py


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# --------------------------------------------------------------------------------------------
# kv_cache_append
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("D", [64, 128])
def test_kv_append_bit_identical_to_rope(D, T):
    """Rotated q (in place) and cached k equal ops.apply_rotary_emb at positions pos[b] + t bit for bit, cached v
    equals the input; the caches are layer 1 of a [3, ...] allocation. The row at S_max - 1 keeps only the tokens
    that fit: the others leave q unrotated and the cache untouched."""
    from picotron_amd import generate as G
    from picotron_amd import ops
    B, Hq, Hkv, S = 3, 4, 2, 48
    torch.manual_seed(D + T)
    qkv = torch.randn(B, T, (Hq + 2 * Hkv) * D, device=DEV).to(BF)
    src = qkv.clone().view(B, T, Hq + 2 * Hkv, D)
    cos, sin = [t.to(DEV) for t in H.get_cos_sin(64, D, 10000.0)]
    cos, sin = cos[:, : D // 2], sin[:, : D // 2]
    kall = torch.full((3, B, Hkv, S, D), -3.0, device=DEV, dtype=BF)
    vall = torch.full((3, B, Hkv, S, D), -3.0, device=DEV, dtype=BF)
    pos = [0, 5, S - 1]
    q = G.kv_cache_append(qkv, cos, sin, torch.tensor(pos, dtype=torch.int32, device=DEV), kall[1], vall[1], Hq, Hkv)
    assert q.data_ptr() == qkv.data_ptr() and q.shape == (B, T, Hq, D)
    x = qkv.view(B, T, Hq + 2 * Hkv, D)
    for b, p0 in enumerate(pos):
        n = min(T, S - p0)
        want = ops.apply_rotary_emb(src[b:b + 1, :n, : Hq + Hkv], cos[p0:p0 + n], sin[p0:p0 + n])[0]
        assert _same_bits(q[b, :n], want[:, :Hq]), (b, "q")
        assert _same_bits(kall[1, b, :, p0:p0 + n], want[:, Hq:].transpose(0, 1)), (b, "k")
        assert _same_bits(vall[1, b, :, p0:p0 + n], src[b, :n, Hq + Hkv:].transpose(0, 1)), (b, "v")
        assert _same_bits(x[b, n:], src[b, n:]), (b, "skipped tokens")
        rest = torch.ones(S, dtype=torch.bool, device=DEV)
        rest[p0:p0 + n] = False
        assert (kall[1, b][:, rest] == -3.0).all() and (vall[1, b][:, rest] == -3.0).all()
    assert _same_bits(x[:, :, Hq + Hkv:], src[:, :, Hq + Hkv:])
    assert (kall[0] == -3.0).all() and (kall[2] == -3.0).all() and (vall[0] == -3.0).all() and (vall[2] == -3.0).all()


@pytest.mark.parametrize("D", [64, 128])
def test_kv_append_never_writes_outside_the_cache(D):
    """pos = S_max - 1, T = 2, the cache a window of a larger tensor filled with a sentinel: everything outside the
    one written row keeps the sentinel."""
    from picotron_amd import generate as G
    B, Hq, Hkv, S, PAD = 2, 2, 2, 24, 8
    torch.manual_seed(7)
    qkv = (torch.rand(B, 2, (Hq + 2 * Hkv) * D, device=DEV) + 1.0).to(BF)  # no element equals the sentinel
    cos, sin = [t.to(DEV)[:, : D // 2] for t in H.get_cos_sin(64, D, 10000.0)]
    big_k = torch.full((3, B, Hkv, S + 2 * PAD, D), -9.0, device=DEV, dtype=BF)
    big_v = torch.full((3, B, Hkv, S + 2 * PAD, D), -9.0, device=DEV, dtype=BF)
    kc, vc = big_k[1][:, :, PAD:PAD + S], big_v[1][:, :, PAD:PAD + S]
    G.kv_cache_append(qkv, cos, sin, torch.full((B,), S - 1, dtype=torch.int32, device=DEV), kc, vc, Hq, Hkv)
    for big in (big_k, big_v):
        written = big != -9.0
        expect = torch.zeros_like(written)
        expect[1, :, :, PAD + S - 1] = True
        assert torch.equal(written, expect)


# --------------------------------------------------------------------------------------------
# attention_decode
# --------------------------------------------------------------------------------------------
_DECODE_CASES = {}


def _decode_case(Hq, Hkv, D, S=160, lens=(1, 31, 32, 33, 160), qscale=1.0):
    """bf16 inputs on the device and the fp64 restatement's result on them (computed once per shape)."""
    key = (Hq, Hkv, D, S, lens, qscale)
    if key not in _DECODE_CASES:
        from picotron_amd import generate as G
        B = len(lens)
        g = torch.Generator().manual_seed(Hq * 1000 + Hkv * 100 + D + S)
        q = (torch.randn(B, Hq, D, generator=g) * qscale).to(BF)
        k = torch.randn(B, Hkv, S, D, generator=g).to(BF)
        v = torch.randn(B, Hkv, S, D, generator=g).to(BF)
        lt = torch.tensor(lens, dtype=torch.int32)
        ref = G.attention_decode(q.double(), k.double(), v.double(), lt, return_lse=True)
        _DECODE_CASES[key] = (q.to(DEV), k.to(DEV), v.to(DEV), lt.to(DEV), ref)
    return _DECODE_CASES[key]


def _check_decode(o, lse, ref):
    O, L = ref
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    e_o, e_l = rel_l2(o.cpu(), O), max_abs(lse.cpu(), L)
    print(f"decode O rel-L2 {e_o:.3e} LSE max-abs {e_l:.3e}")
    assert e_o < O_REL and e_l < LSE_ABS, (e_o, e_l)
    # and per row, so that a short row cannot hide behind a long one
    for b in range(o.shape[0]):
        assert rel_l2(o[b].cpu(), O[b]) < O_REL, b


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", [(4, 4), (4, 2), (6, 2), (8, 1)])
def test_attention_decode_matches_fp64(heads, D):
    from picotron_amd import generate as G
    q, k, v, lens, ref = _decode_case(*heads, D)
    o, lse = G.attention_decode(q, k, v, lens, split_keys=32, return_lse=True)
    assert o.dtype == BF and lse.dtype == torch.float32
    _check_decode(o, lse, ref)


@pytest.mark.parametrize("heads,D", [((4, 2), 64), ((8, 1), 128)])
def test_attention_decode_default_split(heads, D):
    from picotron_amd import generate as G
    q, k, v, lens, ref = _decode_case(*heads, D, S=1024, lens=(1, 1000))
    sk = G.default_split_keys(2, heads[1], 1024, D)
    assert 256 <= sk < 1024  # more than one chunk per row
    o, lse = G.attention_decode(q, k, v, lens, return_lse=True)
    _check_decode(o, lse, ref)
    # strided q (rows of a wider projection output) and caches that are slices of a [L, ...] allocation
    wide = torch.zeros(2, heads[0] * D + 2 * heads[1] * D, device=DEV, dtype=BF)
    wide[:, : heads[0] * D] = q.reshape(2, -1)
    kv = torch.stack([torch.zeros_like(k), k, v])
    o2, lse2 = G.attention_decode(wide[:, : heads[0] * D].view(2, heads[0], D), kv[1], kv[2], lens, return_lse=True)
    assert _same_bits(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("heads,D", [((4, 2), 64), ((6, 2), 128)])
def test_attention_decode_ignores_stale_cache(heads, D):
    from picotron_amd import generate as G
    q, k, v, lens, ref = _decode_case(*heads, D)
    o, lse = G.attention_decode(q, k, v, lens, split_keys=32, return_lse=True)
    k2, v2 = k.clone(), v.clone()
    for b, n in enumerate(lens.tolist()):
        k2[b, :, n:] = float("nan")
        v2[b, :, n:] = float("nan")
    o2, lse2 = G.attention_decode(q, k2, v2, lens, split_keys=32, return_lse=True)
    assert torch.isfinite(o2).all() and torch.isfinite(lse2).all()
    assert _same_bits(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("heads,D", [((4, 2), 64), ((8, 1), 128)])
def test_attention_decode_large_scores(heads, D):
    """q scaled by 20: scores scale * q . k have standard deviation 20 and reach about +-60 over 160 keys."""
    from picotron_amd import generate as G
    q, k, v, lens, ref = _decode_case(*heads, D, qscale=20.0)
    s = torch.einsum("bhd,bsd->bhs", q.float(), k[:, 0].float()) / math.sqrt(D)
    assert float(s.abs().max()) > 45.0
    o, lse = G.attention_decode(q, k, v, lens, split_keys=32, return_lse=True)
    _check_decode(o, lse, ref)


@pytest.mark.parametrize("heads,D", [((6, 2), 64), ((4, 4), 128)])
def test_attention_decode_is_deterministic_and_row_independent(heads, D):
    from picotron_amd import generate as G
    q, k, v, lens, _ = _decode_case(*heads, D)
    o, lse = G.attention_decode(q, k, v, lens, split_keys=32, return_lse=True)
    o2, lse2 = G.attention_decode(q, k, v, lens, split_keys=32, return_lse=True)
    assert _same_bits(o, o2) and torch.equal(lse, lse2)
    for b in range(q.shape[0]):
        ob, lb = G.attention_decode(q[b:b + 1], k[b:b + 1], v[b:b + 1], lens[b:b + 1], split_keys=32, return_lse=True)
        assert _same_bits(ob, o[b:b + 1]) and torch.equal(lb, lse[b:b + 1]), b


def test_attention_decode_zero_length():
    from picotron_amd import generate as G
    q, k, v, _, _ = _decode_case(4, 2, 64)
    lens = torch.tensor([0, 0, 7, 0, 160], dtype=torch.int32, device=DEV)
    for sk in (32, None):
        o, lse = G.attention_decode(q, k, v, lens, split_keys=sk, return_lse=True)
        for b in (0, 1, 3):
            assert (o[b] == 0).all() and torch.isinf(lse[b]).all() and (lse[b] < 0).all()
        assert torch.isfinite(o).all() and torch.isfinite(lse[2]).all() and torch.isfinite(lse[4]).all()


# --------------------------------------------------------------------------------------------
# model level
# --------------------------------------------------------------------------------------------
_MODELS = {}


def _tiny(golden_loss, kind):
    """The golden tiny geometry with a 1024-row RoPE table ('gqa2': 4 heads / 2 kv heads, D = 64), or the same
    with 2 heads / 1 kv head ('d128': D = 128); the gfx950 model in bf16 and the fp32 CPU oracle on its weights.
    build_llama zero-fills the LM head, so it is drawn from N(0, 0.02) first."""
    if kind not in _MODELS:
        from picotron_amd.model import LlamaConfig, build_llama
        cfg = LlamaConfig(**{**golden_loss["config"], "max_position_embeddings": 1024})
        if kind == "d128":
            cfg = dataclasses.replace(cfg, num_attention_heads=2, num_key_value_heads=1)
        torch.manual_seed(golden_loss["seed"])
        m = build_llama(cfg, device=DEV, dtype=BF)
        with torch.no_grad():
            m.final_proj.weight.normal_(0.0, 0.02)
        orc = omodel.build(cfg)
        orc.load_state_dict({k: v.detach().float().cpu() for k, v in m.state_dict().items()}, strict=True)
        _MODELS[kind] = (m, orc, cfg)
    return _MODELS[kind]


def _oracle_and_yardstick(m, orc, seq):
    """fp32 oracle logits [B, S, V] of `seq`, and the error of the existing training forward model(seq) against
    them (max-abs, rel-L2): code this feature does not touch."""
    with torch.no_grad():
        want = orc(seq.cpu())
        have = m(seq).float().cpu()
    return want, (max_abs(have, want), rel_l2(have, want))


def _within(logits, want, yard, what):
    e = (max_abs(logits, want), rel_l2(logits, want))
    print(f"{what}: max-abs {e[0]:.3e} rel-L2 {e[1]:.3e}; model(input_ids): max-abs {yard[0]:.3e} rel-L2 {yard[1]:.3e}")
    assert e[0] <= 2 * yard[0] and e[1] <= 2 * yard[1], (what, e, yard)


@pytest.mark.parametrize("kind", ["gqa2", "d128"])
def test_teacher_forced_logits_match_oracle(golden_loss, kind):
    """Prefill (ragged prompts 5 and 3) then the true next tokens through decode_step: every step's logits against
    the oracle, within 2x the error of the existing model(input_ids) logits on the same tokens (same bf16 rounding
    points; different GEMM shapes and summation orders; each maximum over few samples)."""
    from picotron_amd import generate as G
    m, orc, cfg = _tiny(golden_loss, kind)
    g = torch.Generator().manual_seed(17)
    toks = torch.randint(0, cfg.vocab_size, (2, 48), generator=g).to(DEV)
    want, yard = _oracle_and_yardstick(m, orc, toks)
    plens = [5, 3]
    prompt = toks[:, :5].clone()
    prompt[1, 3:] = 0
    cache = G.KVCache(m, 2, 64)
    got = [G.prefill(m, prompt, cache, plens)]
    ref = [torch.stack([want[b, plens[b] - 1] for b in range(2)])]
    steps = 48 - 5
    for j in range(steps):
        nxt = torch.stack([toks[b, plens[b] + j] for b in range(2)])
        got.append(G.decode_step(m, nxt, cache))
        ref.append(torch.stack([want[b, plens[b] + j] for b in range(2)]))
    assert cache.lens.tolist() == [5 + steps, 3 + steps]
    got = torch.stack(got, 1).cpu()
    assert got.dtype == torch.float32 and got.shape == (2, steps + 1, cfg.vocab_size)
    _within(got, torch.stack(ref, 1), yard, f"{kind} prefill + decode_step")


@pytest.mark.parametrize("kind", ["gqa2", "d128"])
def test_generate_equals_manual_loop(golden_loss, kind):
    from picotron_amd import generate as G
    m, orc, cfg = _tiny(golden_loss, kind)
    g = torch.Generator().manual_seed(23)
    prompt = torch.randint(0, cfg.vocab_size, (2, 6), generator=g).to(DEV)
    N = 12
    toks, logits = G.generate(m, prompt, N, return_logits=True)
    assert toks.dtype == torch.int64 and toks.shape == (2, N) and logits.shape == (2, N, cfg.vocab_size)
    assert logits.dtype == torch.float32
    assert torch.equal(toks, logits.argmax(-1))
    toks2, logits2 = G.generate(m, prompt, N, return_logits=True)
    assert torch.equal(toks, toks2) and torch.equal(logits, logits2)
    # the same thing by hand, into a longer, reused cache
    cache = G.KVCache(m, 2, 40)
    cache.lens += 9  # generate() resets a cache it is given; the manual loop does it itself
    cache.reset()
    lg = [G.prefill(m, prompt, cache)]
    tk = [lg[0].argmax(-1)]
    for _ in range(N - 1):
        lg.append(G.decode_step(m, tk[-1], cache))
        tk.append(lg[-1].argmax(-1))
    assert torch.equal(torch.stack(tk, 1), toks) and torch.equal(torch.stack(lg, 1), logits)
    toks3 = G.generate(m, prompt, N, cache=cache)
    assert torch.equal(toks3, toks)
    # the returned logits, teacher-forced against the oracle on the sequence that was generated
    seq = torch.cat([prompt, toks], 1)
    want, yard = _oracle_and_yardstick(m, orc, seq)
    _within(logits.cpu(), want[:, 5:5 + N], yard, f"{kind} generate")


def test_generate_eos(golden_loss):
    from picotron_amd import generate as G
    m, _, cfg = _tiny(golden_loss, "gqa2")
    g = torch.Generator().manual_seed(29)
    prompt = torch.randint(0, cfg.vocab_size, (2, 6), generator=g).to(DEV)
    N, PAD = 12, 7
    toks, logits = G.generate(m, prompt, N, return_logits=True)
    r0, r1 = toks[0].tolist(), toks[1].tolist()
    # a token row 0 emits first at step k < N - 1 and row 1 never emits
    ks = [k for k in range(N - 1) if r0.index(r0[k]) == k and r0[k] not in r1 and r0[k] != PAD]
    assert ks, (r0, r1)
    k = ks[min(2, len(ks) - 1)]
    te, le = G.generate(m, prompt, N, eos_token_id=r0[k], pad_token_id=PAD, return_logits=True)
    assert te[0, :k + 1].tolist() == r0[:k + 1]
    assert te[0, k + 1:].tolist() == [PAD] * (N - 1 - k)
    assert torch.equal(te[1], toks[1]) and torch.equal(le[1], logits[1])


def test_ragged_prompts_match_single_rows(golden_loss):
    """Row b of a right-padded batch against row b generated alone with its unpadded prompt. The GEMM shapes differ
    (2 x 7 rows against 1 x 7 and 1 x 4 in prefill, 2 against 1 per step), so bit identity is not available: the
    check is on the returned logits. Each path is within acc = 2 x yardstick (max-abs) of the oracle, so two paths
    differ by at most delta = 2 acc, and they can pick different tokens only where the batch run's margin between
    the two candidates is at most 2 delta. The rows are compared step by step up to the first such near-tie (after
    it the two runs condition on different tokens)."""
    from picotron_amd import generate as G
    m, orc, cfg = _tiny(golden_loss, "gqa2")
    g = torch.Generator().manual_seed(31)
    full = torch.randint(0, cfg.vocab_size, (2, 7), generator=g).to(DEV)
    plens = [7, 4]
    prompt = full.clone()
    prompt[1, 4:] = 0
    N = 10
    toks, logits = G.generate(m, prompt, N, prompt_lens=plens, return_logits=True)
    compared = 0
    for b in range(2):
        seq = torch.cat([full[b:b + 1, :plens[b]], toks[b:b + 1]], 1)
        _, yard = _oracle_and_yardstick(m, orc, seq)
        delta = 2 * (2 * yard[0])
        t1, l1 = G.generate(m, full[b:b + 1, :plens[b]].contiguous(), N, return_logits=True)
        for j in range(N):
            d = max_abs(l1[0, j].cpu(), logits[b, j].cpu())
            assert d <= delta, (b, j, d, delta)
            compared += 1
            if int(t1[0, j]) != int(toks[b, j]):
                margin = float(logits[b, j, toks[b, j]] - logits[b, j, t1[0, j]])
                assert 0 <= margin <= 2 * delta, (b, j, margin, delta)
                break
    assert compared >= 2


def test_decode_step_does_not_synchronise(golden_loss):
    from picotron_amd import generate as G
    m, _, cfg = _tiny(golden_loss, "gqa2")
    prompt = torch.randint(0, cfg.vocab_size, (2, 4), generator=torch.Generator().manual_seed(37)).to(DEV)
    cache = G.KVCache(m, 2, 16)
    tok = G.prefill(m, prompt, cache).argmax(-1)
    tok = G.decode_step(m, tok, cache).argmax(-1)  # first call: workspace and GEMM handles exist afterwards
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        logits = G.decode_step(m, tok, cache)
        logits = G.decode_step(m, logits.argmax(-1), cache)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.isfinite(logits).all() and cache.lens.tolist() == [7, 7]


def test_refusals(golden_loss, monkeypatch):
    from types import SimpleNamespace
    from picotron_amd import generate as G
    from picotron_amd import process_group_manager as pgm
    m, _, cfg = _tiny(golden_loss, "gqa2")
    q = torch.zeros(1, 9, 64, device=DEV, dtype=BF)
    kv = torch.zeros(1, 1, 32, 64, device=DEV, dtype=BF)
    with pytest.raises(ValueError, match="at most 8"):
        G.attention_decode(q, kv, kv, torch.ones(1, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):  # no eager path on the device
        G.attention_decode(q[:, :8].float(), kv.float(), kv.float(), torch.ones(1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="RoPE table"):
        G.KVCache(m, 1, cfg.max_position_embeddings + 1)
    prompt = torch.zeros(1, 10, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="exceed"):
        G.generate(m, prompt, 7, cache=G.KVCache(m, 1, 16))
    with pytest.raises(ValueError, match="exceed"):
        G.generate(m, prompt, cfg.max_position_embeddings - 9)
    monkeypatch.setattr(pgm, "process_group_manager",
                        SimpleNamespace(tp_world_size=2, pp_world_size=1, cp_world_size=1))
    with pytest.raises(RuntimeError, match="parallel"):
        G.generate(m, prompt, 2)
