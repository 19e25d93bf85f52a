"""generate() through the fused device sampler, eager and as a replayed HIP graph (picotron_amd/generate.py): the
replayed iteration against the eager one bit for bit, against the default path where the two must agree, and against
the fp32 CPU oracle with the existing training forward's error as the yardstick. The tiny models are the golden
geometries tests/test_generate_gpu.py uses, built the same way."""
import dataclasses

import pytest
import torch

from conftest import max_abs, rel_l2
from oracle import model as omodel

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"
N = 12
SAMPLED = dict(temperature=0.8, top_k=20, top_p=0.9, seed=1234)
_MODELS = {}


def _tiny(golden_loss, kind):
    """'gqa2': the golden tiny geometry (4 heads / 2 kv heads, D = 64) with a 1024-row RoPE table; 'd128': the same
    with 2 heads / 1 kv head (D = 128). The gfx950 model in bf16 and the fp32 CPU oracle on its weights; the LM head
    (zero-filled by build_llama) drawn from N(0, 0.02)."""
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


def _ragged(cfg, seed):
    """Prompts of lengths 5 and 3, right-padded."""
    g = torch.Generator().manual_seed(seed)
    prompt = torch.randint(0, cfg.vocab_size, (2, 5), generator=g).to(DEV)
    prompt[1, 3:] = 0
    return prompt, [5, 3]


@pytest.mark.parametrize("settings", [dict(temperature=0.0), SAMPLED], ids=["greedy", "sampled"])
@pytest.mark.parametrize("kind", ["gqa2", "d128"])
def test_graph_equals_eager_bit_for_bit(golden_loss, kind, settings):
    from picotron_amd import generate as G
    m, _, cfg = _tiny(golden_loss, kind)
    prompt, plens = _ragged(cfg, 41)
    kw = dict(prompt_lens=plens, return_logits=True, **{"seed": 7, **settings})
    te, le = G.generate(m, prompt, N, graph=False, **kw)
    tg, lg = G.generate(m, prompt, N, graph=True, **kw)
    assert tg.shape == (2, N) and tg.dtype == torch.int64 and lg.shape == (2, N, cfg.vocab_size)
    assert torch.equal(tg, te) and torch.equal(lg, le)
    assert torch.isfinite(lg).all()
    if settings["temperature"] > 0:
        t2 = G.generate(m, prompt, N, graph=False, **{**kw, "seed": 99, "return_logits": False})
        assert not torch.equal(t2, te)  # the seed is what the tokens depend on
        assert not torch.equal(te, le.argmax(-1))


@pytest.mark.parametrize("kind", ["gqa2", "d128"])
def test_greedy_fused_equals_default_path(golden_loss, kind):
    """Where every step's logits have one maximum, the fused greedy route (eager and replayed) picks the default
    path's tokens, from the same logits."""
    from picotron_amd import generate as G
    m, _, cfg = _tiny(golden_loss, kind)
    # the logits are fp32 images of bf16 values, so two entries can share the maximum: the prompts are the first seed
    # at which no step of the default path has such a tie (the precondition, asserted on what is used)
    for seed in range(43, 59):
        prompt, plens = _ragged(cfg, seed)
        t0, l0 = G.generate(m, prompt, N, prompt_lens=plens, return_logits=True)
        if bool(((l0 == l0.max(-1, keepdim=True).values).sum(-1) == 1).all()):
            break
    assert bool(((l0 == l0.max(-1, keepdim=True).values).sum(-1) == 1).all())
    for graph in (False, True):
        t1, l1 = G.generate(m, prompt, N, prompt_lens=plens, return_logits=True, seed=5, graph=graph)
        assert torch.equal(t1, t0) and torch.equal(l1, l0), graph


@pytest.mark.parametrize("kind", ["gqa2", "d128"])
def test_default_path_is_unchanged(golden_loss, kind):
    """generate() with none of the new arguments is still the manual prefill / decode_step / sample_next loop."""
    from picotron_amd import generate as G
    m, _, cfg = _tiny(golden_loss, kind)
    prompt, plens = _ragged(cfg, 47)
    for temperature, top_k in ((0.0, None), (0.9, 10)):
        toks, logits = G.generate(m, prompt, N, prompt_lens=plens, temperature=temperature, top_k=top_k,
                                  generator=torch.Generator(DEV).manual_seed(3), return_logits=True)
        gen = torch.Generator(DEV).manual_seed(3)
        cache = G.KVCache(m, 2, 5 + N)
        lg = [G.prefill(m, prompt, cache, plens)]
        tk = [G.sample_next(lg[0], temperature, top_k, gen)]
        for _ in range(N - 1):
            lg.append(G.decode_step(m, tk[-1], cache))
            tk.append(G.sample_next(lg[-1], temperature, top_k, gen))
        assert torch.equal(torch.stack(tk, 1), toks) and torch.equal(torch.stack(lg, 1), logits)
        assert cache.graph_captures == 0 and cache._graph is None


@pytest.mark.parametrize("kind", ["gqa2", "d128"])
def test_replayed_logits_match_oracle(golden_loss, kind):
    """The logits the replayed step returns, teacher-forced by construction (each is computed from the tokens
    generated so far), against the fp32 oracle on the generated sequence, within 2x the error of the existing
    model(input_ids) logits on the same tokens: the bound of test_teacher_forced_logits_match_oracle."""
    from picotron_amd import generate as G
    m, orc, cfg = _tiny(golden_loss, kind)
    prompt, plens = _ragged(cfg, 53)
    toks, logits = G.generate(m, prompt, N, prompt_lens=plens, return_logits=True, graph=True, **SAMPLED)
    logits = logits.cpu()
    for b in range(2):
        seq = torch.cat([prompt[b:b + 1, :plens[b]], toks[b:b + 1]], 1)
        with torch.no_grad():
            want = orc(seq.cpu())
            have = m(seq).float().cpu()
        yard = (max_abs(have, want), rel_l2(have, want))
        ref = want[0, plens[b] - 1:plens[b] - 1 + N]
        e = (max_abs(logits[b], ref), rel_l2(logits[b], ref))
        print(f"{kind} row {b}: max-abs {e[0]:.3e} rel-L2 {e[1]:.3e}; model(input_ids): {yard[0]:.3e} {yard[1]:.3e}")
        assert e[0] <= 2 * yard[0] and e[1] <= 2 * yard[1], (b, e, yard)


def test_graph_is_reused_across_calls(golden_loss):
    """One capture per (model, batch): a second call on the same cache with other prompts, temperature and seed
    replays the held graph and still equals its eager run; a cache of another batch size captures its own."""
    from picotron_amd import generate as G
    m, _, cfg = _tiny(golden_loss, "gqa2")
    cache = G.KVCache(m, 2, 32)
    p1, l1 = _ragged(cfg, 59)
    a = G.generate(m, p1, N, prompt_lens=l1, cache=cache, graph=True, **SAMPLED)
    assert cache.graph_captures == 1
    assert torch.equal(a, G.generate(m, p1, N, prompt_lens=l1, **SAMPLED))
    p2, l2 = _ragged(cfg, 61)
    kw = dict(prompt_lens=l2, temperature=1.3, top_k=None, top_p=0.95, seed=77, return_logits=True)
    tg, lg = G.generate(m, p2, N + 3, cache=cache, graph=True, **kw)
    assert cache.graph_captures == 1
    te, le = G.generate(m, p2, N + 3, **kw)
    assert torch.equal(tg, te) and torch.equal(lg, le)
    assert not torch.equal(tg[:, :N], a)
    # greedy through the same graph: the settings are read from the device at replay
    tz, lz = G.generate(m, p2, N, prompt_lens=l2, cache=cache, graph=True, return_logits=True)
    t0, l0 = G.generate(m, p2, N, prompt_lens=l2, seed=0, return_logits=True)
    assert cache.graph_captures == 1 and torch.equal(tz, t0) and torch.equal(lz, l0)
    assert torch.equal(lz.max(-1).values, lz.gather(-1, tz[..., None]).squeeze(-1))  # greedy it is
    # a larger cache (batch 8, 256 positions) captures its own graph; its warm-up needs a larger decode attention
    # workspace on the capture stream, which replaces the one the first graph was captured with
    first_ws = cache._graph.workspace
    assert any(ws is first_ws for ws in G._WORKSPACES.values())
    cache8 = G.KVCache(m, 8, 256)
    p8 = torch.cat([p2, p1, p2, p1])
    t8 = G.generate(m, p8, 4, cache=cache8, graph=True, seed=1)
    assert cache8.graph_captures == 1 and cache.graph_captures == 1
    assert torch.equal(t8, G.generate(m, p8, 4, seed=1))
    assert not any(ws is first_ws for ws in G._WORKSPACES.values())  # the precondition of what follows
    assert cache8._graph.workspace.numel() > first_ws.numel()
    # the first graph holds its workspace: replayed after that, it still equals its eager run bit for bit
    ta, la = G.generate(m, p1, N, prompt_lens=l1, cache=cache, graph=True, return_logits=True, **SAMPLED)
    assert cache.graph_captures == 1 and cache._graph.workspace is first_ws
    te, le = G.generate(m, p1, N, prompt_lens=l1, return_logits=True, **SAMPLED)
    assert torch.equal(ta, a) and torch.equal(ta, te) and torch.equal(la, le)


def test_eos_pad_tail_matches_eager(golden_loss):
    """An EOS forced early, as test_generate_eos does: the graph's pad tail is the eager route's and the default
    path's."""
    from picotron_amd import generate as G
    m, _, cfg = _tiny(golden_loss, "gqa2")
    g = torch.Generator().manual_seed(29)
    prompt = torch.randint(0, cfg.vocab_size, (2, 6), generator=g).to(DEV)
    PAD = 7
    toks = G.generate(m, prompt, N)
    r0, r1 = toks[0].tolist(), toks[1].tolist()
    ks = [k for k in range(N - 1) if r0.index(r0[k]) == k and r0[k] not in r1 and r0[k] != PAD]
    assert ks, (r0, r1)
    k = ks[min(2, len(ks) - 1)]
    kw = dict(eos_token_id=r0[k], pad_token_id=PAD, return_logits=True)
    td, ld = G.generate(m, prompt, N, **kw)
    te, le = G.generate(m, prompt, N, seed=1, **kw)
    tg, lg = G.generate(m, prompt, N, seed=1, graph=True, **kw)
    assert tg[0, k + 1:].tolist() == [PAD] * (N - 1 - k) and tg[0, :k + 1].tolist() == r0[:k + 1]
    assert torch.equal(tg, te) and torch.equal(lg, le)
    assert torch.equal(tg[1], toks[1])
    # (the default path's logits agree too where its argmax was unique; the tokens are what the EOS rule fixes)
    assert torch.equal(tg, td)


def test_replay_loop_does_not_synchronise(golden_loss):
    """After the capture, a whole generate(graph=True) call, logits included, makes no synchronising call apart from
    what prefill itself does; the loop is checked on its own: replay + the logits copy."""
    from picotron_amd import generate as G
    m, _, cfg = _tiny(golden_loss, "gqa2")
    cache = G.KVCache(m, 2, 32)
    prompt, plens = _ragged(cfg, 67)
    want, wl = G.generate(m, prompt, N, prompt_lens=plens, cache=cache, graph=True, return_logits=True, **SAMPLED)
    held = cache._graph
    assert held is not None and cache.graph_captures == 1
    # the same call again, by hand, with the loop under the sync checker
    cache.reset()
    logits = G.prefill(m, prompt, cache, plens)
    held.state.reset()
    keep = torch.empty_like(wl)
    keep[:, 0] = logits
    G.sample_tokens(logits, held.state)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for step in range(1, N):
            held.graph.replay()
            keep[:, step] = held.logits
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(held.state.out[:, :N], want) and torch.equal(keep, wl)
    assert cache.lens.tolist() == [5 + N - 1, 3 + N - 1]
