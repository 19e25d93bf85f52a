"""The fused sampler's contract on the host: the CPU path of picotron_amd.generate.sample_tokens (plain torch, fp64
masses) against the fp64 loop reference and the acceptance rule of tests/sample_ref.py, the state rules (draws, done,
out, pad), SamplerState.set, and pico_sample's argument errors. The checks are functions of a sampler callable, so
that three wrong samplers (descending-probability cumulation, ties dropped at k, counter n + 1) can be shown to fail
them. tests/test_sample_gpu.py holds the kernel to the same reference."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sample_ref as R

SEED = 0x1234_5678_9ABC_DEF0
NINF, NAN = float("-inf"), float("nan")


# --------------------------------------------------------------------------------------------
# samplers: (logits [B, V] fp32 tensor, settings dict, draws list) -> (tokens list, kept list)
# --------------------------------------------------------------------------------------------
def cpu_path(logits, settings, draws):
    from picotron_amd import generate as G
    st = G.SamplerState(logits.shape[0], "cpu", seed=SEED, **settings)
    st.draws.copy_(torch.tensor(draws, dtype=torch.int32))
    tok, kept = G.sample_tokens(logits, st, return_kept=True)
    assert st.draws.tolist() == [n + 1 for n in draws]
    return tok.tolist(), kept.tolist()


def loop_sampler(order="vocab", ties=True, shift=0):
    """A sampler written against the reference's own pieces; the defaults are the contract, each flag one mutant."""

    def run(logits, settings, draws):
        T, k, p = settings.get("temperature", 0.0), settings.get("top_k"), settings.get("top_p")
        rs = R.draw_words(SEED, range(logits.shape[0]), [n + shift for n in draws])
        toks, kepts, shared = [], [], None
        for b in range(logits.shape[0]):
            if shared is None or logits.stride(0) != 0:  # expanded copies of one row share its reference
                x = logits[b].numpy()
                row = R.Row(x, T, k, p)
                keep = row.keep.copy()
                if not ties and T > 0 and k is not None and 0 < k < len(keep) and p is None:
                    keep[:] = False
                    keep[np.argsort(-R.canon(x), kind="stable")[:k]] = True
                w = np.where(keep, row.w, 0.0)
                idx = np.arange(len(w)) if order == "vocab" else np.argsort(-w, kind="stable")
                shared = (row, idx, np.cumsum(w[idx]), int(keep.sum()))
            row, idx, c, size = shared
            if not row.live:
                toks.append(0)
                kepts.append(0)
                continue
            j = int(np.searchsorted(c, rs[b] / 2.0 ** 64 * c[-1], side="right"))
            toks.append(int(idx[min(j, len(idx) - 1)]))
            kepts.append(size)
        return toks, kepts

    return run


# --------------------------------------------------------------------------------------------
# the checks
# --------------------------------------------------------------------------------------------
HAND_ROWS = [
    # name, row, settings, the kept set
    ("ties at k", [3.0, 1.0, 2.0, 2.0, 2.0, 0.0, -1.0], dict(temperature=1.0, top_k=2), {0, 2, 3, 4}),
    ("ties at the cut", [2.0, 1.0, 1.0, 1.0, -3.0, -3.0], dict(temperature=1.0, top_p=0.6), {0, 1, 2, 3}),
    ("dominant", [10.0, 0.0, 0.0, 0.0, 0.0], dict(temperature=1.0, top_p=0.9), {0}),
    ("bans, no filter", [1.0, NINF, NAN, 0.5], dict(temperature=1.0), {0, 1, 2, 3}),
    ("bans, k = 2", [1.0, NINF, NAN, 0.5], dict(temperature=1.0, top_k=2), {0, 3}),
    ("bans, k = 3", [1.0, NINF, NAN, 0.5], dict(temperature=1.0, top_k=3), {0, 1, 2, 3}),
    ("k = 1", [0.5, 2.0, 1.5, 2.0], dict(temperature=1.0, top_k=1), {1, 3}),
    ("k = 1, no tie", [0.5, 2.0, 1.5, 1.0], dict(temperature=2.0, top_k=1), {1}),
    ("k >= V", [0.5, 2.0, 1.5, 1.0], dict(temperature=1.0, top_k=4), {0, 1, 2, 3}),
    ("p >= 1", [0.5, 2.0, 1.5, 1.0], dict(temperature=1.0, top_p=1.0), {0, 1, 2, 3}),
    ("k and p", [4.0, 3.5, 3.5, 1.0, 0.0, 3.0], dict(temperature=1.0, top_k=4, top_p=0.5), {0, 1, 2}),
]
COPIES = 512  # rows per hand-built case: same logits, their own draws


def check_hand_rows(sampler):
    """Exact kept sets: the reference agrees with the set written down; the sampler's `kept` is its size, every token
    lies in it and is accepted, and over 512 draws every member with mass shows up."""
    for name, row, settings, want in HAND_ROWS:
        x = torch.tensor(row, dtype=torch.float32)
        ref = R.Row(x.numpy(), settings["temperature"], settings.get("top_k"), settings.get("top_p"))
        assert set(np.flatnonzero(ref.keep).tolist()) == want, name
        assert ref.margin > R.tau(len(row)), name
        toks, kept = sampler(x.expand(COPIES, -1), settings, [0] * COPIES)
        assert set(kept) == {len(want)}, (name, set(kept))
        rs = R.draw_words(SEED, range(COPIES), [0] * COPIES)
        assert all(ref.accepts(t, r, R.tau(len(row))) for t, r in zip(toks, rs)), name
        assert set(toks) == {i for i in want if ref.w[i] > 0}, (name, set(toks))


def check_dead_row(sampler):
    x = torch.tensor([[NINF] * 5, [NAN, NINF, NAN, NINF, NINF], [0.0, 1.0, NINF, NAN, 0.5]])
    for settings in (dict(temperature=0.0), dict(temperature=1.0), dict(temperature=0.7, top_k=2, top_p=0.9)):
        toks, kept = sampler(x, settings, [0, 0, 0])
        assert toks[:2] == [0, 0] and kept[:2] == [0, 0], (settings, toks, kept)
        assert toks[2] in (0, 1, 4) and kept[2] >= 1


def check_greedy(sampler):
    x = torch.tensor([[1.0, 5.0, 5.0, 2.0], [7.0, 7.0, 7.0, 7.0], [-1.0, -2.0, -0.5, -0.5], [0.0, -0.0, -1.0, 0.0],
                      [NAN, 3.0, NINF, 3.0]])
    toks, kept = sampler(x, dict(temperature=0.0, top_k=2, top_p=0.5), [3] * 5)
    assert toks == [1, 0, 2, 0, 1] and kept == [1] * 5


def _vector(V, settings):
    """One logit vector (randn * 4) whose top-p cut clears tau(V) under `settings`: the first seed that does."""
    for seed in range(64):
        x = (torch.randn(V, generator=torch.Generator().manual_seed(1000 * V + seed)) * 4).float()
        ref = R.Row(x.numpy(), settings["temperature"], settings.get("top_k"), settings.get("top_p"))
        if ref.margin > R.tau(V):
            return x, ref
    raise AssertionError("no seed gives the cut a margin")


DRAW_SETTINGS = [dict(temperature=0.8), dict(temperature=1.0, top_k=5), dict(temperature=0.7, top_p=0.9),
                 dict(temperature=1.3, top_k=50, top_p=0.9)]
ROWS = 4096


def check_draws(sampler, counter=0):
    """4096 rows of one logit vector, each with its own draw: every token is accepted. Consecutive kept tokens'
    intervals share an end point only, so a token one position off in the cumulative order fails."""
    for V in (7, 257, 1000):
        for settings in DRAW_SETTINGS:
            x, ref = _vector(V, settings)
            assert ref.margin > R.tau(V)
            toks, kept = sampler(x.expand(ROWS, -1), settings, [counter] * ROWS)
            rs = R.draw_words(SEED, range(ROWS), [counter] * ROWS)
            bad = [b for b in range(ROWS) if not ref.accepts(toks[b], rs[b], R.tau(V))]
            assert not bad, (V, settings, len(bad), bad[:4])
            assert set(kept) == {ref.kept}, (V, settings)


CHECKS = [check_hand_rows, check_dead_row, check_greedy, check_draws, lambda s: check_draws(s, counter=5)]


# --------------------------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", range(len(CHECKS)))
def test_cpu_path_meets_the_contract(check):
    CHECKS[check](cpu_path)


def _failure(check, sampler):
    try:
        check(sampler)
    except AssertionError as e:
        return str(e) or "failed"
    return None


def test_the_checks_pass_the_loop_sampler_and_fail_its_mutants():
    """The contract written as a loop passes every check; each mutant fails the check that is there to see it:
    dropped ties the kept size of the 'ties at k' hand row, the other two the acceptance of the draws."""
    for check in CHECKS:
        check(loop_sampler())
    msg = _failure(check_hand_rows, loop_sampler(ties=False))
    assert msg is not None and "ties at k" in msg, msg
    for mutant in (loop_sampler(order="mass"), loop_sampler(shift=1)):
        assert _failure(check_draws, mutant) is not None
        assert _failure(CHECKS[4], mutant) is not None  # and at draw counter 5
        assert _failure(check_greedy, mutant) is None  # greedy neither cumulates nor draws


def test_state_rules_over_five_steps():
    """draws, done, out and pad against a Python loop over the same tokens: rows hit EOS at different steps, out is
    narrower than the number of steps, a done row keeps drawing counters."""
    from picotron_amd import generate as G
    B, V, STEPS, EOS, PAD = 6, 9, 5, 4, 7
    g = torch.Generator().manual_seed(5)
    logits = [torch.randn(B, V, generator=g) * 2 for _ in range(STEPS)]
    out = torch.full((B, 4), -1, dtype=torch.int64)
    st = G.SamplerState(B, "cpu", temperature=1.0, eos_token_id=EOS, pad_token_id=PAD, seed=SEED, out=out)
    done, want_out, hit = [False] * B, [[-1] * 4 for _ in range(B)], 0
    for n in range(STEPS):
        toks = G.sample_tokens(logits[n], st).tolist()
        rs = R.draw_words(SEED, range(B), [n] * B)
        for b in range(B):
            if done[b]:
                assert toks[b] == PAD, (n, b)
            else:
                assert R.Row(logits[n][b].numpy(), 1.0).accepts(toks[b], rs[b], R.tau(V)), (n, b)
            done[b] = done[b] or toks[b] == EOS
            hit += toks[b] == EOS
            if n < 4:
                want_out[b][n] = toks[b]
        assert st.draws.tolist() == [n + 1] * B and st.done.tolist() == [int(d) for d in done]
        assert out.tolist() == want_out
    assert hit >= 1 and not all(done)
    st.reset()
    assert st.draws.tolist() == [0] * B and st.done.tolist() == [0] * B
    # without an EOS nothing is ever latched
    st2 = G.SamplerState(B, "cpu", temperature=1.0, seed=SEED)
    for n in range(STEPS):
        G.sample_tokens(logits[n], st2)
    assert st2.done.tolist() == [0] * B


def test_set_rewrites_params_in_place():
    from picotron_amd import generate as G
    x = torch.tensor([[0.0, 1.0, 3.0, 2.0, 2.5]]).expand(64, -1)
    st = G.SamplerState(64, "cpu", temperature=1.0, seed=3)
    params, ptr = st.params, st.params.data_ptr()
    assert len(set(G.sample_tokens(x, st).tolist())) > 1
    st.set(temperature=0.0)
    assert st.params is params and st.params.data_ptr() == ptr
    assert G.sample_tokens(x, st).tolist() == [2] * 64
    st.set(temperature=1.0, top_k=2)
    assert set(G.sample_tokens(x, st).tolist()) == {2, 4}
    st.set(top_k=None, seed=4)  # the other settings stay
    a = G.sample_tokens(x, st.reset()).tolist()
    b = G.sample_tokens(x, st.set(seed=3).reset()).tolist()
    assert a != b and len(set(a)) > 2
    # seed=None is torch.initial_seed(), as AdamW's sr_seed
    torch.manual_seed(99)
    c = G.sample_tokens(x, G.SamplerState(64, "cpu", temperature=1.0)).tolist()
    assert c == G.sample_tokens(x, G.SamplerState(64, "cpu", temperature=1.0, seed=99)).tolist()
    for bad in (dict(temperature=-1.0), dict(top_k=0), dict(top_p=0.0), dict(top_p=1.5), dict(eos_token_id=-2)):
        with pytest.raises(ValueError):
            st.set(**bad)


def test_generate_refuses_generator_with_the_fused_route():
    from picotron_amd import generate as G
    for kw in (dict(seed=1), dict(top_p=0.9), dict(graph=True)):
        with pytest.raises(ValueError, match="generator"):
            G.generate(None, torch.zeros(1, 2, dtype=torch.int64), 2, generator=torch.Generator(), **kw)


def test_sample_tokens_argument_errors():
    from picotron_amd import generate as G
    st = G.SamplerState(2, "cpu")
    with pytest.raises(ValueError):
        G.sample_tokens(torch.zeros(3, 4), st)
    with pytest.raises(ValueError):
        G.sample_tokens(torch.zeros(2, 8)[:, ::2], st)
    with pytest.raises(TypeError):
        G.sample_tokens(torch.zeros(2, 4, dtype=torch.int64), st)
    with pytest.raises(ValueError):
        G.SamplerState(2, "cpu", out=torch.zeros(3, 4, dtype=torch.int64))


@pytest.fixture(scope="module")
def lib():
    from picotron_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from picotron_amd.build import build
        build()
    return _lib.load()


def test_abi_argument_errors(lib):
    from picotron_amd import _lib
    assert "pico_sample" in _lib.EXPORTED_SYMBOLS and lib.pico_abi_version() == 2
    p = ctypes.c_void_p(64)

    def call(logits=p, dtype=0, rows=2, vocab=100, params=p, draws=p, tokens=p):
        return lib.pico_sample(logits, dtype, 100, rows, vocab, params, draws, None, tokens, None, 0, 0, None, None)

    for kw, word in ((dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(vocab=0), b"vocab"),
                     (dict(vocab=(1 << 20) + 1), b"vocab"), (dict(logits=None), b"null"), (dict(params=None), b"null"),
                     (dict(draws=None), b"null"), (dict(tokens=None), b"null"), (dict(rows=-1), b"rows")):
        assert call(**kw) == 1000, kw
        assert word in lib.pico_last_error(), (kw, lib.pico_last_error())
    assert call(rows=0) == 0  # nothing to do: no launch
