"""pico_sample (csrc/sample.hip) through picotron_amd.generate.sample_tokens, against the fp64 loop reference and the
acceptance rule of tests/sample_ref.py (tau(V) is derived there).

Inputs are chosen by seed on the CPU: a row is redrawn with its next seed until the reference's top-p cut clears
tau(V) under every setting (asserted again on what is used), and for each row, setting and draw counter the tokens
the rule accepts are written down before the kernel runs. No row is left out of any check."""
import numpy as np
import pytest
import torch

import sample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0x0BAD_5EED_0123_4567
B = 64
VOCABS = [1, 7, 255, 256, 257, 1000, 4099, 49152, 50257, 128256]
PADDED = {7, 257, 4099, 50257}  # row stride V + 3: rows start at every alignment of the vector load
SETTINGS = {
    "greedy": dict(temperature=0.0),
    "T0.7": dict(temperature=0.7),
    "k50": dict(temperature=1.0, top_k=50),
    "p0.9": dict(temperature=1.0, top_p=0.9),
    "k50p0.9": dict(temperature=1.0, top_k=50, top_p=0.9),
    "T0.05": dict(temperature=0.05),
    "T50": dict(temperature=50.0),
}
COUNTERS = (0, 1)


def _rows_with_margin(make_row, n, settings):
    """n rows, row b = make_row(b, attempt) for the first attempt whose top-p cut clears tau under every setting;
    per row and setting: (kept, argmax, acceptable tokens per counter)."""
    rows, refs = [], []
    for b in range(n):
        for attempt in range(32):
            x = make_row(b, attempt)
            xs = x.float().numpy()
            order = np.argsort(-R.canon(xs))
            rr = {k: R.Row(xs, s["temperature"], s.get("top_k"), s.get("top_p"), order=order)
                  for k, s in settings.items()}
            if all(r.margin > R.tau(len(xs)) for r in rr.values()):
                break
        assert all(r.margin > R.tau(len(xs)) for r in rr.values()), (b, "no seed gives the cut a margin")
        rows.append(x)
        draws = {c: R.draw_words(SEED, [b], [c])[0] for c in COUNTERS}
        refs.append({k: (r.kept, r.argmax, {c: r.acceptable(draws[c], R.tau(len(xs))) for c in COUNTERS})
                     for k, r in rr.items()})
    return torch.stack(rows), refs


_CASES = {}


def _case(V, dtype):
    """Logits randn * 4 [64, V] in `dtype` on the CPU and their reference (computed once, shared, never changed)."""
    if (V, dtype) not in _CASES:
        def make_row(b, attempt):
            g = torch.Generator().manual_seed((V * 64 + b) * 32 + attempt)
            return (torch.randn(V, generator=g) * 4).to(dtype)
        _CASES[V, dtype] = _rows_with_margin(make_row, B, SETTINGS)
    return _CASES[V, dtype]


def _device_logits(x, padded):
    if not padded:
        return x.to(DEV)
    wide = torch.full((x.shape[0], x.shape[1] + 3), 1e30, dtype=x.dtype, device=DEV)  # a read past a row would win
    wide[:, :x.shape[1]] = x.to(DEV)
    return wide[:, :x.shape[1]]


def _check(tokens, kept, refs, name, counter):
    tokens, kept = tokens.tolist(), kept.tolist()
    for b, ref in enumerate(refs):
        want_kept, _, ok = ref[name]
        assert tokens[b] in ok[counter], (name, counter, b, tokens[b], ok[counter])
        assert kept[b] == want_kept, (name, b, kept[b], want_kept)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", VOCABS)
def test_tokens_are_accepted(V, dtype):
    """Every setting, every row: the token is one the rule accepts and `kept` is the reference's count, for the
    first draw and for the second (counter 1) on the same logits; greedy is the lowest index of the maximum."""
    from picotron_amd import generate as G
    x, refs = _case(V, dtype)
    xd = _device_logits(x, V in PADDED)
    assert xd.stride(0) == V + (3 if V in PADDED else 0)
    for name, settings in SETTINGS.items():
        st = G.SamplerState(B, DEV, seed=SEED, **settings)
        for counter in COUNTERS:
            tok, kept = G.sample_tokens(xd, st, return_kept=True)
            assert tok.dtype == torch.int64 and kept.dtype == torch.int32
            _check(tok.cpu(), kept.cpu(), refs, name, counter)
            assert st.draws.tolist() == [counter + 1] * B
    st = G.SamplerState(B, DEV, seed=SEED, temperature=0.0)
    tok = G.sample_tokens(xd, st).cpu()
    assert tok.tolist() == [ref["greedy"][1] for ref in refs]
    xf = x.float()
    unique = (xf == xf.max(-1, keepdim=True).values).sum(-1) == 1
    assert unique.any() and torch.equal(tok[unique], xf.argmax(-1)[unique])


def _structured(V):
    """Rows that exercise the rules rather than the arithmetic, on a randn * 4 background (bounded by 24):
    0: 60 entries tied at the top (top-k 50 keeps all 60); 1: 10 entries tied far above the rest (the top-p cut falls
    inside the tie: all 10 stay); 2: one-hot (one finite entry); 3: every other entry banned with -inf; 4: NaN
    entries; 5: all -inf; 6: a +inf entry and a -0 / +0 pair; 7: the maximum planted at three indices."""
    def make_row(b, attempt):
        g = torch.Generator().manual_seed((V * 8 + b) * 32 + attempt)
        x = torch.randn(V, generator=g) * 4
        pick = torch.randperm(V, generator=g)
        if b == 0:
            x[pick[:60]] = 30.0
        elif b == 1:
            x[pick[:10]] = 60.0
        elif b == 2:
            x[:] = float("-inf")
            x[pick[0]] = 0.25
        elif b == 3:
            x[::2] = float("-inf")
        elif b == 4:
            x[pick[:V // 3]] = float("nan")
        elif b == 5:
            x[:] = float("-inf")
        elif b == 6:
            x[pick[0]] = float("inf")
            x[pick[1]], x[pick[2]] = -0.0, 0.0
        else:
            x[pick[:3]] = 31.0
        return x
    return make_row


@pytest.mark.parametrize("V", [1000, 49152])
def test_structured_rows(V):
    from picotron_amd import generate as G
    key = (V, "structured")
    if key not in _CASES:
        _CASES[key] = _rows_with_margin(_structured(V), 8, SETTINGS)
    x, refs = _CASES[key]
    assert refs[0]["k50"][0] == 60 and refs[1]["p0.9"][0] == 10 and refs[1]["k50p0.9"][0] == 10
    assert refs[5]["T0.7"][0] == 0 and refs[5]["greedy"][2][0] == [0]
    assert refs[7]["greedy"][1] == int((x[7] == 31.0).nonzero()[0])
    xd = x.to(DEV)
    for name, settings in SETTINGS.items():
        st = G.SamplerState(8, DEV, seed=SEED, **settings)
        for counter in COUNTERS:
            tok, kept = G.sample_tokens(xd, st, return_kept=True)
            _check(tok.cpu(), kept.cpu(), refs, name, counter)


@pytest.mark.parametrize("V,dtype", [(1000, torch.float32), (50257, torch.bfloat16), (50257, torch.float32)])
def test_deterministic_and_row_independent(V, dtype):
    """Equal state gives equal tokens; row b's token depends on row b's logits, b and draws[b] only: the other rows
    replaced (and their counters changed) leave it alone."""
    from picotron_amd import generate as G
    x, _ = _case(V, dtype)
    xd = _device_logits(x, True)
    for settings in (SETTINGS["T0.7"], SETTINGS["k50p0.9"], SETTINGS["p0.9"]):
        st = G.SamplerState(B, DEV, seed=SEED, **settings)
        st.draws.copy_(torch.arange(B, dtype=torch.int32) % 5)  # rows at different counters
        start = st.draws.clone()
        tok, kept = [t.clone() for t in G.sample_tokens(xd, st, return_kept=True)]
        for _ in range(3):
            st.draws.copy_(start)
            again, kept2 = G.sample_tokens(xd, st, return_kept=True)
            assert torch.equal(again, tok) and torch.equal(kept2, kept)
        other = xd.clone()
        perm = torch.roll(torch.arange(B, device=DEV), 1)
        keep_rows = torch.arange(B, device=DEV) % 4 == 0
        other[~keep_rows] = xd[perm][~keep_rows]
        st.draws.copy_(torch.where(keep_rows, start, start + 7))
        mixed = G.sample_tokens(other, st)
        assert torch.equal(mixed[keep_rows], tok[keep_rows])
        assert not torch.equal(mixed[~keep_rows], tok[~keep_rows])


def test_guard_bands_and_state_rules():
    """tokens, out, done, draws and kept are windows of larger sentinel-filled tensors: nothing outside their own
    positions changes, out is written at column n only and not at all once n >= out_cols. A done row yields pad and
    still advances its counter; an EOS drawn this step latches done."""
    from picotron_amd import generate as G
    V, COLS, PAD, G0 = 257, 3, 11, 5
    x, refs = _case(V, torch.float32)
    xd = x.to(DEV)
    greedy = [ref["greedy"][1] for ref in refs]
    EOS = greedy[0]
    st = G.SamplerState(B, DEV, temperature=0.0, eos_token_id=EOS, pad_token_id=PAD, seed=SEED)
    big = {"tokens": torch.full((B + 2 * G0,), -7, dtype=torch.int64, device=DEV),
           "draws": torch.full((B + 2 * G0,), -7, dtype=torch.int32, device=DEV),
           "kept": torch.full((B + 2 * G0,), -7, dtype=torch.int32, device=DEV),
           "done": torch.full((B + 2 * G0,), 77, dtype=torch.uint8, device=DEV),
           "out": torch.full((B + 2, COLS + 2 * G0), -7, dtype=torch.int64, device=DEV)}
    st.tokens, st.draws, st.kept, st.done = (big[k][G0:G0 + B] for k in ("tokens", "draws", "kept", "done"))
    st.out = big["out"][1:B + 1, G0:G0 + COLS]
    st.draws.zero_()
    st.done.zero_()
    st.done[3] = 1  # done before the first step
    is_eos = [t == EOS for t in greedy]
    want_out = torch.full((B, COLS), -7, dtype=torch.int64)
    for n in range(COLS + 2):
        tok = G.sample_tokens(xd, st).cpu()
        for b in range(B):
            done_before = b == 3 or (n > 0 and is_eos[b])
            assert int(tok[b]) == (PAD if done_before else greedy[b]), (n, b)
            if n < COLS:
                want_out[b, n] = tok[b]
        assert st.draws.tolist() == [n + 1] * B
        assert st.done.tolist() == [int(b == 3 or is_eos[b]) for b in range(B)]
        assert st.kept.tolist() == [0 if (b == 3 or (n > 0 and is_eos[b])) else 1 for b in range(B)]
        assert torch.equal(st.out.cpu(), want_out)
        for k in ("tokens", "draws", "kept", "done"):
            s = 77 if k == "done" else -7
            assert (big[k][:G0] == s).all() and (big[k][G0 + B:] == s).all(), k
        o = big["out"].clone()
        o[1:B + 1, G0:G0 + COLS] = -7
        assert (o == -7).all()
    assert is_eos[0] and not all(is_eos)
    # without done / out / kept buffers the launch writes tokens and draws only
    st2 = G.SamplerState(B, DEV, temperature=0.0, seed=SEED)
    st2.out = None
    assert G.sample_tokens(xd, st2).tolist() == greedy


def test_sample_tokens_does_not_synchronise():
    from picotron_amd import generate as G
    x, refs = _case(1000, torch.float32)
    xd = x.to(DEV)
    st = G.SamplerState(B, DEV, seed=SEED, out=torch.zeros((B, 4), dtype=torch.int64, device=DEV),
                        **SETTINGS["k50p0.9"])
    G.sample_tokens(xd, st)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tok, kept = G.sample_tokens(xd, st, return_kept=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    _check(tok.cpu(), kept.cpu(), refs, "k50p0.9", 1)


def test_refuses_other_dtypes_on_the_device():
    from picotron_amd import generate as G
    st = G.SamplerState(2, DEV)
    with pytest.raises(TypeError):
        G.sample_tokens(torch.zeros(2, 8, dtype=torch.float16, device=DEV), st)
    with pytest.raises(ValueError):
        G.sample_tokens(torch.zeros(2, 8), st)
