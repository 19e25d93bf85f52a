"""pico_decode_linear on the GPU against the fp64 reference and bounds of tests/decode_linear_ref.py, on NaN-guarded
buffers; determinism and row independence bit for bit; decode_step / generate with skinny_linear=True against the
yardstick and the graph rules of tests/test_generate_gpu.py.

Shapes from csrc/decode_linear_plan.h: a workgroup owns 32 rows of W (SWIGLU 16 + 16), a K step is 32, a wave's trip
128; the default rule first splits a single column block at K = 1024 and every shape beyond K = 2048."""
import pytest
import torch

import decode_linear_ref as D
import test_generate_gpu as TG

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"
# (N, K, split_k): one K step; a partial second block, a trip and a lone step; N = 8, two trips on wave 0 (the
# prefetch); the rule's first split and one below it; more than one LDS slice; an explicit split with a short last slice
SHAPES = [(32, 32, 0), (40, 160, 0), (8, 640, 0), (64, 1024, 0), (64, 992, 0), (72, 2080, 0), (40, 160, 2)]
FORMS = ["f32", "norm", "norm_res", "norm_res_noout"]


def _run(form, M, N, K, split_k, **strides):
    x, w, nw, res = D.inputs(M, N, K)
    kw = dict(norm_weight=nw, residual=res if "res" in form else None) if "norm" in form else {}
    ref = D.reference(x, w, **kw)
    got = D.launch(x, w, f32=form == "f32", split_k=split_k, want_res_out="noout" not in form, **kw, **strides)
    if got["residual_out"] is None:
        ref["residual_out"] = None
    elif ref["residual_out"] is None:  # residual_out without a residual: x itself
        ref["residual_out"] = x
    D.check(f"decode_linear {form} M{M} N{N} K{K} split{split_k}", got, ref)
    return got


@pytest.mark.parametrize("M", [1, 3, 8, 16])
@pytest.mark.parametrize("N,K,split_k", SHAPES)
def test_projection_matches_fp64(M, N, K, split_k):
    if split_k == 0 and K in (992, 1024):
        from picotron_amd import _lib
        assert _lib.load().pico_decode_linear_split_k(N, K, 0) == (2 if K == 1024 else 1)
    _run("bf16", M, N, K, split_k)


@pytest.mark.parametrize("M", [3, 16])
@pytest.mark.parametrize("N,K,split_k", [(176, 160, 0), (272, 192, 2)])
@pytest.mark.parametrize("form", FORMS)
def test_forms_match_fp64(form, M, N, K, split_k):
    _run(form, M, N, K, split_k)


@pytest.mark.parametrize("M", [3, 16])
@pytest.mark.parametrize("N,K,split_k", [(176, 160, 1), (272, 192, 2), (144, 1024, 2), (80, 2080, 2)])
@pytest.mark.parametrize("form", ["bf16", "norm_res"])
def test_swiglu_is_the_epilogue_of_the_same_projection(form, M, N, K, split_k):
    """SWIGLU against pico_swiglu_fwd on the BF16 run's output for the same stacked W and split_k, bit for bit (the
    BF16 run itself is inside the fp64 bound): randn, a partial last block, two trips on one wave, two LDS slices."""
    y = _run(form, M, N, K, split_k)["y"]
    x, w, nw, res = D.inputs(M, N, K)
    kw = dict(norm_weight=nw, residual=res) if form == "norm_res" else {}
    act = D.launch(x, w, swiglu=True, split_k=split_k, **kw)["y"]
    assert torch.equal(act.contiguous().view(torch.int16), D.swiglu_of(y, exact=True).contiguous().view(torch.int16))


def test_strided_rows():
    _run("bf16", 3, 40, 160, 0, ldx=168, ldw=176)


@pytest.mark.parametrize("M,N,K,split_k", [(16, 72, 640, 0), (5, 40, 2080, 0), (16, 64, 256, 4)])
def test_planted_weights_name_what_was_read(M, N, K, split_k):
    x, w = D.planted(M, N, K)
    y = D.launch(x, w, split_k=split_k)["y"].cpu()
    assert torch.equal(y.float(), x.float()[:, (5 * torch.arange(N) + 3) % K])


@pytest.mark.parametrize("form,N,K,split_k", [("bf16", 72, 2080, 0), ("norm_res_swiglu", 80, 1024, 2)])
def test_deterministic_and_row_independent(form, N, K, split_k):
    x, w, nw, res = D.inputs(16, N, K)
    kw = dict(swiglu="swiglu" in form, split_k=split_k)
    if "norm" in form:
        kw.update(norm_weight=nw, residual=res)
    bits = lambda t: t.contiguous().view(torch.int16)
    y = bits(D.launch(x, w, **kw)["y"])
    assert torch.equal(y, bits(D.launch(x, w, **kw)["y"]))
    for m in (0, 9, 15):
        if "norm" in form:
            kw["residual"] = res[m:m + 1]
        assert torch.equal(bits(D.launch(x[m:m + 1], w, **kw)["y"]), y[m:m + 1]), m


@pytest.mark.parametrize("kind", ["gqa2", "d128"])
def test_decode_step_skinny_within_the_yardstick(golden_loss, kind):
    from picotron_amd import generate as G
    m, orc, cfg = TG._tiny(golden_loss, kind)
    toks = torch.randint(0, cfg.vocab_size, (2, 24), generator=torch.Generator().manual_seed(17)).to(DEV)
    want, yard = TG._oracle_and_yardstick(m, orc, toks)
    cache = G.KVCache(m, 2, 32)
    G.prefill(m, toks[:, :5].contiguous(), cache)
    got = torch.stack([G.decode_step(m, toks[:, j], cache, skinny_linear=True) for j in range(5, 24)], 1).cpu()
    TG._within(got, want[:, 5:24], yard, f"{kind} decode_step(skinny_linear=True)")


def test_generate_skinny_graph_equals_eager(golden_loss):
    from picotron_amd import generate as G
    m, _, cfg = TG._tiny(golden_loss, "gqa2")
    prompt = torch.randint(0, cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(23)).to(DEV)
    base = G.generate(m, prompt, 12, seed=5)  # the default route: the flag off, eager or replayed, changes nothing
    assert torch.equal(G.generate(m, prompt, 12, seed=5, skinny_linear=False), base)
    assert torch.equal(G.generate(m, prompt, 12, seed=5, graph=True), base)
    te, le = G.generate(m, prompt, 12, seed=5, skinny_linear=True, return_logits=True)
    cache = G.KVCache(m, 2, 32)
    tg, lg = G.generate(m, prompt, 12, seed=5, graph=True, skinny_linear=True, return_logits=True, cache=cache)
    assert torch.equal(tg, te) and torch.equal(lg, le)
    kw = dict(temperature=0.8, top_k=20, top_p=0.9, seed=7, skinny_linear=True)
    assert torch.equal(G.generate(m, prompt, 12, graph=True, cache=cache, **kw), G.generate(m, prompt, 12, **kw))
    assert cache.graph_captures == 1
    G.generate(m, prompt, 12, seed=5, graph=True, cache=cache)  # the other route: its own capture, not a replay
    assert cache.graph_captures == 2
    with pytest.raises(ValueError, match="at most 16"):
        G.generate(m, torch.zeros(17, 4, dtype=torch.int64, device=DEV), 2, skinny_linear=True)
