"""pico_quantize_rows_fp8 and pico_decode_linear_fp8 on the GPU, on NaN-guarded buffers, against the CPU restatement
(bit for bit), exact one-hot products and tests/decode_linear_ref.py's fp64 reference and bound on the dequantised
weight. The cases are tests/test_decode_linear_fp8_host.py's: a K step is 64 columns, a trip 256."""
import copy
import ctypes

import pytest
import torch

import attn_ref as A
import decode_linear_ref as D
import test_decode_linear_fp8_host as H
import test_generate_gpu as TG

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(x, q, norm_weight=None, eps=1e-5, residual=None, want_res_out=True, swiglu=False, f32=False, split_k=0):
    """pico_decode_linear_fp8 on guarded buffers (D.launch's layout; the codes' rows 16 bytes apart from the next)."""
    from picotron_amd import _lib as L
    lib = L.load()
    (M, K), N = x.shape, q.shape[0]
    epi = L.DL_SWIGLU if swiglu else (L.DL_F32 if f32 else L.DL_BF16)
    G = A.Guards(torch.device(DEV))
    xg = G.mat("x", M, K, data=x.to(DEV), ld=K + 8)
    wg = G.mat("codes", N, K, dtype=torch.uint8, data=q.codes.view(torch.uint8).to(DEV), ld=K + 16)
    sg = G.flat("scale", N, F32, data=q.scale.to(DEV))
    outs = N // 2 if swiglu else N
    y = G.mat("y", M, outs, dtype=F32 if f32 else BF, ld=outs + 8)
    a = L.DecodeLinearFp8Args()
    a.x, a.weight, a.weight_scale, a.y = xg.data_ptr(), wg.data_ptr(), sg.data_ptr(), y.data_ptr()
    a.ldx, a.ldw, a.ldy = xg.stride(0), wg.stride(0), y.stride(0)
    ro = None
    if norm_weight is not None:
        a.norm_weight = G.mat("norm_weight", 1, K, data=norm_weight.to(DEV)).data_ptr()
        if residual is not None:
            rg = G.mat("residual", M, K, data=residual.to(DEV), ld=K + 8)
            a.residual, a.ldr = rg.data_ptr(), rg.stride(0)
        if want_res_out:
            ro = G.mat("residual_out", M, K, ld=K + 16)
            a.residual_out, a.ldro = ro.data_ptr(), ro.stride(0)
    plan = (ctypes.c_int64 * 4)()
    assert lib.pico_decode_linear_fp8_plan(M, N, K, epi, split_k, 0, plan) == 0, lib.pico_last_error()
    if plan[3]:
        a.workspace = G.flat("workspace", plan[3], torch.uint8).data_ptr()
    a.m, a.n, a.k, a.split_k, a.eps, a.epilogue = M, N, K, split_k, eps, epi
    G.arm()
    L.check(lib.pico_decode_linear_fp8(ctypes.byref(a), L.stream_of(xg)), "pico_decode_linear_fp8")
    torch.cuda.synchronize()
    G.check()
    return {"y": y, "residual_out": ro, "split_k": plan[1]}


@pytest.mark.parametrize("N,K", H.QUANT_SHAPES)
def test_quantiser_equals_the_restatement(N, K):
    from picotron_amd import _lib as L, ops
    w = H.quant_input(N, K)
    want = ops.quantize_weight_fp8(w)
    G = A.Guards(torch.device(DEV))
    wg = G.mat("w", N, K, data=w.to(DEV), ld=K + 24)
    codes = G.mat("codes", N, K, dtype=torch.uint8, ld=K + 8)
    scale = G.flat("scale", N, F32)
    G.arm()
    L.check(L.load().pico_quantize_rows_fp8(wg.data_ptr(), wg.stride(0), codes.data_ptr(), codes.stride(0),
                                            scale.data_ptr(), N, K, L.stream_of(wg)), "pico_quantize_rows_fp8")
    torch.cuda.synchronize()
    G.check()
    assert torch.equal(scale.cpu().view(torch.int32), want.scale.view(torch.int32))
    assert torch.equal(codes.cpu(), want.codes.view(torch.uint8))
    assert not bool((codes & 0x7f == 0x7f).any())


@pytest.mark.parametrize("split_k", [1, 2])
@pytest.mark.parametrize("K", [64, 320])
@pytest.mark.parametrize("M", [1, 16])
def test_every_code_at_every_k_position(M, K, split_k):
    x, q, want = H.one_hot_case(M, K)
    assert torch.equal(_launch(x, q, split_k=split_k)["y"].float().cpu(), want)


def _run(form, M, N, K, split_k):
    x, q, w64, nw, res = H.fp8_case(M, N, K)
    kw = H.form_kwargs(form, nw, res)
    ref = D.reference(x, w64, **kw)
    got = _launch(x, q, f32=form == "f32", split_k=split_k, want_res_out="noout" not in form, **kw)
    if got["residual_out"] is None:
        ref["residual_out"] = None
    elif ref["residual_out"] is None:  # residual_out without a residual: x itself
        ref["residual_out"] = x
    D.check(f"decode_linear_fp8 {form} M{M} N{N} K{K} split{split_k}", got, ref)
    return got


@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("form,N,K,split_k", [("bf16", *s) for s in H.SHAPES] +
                         [(f, *s) for f in H.FORMS for s in H.FORM_SHAPES])
def test_projection_matches_fp64(form, M, N, K, split_k):
    got = _run(form, M, N, K, split_k)
    assert got["split_k"] == {1024: 2, 2112: 4}.get(K, split_k or 1)  # the default rule's splits


@pytest.mark.parametrize("M", [3, 16])
@pytest.mark.parametrize("N,K,split_k", [(176, 320, 1), (144, 1024, 2)])
@pytest.mark.parametrize("form", ["bf16", "norm_res"])
def test_swiglu_is_the_epilogue_of_the_same_projection(form, M, N, K, split_k):
    y = _run(form, M, N, K, split_k)["y"]
    x, q, _, nw, res = H.fp8_case(M, N, K)
    act = _launch(x, q, swiglu=True, split_k=split_k, **H.form_kwargs(form, nw, res))["y"]
    assert torch.equal(_bits(act), _bits(D.swiglu_of(y, exact=True)))


@pytest.mark.parametrize("form,N,K,split_k", [("bf16", 72, 1280, 1), ("norm_res_swiglu", 80, 1024, 2)])
def test_deterministic_and_row_independent(form, N, K, split_k):
    x, q, _, nw, res = H.fp8_case(16, N, K)
    kw = dict(swiglu="swiglu" in form, split_k=split_k, **H.form_kwargs(form, nw, res))
    y = _bits(_launch(x, q, **kw)["y"])
    assert torch.equal(y, _bits(_launch(x, q, **kw)["y"]))
    if "norm" in form:
        kw["residual"] = res[5:6]
    assert torch.equal(_bits(_launch(x[5:6], q, **kw)["y"]), y[5:6])


def _fp8_models(golden_loss, kind):
    """(the tiny model on bf16(scale * e4m3(code)), the fp32 oracle on scale * e4m3(code) exactly, the DecodeWeights)."""
    from picotron_amd import generate as G
    m, orc, cfg = TG._tiny(golden_loss, kind)
    m2, orc2 = copy.deepcopy(m), copy.deepcopy(orc)
    w = G.quantize_decode_weights(m2)
    sd = {k: v.detach().float().cpu() for k, v in m2.state_dict().items()}
    for i, (qkv, out, gu, down) in enumerate(w.layers):
        a, f, (nq, nk) = f"decoder_layers.{i}.attention.", f"decoder_layers.{i}.mlp.", (cfg.hidden_size, qkv.shape[0])
        nk, inter = (nk - nq) // 2, gu.shape[0] // 2
        qkv, out, gu, down = (t.dequantize().cpu() for t in (qkv, out, gu, down))
        sd.update({a + "q_proj.weight": qkv[:nq], a + "k_proj.weight": qkv[nq:nq + nk],
                   a + "v_proj.weight": qkv[nq + nk:], a + "out_proj.weight": out, f + "gate_proj.weight": gu[:inter],
                   f + "up_proj.weight": gu[inter:], f + "down_proj.weight": down})
    sd["final_proj.weight"] = w.head.dequantize().cpu()
    orc2.load_state_dict(sd, strict=True)
    m2.load_state_dict({k: v.to(BF) for k, v in sd.items()}, strict=True)
    return m2, orc2, cfg, w


@pytest.mark.parametrize("kind", ["gqa2", "d128"])
def test_decode_step_fp8_within_the_bf16_skinny_yardstick(golden_loss, kind):
    """Teacher-forced: the FP8 route within 2x the bf16 skinny route's error; both prefill on the same weights."""
    from picotron_amd import generate as G
    m2, orc2, cfg, w = _fp8_models(golden_loss, kind)
    toks = torch.randint(0, cfg.vocab_size, (2, 24), generator=torch.Generator().manual_seed(17)).to(DEV)
    with torch.no_grad():
        want = orc2(toks.cpu())[:, 5:24]
    runs = []
    for dw in (None, w):
        cache = G.KVCache(m2, 2, 32)
        G.prefill(m2, toks[:, :5].contiguous(), cache)
        runs.append(torch.stack([G.decode_step(m2, toks[:, j], cache, skinny_linear=True, decode_weights=dw)
                                 for j in range(5, 24)], 1).cpu())
    yard = (TG.max_abs(runs[0], want), TG.rel_l2(runs[0], want))
    TG._within(runs[1], want, yard, f"{kind} decode_step(decode_weights=w) [yardstick: the bf16 skinny route]")


def test_generate_fp8_graph_equals_eager(golden_loss):
    from picotron_amd import generate as G
    m2, _, cfg, w = _fp8_models(golden_loss, "gqa2")
    prompt = torch.randint(0, cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(23)).to(DEV)
    kw = dict(seed=5, skinny_linear=True, decode_weights=w, return_logits=True)
    te, le = G.generate(m2, prompt, 12, **kw)
    cache = G.KVCache(m2, 2, 32)
    tg, lg = G.generate(m2, prompt, 12, graph=True, cache=cache, **kw)
    assert torch.equal(tg, te) and torch.equal(lg, le)
    assert not torch.equal(le, G.generate(m2, prompt, 12, seed=5, skinny_linear=True, return_logits=True)[1])
    kw = dict(temperature=0.8, top_k=20, top_p=0.9, seed=7, skinny_linear=True, decode_weights=w)
    assert torch.equal(G.generate(m2, prompt, 12, graph=True, cache=cache, **kw), G.generate(m2, prompt, 12, **kw))
    assert cache.graph_captures == 1
    kw["decode_weights"] = G.quantize_decode_weights(m2)  # another snapshot: its own capture, not a replay
    assert torch.equal(G.generate(m2, prompt, 12, graph=True, cache=cache, **kw), G.generate(m2, prompt, 12, **kw))
    assert cache.graph_captures == 2
