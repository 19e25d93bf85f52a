"""pico_quantize_rows_mxfp4 and pico_decode_linear_mxfp4 on the GPU, on NaN-guarded buffers, against the CPU
restatement (bit for bit), exact one-hot products and tests/decode_linear_ref.py's fp64 reference and bound on the
dequantised weight. The cases are tests/test_decode_linear_mxfp4_host.py's: a K step is 128 columns, a trip 512."""
import copy
import ctypes

import pytest
import torch

import attn_ref as A
import decode_linear_ref as D
import test_decode_linear_mxfp4_host as H
import test_generate_gpu as TG

pytestmark = pytest.mark.gpu
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(x, q, norm_weight=None, eps=1e-5, residual=None, want_res_out=True, swiglu=False, f32=False, split_k=0):
    """pico_decode_linear_mxfp4 on guarded buffers (D.launch's layout; code rows 16, scale rows 4 bytes apart)."""
    from picotron_amd import _lib as L
    lib = L.load()
    (M, K), N = x.shape, q.shape[0]
    epi = L.DL_SWIGLU if swiglu else (L.DL_F32 if f32 else L.DL_BF16)
    G = A.Guards(torch.device(DEV))
    xg = G.mat("x", M, K, data=x.to(DEV), ld=K + 8)
    wg = G.mat("codes", N, K // 2, dtype=U8, data=q.codes.to(DEV), ld=K // 2 + 16)
    sg = G.mat("scales", N, K // 32, dtype=U8, data=q.scales.to(DEV), ld=K // 32 + 4)
    outs = N // 2 if swiglu else N
    y = G.mat("y", M, outs, dtype=F32 if f32 else BF, ld=outs + 8)
    a = L.DecodeLinearMxfp4Args()
    a.x, a.weight, a.weight_scale, a.y = xg.data_ptr(), wg.data_ptr(), sg.data_ptr(), y.data_ptr()
    a.ldx, a.ldw, a.lds, a.ldy = xg.stride(0), wg.stride(0), sg.stride(0), y.stride(0)
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
    assert lib.pico_decode_linear_mxfp4_plan(M, N, K, epi, split_k, 0, plan) == 0, lib.pico_last_error()
    if plan[3]:
        a.workspace = G.flat("workspace", plan[3], U8).data_ptr()
    a.m, a.n, a.k, a.split_k, a.eps, a.epilogue = M, N, K, split_k, eps, epi
    G.arm()
    L.check(lib.pico_decode_linear_mxfp4(ctypes.byref(a), L.stream_of(xg)), "pico_decode_linear_mxfp4")
    torch.cuda.synchronize()
    G.check()
    return {"y": y, "residual_out": ro, "split_k": plan[1]}


@pytest.mark.parametrize("N,K", H.QUANT_SHAPES)
def test_quantiser_equals_the_restatement(N, K):
    from picotron_amd import _lib as L, ops
    w = H.quant_input(N, K)
    want = ops.quantize_weight_mxfp4(w)
    G = A.Guards(torch.device(DEV))
    wg = G.mat("w", N, K, data=w.to(DEV), ld=K + 24)
    codes = G.mat("codes", N, K // 2, dtype=U8, ld=K // 2 + 4)
    scales = G.mat("scales", N, K // 32, dtype=U8, ld=K // 32 + 3)
    G.arm()
    L.check(L.load().pico_quantize_rows_mxfp4(wg.data_ptr(), wg.stride(0), codes.data_ptr(), codes.stride(0),
                                              scales.data_ptr(), scales.stride(0), N, K, L.stream_of(wg)),
            "pico_quantize_rows_mxfp4")
    torch.cuda.synchronize()
    G.check()
    assert torch.equal(scales.cpu(), want.scales)
    assert torch.equal(codes.cpu(), want.codes)
    dev = ops.quantize_weight_mxfp4(w.to(DEV))  # the public entry point on the device
    assert torch.equal(dev.codes.cpu(), want.codes) and torch.equal(dev.scales.cpu(), want.scales)


@pytest.mark.parametrize("split_k", [1, 2])
@pytest.mark.parametrize("K", [128, 640])
@pytest.mark.parametrize("M", [1, 16])
def test_every_code_at_every_k_position(M, K, split_k):
    x, q, want = H.one_hot_case(M, K)
    assert torch.equal(_launch(x, q, split_k=split_k)["y"].float().cpu(), want)


def _run(form, M, N, K, split_k):
    x, q, w64, nw, res = H.mx_case(M, N, K)
    kw = H.form_kwargs(form, nw, res)
    ref = D.reference(x, w64, **kw)
    got = _launch(x, q, f32=form == "f32", split_k=split_k, want_res_out="noout" not in form, **kw)
    if got["residual_out"] is None:
        ref["residual_out"] = None
    elif ref["residual_out"] is None:  # residual_out without a residual: x itself
        ref["residual_out"] = x
    D.check(f"decode_linear_mxfp4 {form} M{M} N{N} K{K} split{split_k}", got, ref)
    return got


@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("form,N,K,split_k", [("bf16", *s) for s in H.SHAPES] +
                         [(f, *s) for f in H.FORMS for s in H.FORM_SHAPES])
def test_projection_matches_fp64(form, M, N, K, split_k):
    got = _run(form, M, N, K, split_k)
    assert got["split_k"] == (split_k or {2048: 2, 2176: 2}.get(K, 1))  # the default rule's splits


@pytest.mark.parametrize("M", [3, 16])
@pytest.mark.parametrize("N,K,split_k", [(176, 640, 1), (144, 2048, 2)])
@pytest.mark.parametrize("form", ["bf16", "norm_res"])
def test_swiglu_is_the_epilogue_of_the_same_projection(form, M, N, K, split_k):
    y = _run(form, M, N, K, split_k)["y"]
    x, q, _, nw, res = H.mx_case(M, N, K)
    act = _launch(x, q, swiglu=True, split_k=split_k, **H.form_kwargs(form, nw, res))["y"]
    assert torch.equal(_bits(act), _bits(D.swiglu_of(y, exact=True)))


@pytest.mark.parametrize("form,N,K,split_k", [("bf16", 72, 1664, 1), ("norm_res_swiglu", 80, 2048, 2)])
def test_deterministic_and_row_independent(form, N, K, split_k):
    x, q, _, nw, res = H.mx_case(16, N, K)
    kw = dict(swiglu="swiglu" in form, split_k=split_k, **H.form_kwargs(form, nw, res))
    y = _bits(_launch(x, q, **kw)["y"])
    assert torch.equal(y, _bits(_launch(x, q, **kw)["y"]))
    if "norm" in form:
        kw["residual"] = res[5:6]
    assert torch.equal(_bits(_launch(x[5:6], q, **kw)["y"]), y[5:6])


def _mx_models(golden_loss, kind):
    """(the tiny model on the dequantised MXFP4 weights, exactly bf16; the fp32 oracle on the same values; the set)."""
    from picotron_amd import generate as G
    m, orc, cfg = TG._tiny(golden_loss, kind)
    m2, orc2 = copy.deepcopy(m), copy.deepcopy(orc)
    w = G.quantize_decode_weights(m2, fmt="mxfp4")
    with torch.no_grad():
        for layer, (qkv, out, gu, down) in zip(m2.decoder_layers, w.layers):
            a, f = layer.attention, layer.mlp
            for mods, t in (((a.q_proj, a.k_proj, a.v_proj), qkv), ((a.out_proj,), out),
                            ((f.gate_proj, f.up_proj), gu), ((f.down_proj,), down)):
                for mod, rows in zip(mods, t.dequantize(BF).split([mod.weight.shape[0] for mod in mods])):
                    mod.weight.copy_(rows)
        m2.final_proj.weight.copy_(w.head.dequantize(BF))
    orc2.load_state_dict({k: v.detach().float().cpu() for k, v in m2.state_dict().items()}, strict=True)
    return m2, orc2, cfg, w


@pytest.mark.parametrize("kind", ["gqa2", "d128"])
def test_decode_and_extend_step_within_the_bf16_skinny_yardstick(golden_loss, kind):
    """Teacher-forced against the fp32 oracle: the MXFP4 route, then one extend_step of 4 tokens, within 2x the bf16
    skinny route's error on the same (dequantised) weights."""
    from picotron_amd import generate as G
    m2, orc2, cfg, w = _mx_models(golden_loss, kind)
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
    TG._within(runs[1], want, yard, f"{kind} decode_step(mxfp4) [yardstick: the bf16 skinny route]")
    cache = G.KVCache(m2, 2, 32)
    G.prefill(m2, toks[:, :5].contiguous(), cache)
    ext = G.extend_step(m2, toks[:, 5:9].contiguous(), cache, skinny_linear=True, decode_weights=w).cpu()
    yard4 = (TG.max_abs(runs[0][:, :4], want[:, :4]), TG.rel_l2(runs[0][:, :4], want[:, :4]))
    TG._within(ext, want[:, :4], yard4, f"{kind} extend_step(mxfp4) T 4 [yardstick: the bf16 skinny route]")


def test_generate_mxfp4_graph_equals_eager(golden_loss):
    from picotron_amd import generate as G
    m2, _, cfg, w = _mx_models(golden_loss, "gqa2")
    prompt = torch.randint(0, cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(23)).to(DEV)
    kw = dict(seed=5, skinny_linear=True, decode_weights=w, return_logits=True)
    te, le = G.generate(m2, prompt, 12, **kw)
    cache = G.KVCache(m2, 2, 32)
    tg, lg = G.generate(m2, prompt, 12, graph=True, cache=cache, **kw)
    assert torch.equal(tg, te) and torch.equal(lg, le)
    kw = dict(temperature=0.8, top_k=20, top_p=0.9, seed=7, skinny_linear=True, decode_weights=w)
    assert torch.equal(G.generate(m2, prompt, 12, graph=True, cache=cache, **kw), G.generate(m2, prompt, 12, **kw))
    assert cache.graph_captures == 1
