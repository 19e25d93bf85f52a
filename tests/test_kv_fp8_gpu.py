"""FP8 (e4m3) KV cache on the GPU: pico_kv_append_fp8 bit for bit against the bf16 append followed by the CPU
quantiser, pico_attn_decode_fp8 exactly on single live rows and against fp64 on scale * e4m3(code), and prefill /
decode_step / generate with an FP8 KVCache against a twin run with a bf16 cache."""
import pytest
import torch

from conftest import max_abs, rel_l2
from oracle import hotpath as H
from test_generate_gpu import _oracle_and_yardstick, _tiny

pytestmark = pytest.mark.gpu
BF, E4, U8 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8
DEV = "cuda"
O_REL, LSE_ABS = 4e-3, 2e-3  # the decode attention's bounds in tests/test_generate_gpu.py


def _quantised(rows):
    """ops.quantize_weight_fp8 on the CPU of bf16 head vectors [..., D]: (codes as uint8, scales)."""
    from picotron_amd import ops
    w = ops.quantize_weight_fp8(rows.detach().cpu().reshape(-1, rows.shape[-1]))
    return w.codes.view(U8).view(rows.shape), w.scale.view(rows.shape[:-1])


@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("D", [64, 128])
def test_append_equals_bf16_append_then_quantiser(D, T):
    """Layer 1 of a [3, ...] cache inside sentinel-filled larger tensors, per-row positions with p < 0 and p >= S_max:
    q, the in-place k, codes and scales against the bf16 twin; nothing outside the live rows changes."""
    from picotron_amd import generate as G
    B, Hq, Hkv, S, PAD = 4, 4, 2, 48, 8
    torch.manual_seed(D + T)
    qkv = torch.randn(B, T, (Hq + 2 * Hkv) * D, device=DEV).to(BF)
    x = qkv.view(B, T, Hq + 2 * Hkv, D)
    x[0, 0, Hq] = 0  # an all-zero k vector
    x[1, 0, Hq + Hkv, 3] = 1e4  # an outlier in a v vector
    x[2, 0, Hq + Hkv + 1] = torch.where(torch.arange(D, device=DEV) % 2 == 0, 0.75, -0.75).to(BF)  # equal magnitudes
    src, twin = qkv.clone().view(B, T, -1, D), qkv.clone()
    cos, sin = [t.to(DEV)[:, : D // 2] for t in H.get_cos_sin(64, D, 10000.0)]
    pos = [0, 5, S - 1, -3]
    pt = torch.tensor(pos, dtype=torch.int32, device=DEV)
    big = [torch.full((3, B, Hkv, S + 2 * PAD, D), 0x55, device=DEV, dtype=U8).view(E4) for _ in range(2)]
    bigs = [torch.full((3, B, Hkv, S + 2 * PAD), -7.0, device=DEV) for _ in range(2)]
    kc, vc = [t[1][:, :, PAD:PAD + S] for t in big]
    ksc, vsc = [t[1][:, :, PAD:PAD + S] for t in bigs]
    kb, vb = [torch.zeros(B, Hkv, S, D, device=DEV, dtype=BF) for _ in range(2)]
    q = G.kv_cache_append(qkv, cos, sin, pt, kc, vc, Hq, Hkv, k_scale=ksc, v_scale=vsc)
    q2 = G.kv_cache_append(twin, cos, sin, pt, kb, vb, Hq, Hkv)
    assert torch.equal(q, q2)
    assert torch.equal(x[:, :, Hq + Hkv:], src[:, :, Hq + Hkv:])  # v stays
    live = torch.zeros(3, B, Hkv, S + 2 * PAD, dtype=torch.bool)
    for b, p0 in enumerate(pos):
        lo = max(p0, 0)
        hi = max(min(p0 + T, S), lo)
        t0, t1 = lo - p0, hi - p0  # the tokens that fit
        assert torch.equal(x[b, t0:t1, Hq:Hq + Hkv], kb[b, :, lo:hi].transpose(0, 1)), (b, "k in place")
        keep = torch.ones(T, dtype=torch.bool)
        keep[t0:t1] = False
        assert torch.equal(x[b, keep], src[b, keep]), (b, "skipped tokens")
        for codes, scales, ref in ((kc, ksc, kb), (vc, vsc, vb)):
            wc, ws = _quantised(ref[b, :, lo:hi])
            assert torch.equal(codes[b, :, lo:hi].view(U8).cpu(), wc) and torch.equal(scales[b, :, lo:hi].cpu(), ws), b
        live[1, b, :, PAD + lo:PAD + hi] = True
    for t, s in zip(big, bigs):
        assert torch.equal(t.view(U8).cpu()[~live], torch.full((int((~live).sum()), D), 0x55, dtype=U8))
        assert (s.cpu()[~live] == -7.0).all()


@pytest.mark.parametrize("D", [64, 128])
def test_decode_converts_every_code_exactly(D):
    """One row carries all the weight (rows before it score -2^100 * 448: p = 0 exactly), so O is its v_scale *
    e4m3(code) and LSE its score. One-hot q: code i of the 254 finite codes at lane position i % D of K; V holds code
    (b D + d) % 254. The live row is row 0 (length 1), then one in every unroll slot, another lane group each."""
    from picotron_amd import generate as G
    B, Hq = 32, 8
    ng = 4 * 64 // (D // 8)
    finite = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=U8)
    idx = torch.arange(B * Hq)
    q = torch.zeros(B * Hq, D)
    q[idx, idx % D] = 1.0
    kcode = finite[idx % 254].view(B, Hq)
    vcode = finite[(torch.arange(B * D) % 254)].view(B, D)
    vscale = 2.0 ** ((torch.arange(B) % 7) - 3)
    kscale = 2.0 ** ((torch.arange(B) % 5) - 6)
    krow = torch.zeros(B * D, dtype=U8)
    krow[(idx // Hq) * D + idx % D] = kcode.view(-1)  # head h's one-hot position holds head h's code
    krow = krow.view(B, D)
    want_o = (vcode.view(E4).float() * vscale[:, None])[:, None, :].expand(B, Hq, D)
    want_l = kcode.view(E4).float() * kscale[:, None]
    for s in [0] + [j * ng + (5 * j + 1) % ng for j in range(8)]:
        k = torch.full((B, 1, s + 1, D), 0x7E, dtype=U8)  # 448 everywhere below the live row
        v = torch.full((B, 1, s + 1, D), 0x7E, dtype=U8)
        ks, vs = torch.full((B, 1, s + 1), -2.0 ** 100), torch.ones(B, 1, s + 1)
        k[:, 0, s], v[:, 0, s], ks[:, 0, s], vs[:, 0, s] = krow, vcode, kscale, vscale
        lens = torch.full((B,), s + 1, dtype=torch.int32, device=DEV)
        o, lse = G.attention_decode(q.view(B, Hq, D).to(BF).to(DEV), k.view(E4).to(DEV), v.view(E4).to(DEV), lens,
                                    softmax_scale=1.0, return_lse=True, k_scale=ks.to(DEV), v_scale=vs.to(DEV))
        assert torch.equal(o.float().cpu(), want_o), s
        rel = ((lse.cpu() - want_l).abs() / want_l.abs().clamp_min(1e-30)).max()
        assert float(rel) <= 1e-5, (s, float(rel))


_CASES = {}


def _case(Hq, Hkv, D, S=160, lens=(1, 31, 32, 33, 160)):
    """Random codes with moderate values and scales on the device, NaN codes and NaN scales beyond each length, and
    the fp64 result on scale * e4m3(code) (once per shape)."""
    key = (Hq, Hkv, D, S, lens)
    if key not in _CASES:
        from picotron_amd import generate as G
        B = len(lens)
        g = torch.Generator().manual_seed(Hq * 1000 + Hkv * 100 + D + S)
        q = torch.randn(B, Hq, D, generator=g).to(BF)
        k, v = [_quantised(torch.randn(B, Hkv, S, D, generator=g).to(BF))[0] for _ in range(2)]
        ks, vs = [torch.rand(B, Hkv, S, generator=g) * 0.008 + 0.004 for _ in range(2)]  # values of N(0, 1) size
        lt = torch.tensor(lens, dtype=torch.int32)
        ref = G.attention_decode(q.double(), k.view(E4), v.view(E4), lt, return_lse=True, k_scale=ks, v_scale=vs)
        for b, n in enumerate(lens):
            k[b, :, n:], v[b, :, n:] = 0x7F, 0xFF
            ks[b, :, n:] = vs[b, :, n:] = float("nan")
        _CASES[key] = ([t.to(DEV) for t in (q, k.view(E4), v.view(E4), lt)], dict(k_scale=ks.to(DEV), v_scale=vs.to(DEV)),
                       ref)
    return _CASES[key]


def _check(o, lse, ref):
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    e_o, e_l = rel_l2(o.cpu(), ref[0]), max_abs(lse.cpu(), ref[1])
    print(f"fp8 decode O rel-L2 {e_o:.3e} LSE max-abs {e_l:.3e}")
    assert e_o < O_REL and e_l < LSE_ABS, (e_o, e_l)
    for b in range(o.shape[0]):
        assert rel_l2(o[b].cpu(), ref[0][b]) < O_REL, b


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", [(4, 4), (4, 2), (6, 2), (8, 1)])
def test_decode_matches_fp64(heads, D):
    """Stale NaN codes and NaN scales lie beyond every length; two runs and row 1 of the batch alone give the same
    bits."""
    from picotron_amd import generate as G
    a, kw, ref = _case(*heads, D)
    o, lse = G.attention_decode(*a, split_keys=32, return_lse=True, **kw)
    assert o.dtype == BF and lse.dtype == torch.float32
    _check(o, lse, ref)
    o2, lse2 = G.attention_decode(*a, split_keys=32, return_lse=True, **kw)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    o1, lse1 = G.attention_decode(*[t[1:2] for t in a], split_keys=32, return_lse=True,
                                  **{n: t[1:2] for n, t in kw.items()})
    assert torch.equal(o1, o[1:2]) and torch.equal(lse1, lse[1:2])


@pytest.mark.parametrize("heads,D", [((4, 2), 64), ((8, 1), 128), ((5, 1), 64)])
def test_decode_default_split_and_zero_length(heads, D):
    from picotron_amd import generate as G
    a, kw, ref = _case(*heads, D, S=1024, lens=(0, 1000, 1))
    assert 256 <= G.default_split_keys(3, heads[1], 1024, D) < 1024
    o, lse = G.attention_decode(*a, return_lse=True, **kw)
    assert (o[0] == 0).all() and torch.isinf(lse[0]).all() and (lse[0] < 0).all()
    _check(o[1:], lse[1:], (ref[0][1:], ref[1][1:]))


def _assert_quantised_twin(c8, cb, layers, b, n):
    """Rows [0, n) of batch row b: the FP8 cache equals the CPU quantiser on the twin's bf16 cache, K and V."""
    for i in layers:
        for codes, scales, ref in ((c8.k, c8.k_scale, cb.k), (c8.v, c8.v_scale, cb.v)):
            wc, ws = _quantised(ref[i, b, :, :n])
            assert torch.equal(codes[i, b, :, :n].view(U8).cpu(), wc), (i, b)
            assert torch.equal(scales[i, b, :, :n].cpu(), ws), (i, b)


@pytest.mark.parametrize("kind", ["gqa2", "d128"])
def test_fp8_cache_against_bf16_twin(golden_loss, kind):
    """Bit-exact wiring against a bf16-cache twin, and the FP8-cache route's logit error against the fp32 oracle:
    e_fp8 <= 2 (yard + e_q), yard the existing model(input_ids) error on the same tokens, e_q the change of fp32 CPU
    logits when K / V pass through the CPU quantiser (never taken from the GPU route), 2 the project's margin for
    another summation order. Measured (MI355X): gqa2 e_fp8 7.5e-3, yard 6.7e-3, e_q 6.5e-3; d128 8.7e-3, 6.9e-3, 6.6e-3."""
    from picotron_amd import generate as G
    m, orc, cfg = _tiny(golden_loss, kind)
    g = torch.Generator().manual_seed(41)
    toks = torch.randint(0, cfg.vocab_size, (2, 26), generator=g).to(DEV)
    plens = [7, 4]
    prompt = toks[:, :7].clone()
    prompt[1, 4:] = 0
    c8, cb = G.KVCache(m, 2, 32, kv_dtype=E4), G.KVCache(m, 2, 32)
    l8, lb = G.prefill(m, prompt, c8, plens), G.prefill(m, prompt, cb, plens)
    assert torch.equal(l8, lb)  # the prompt is attended on the same bf16 K / V
    got = [l8]
    for b in range(2):
        _assert_quantised_twin(c8, cb, range(cfg.num_hidden_layers), b, plens[b])
    mode = torch.cuda.get_sync_debug_mode()
    for j in range(19):  # teacher-forced: layer 0's input is the embedding, whatever the cache
        nxt = torch.stack([toks[b, plens[b] + j] for b in range(2)])
        torch.cuda.set_sync_debug_mode("error" if j >= 2 else mode)  # past the first calls nothing synchronises
        try:
            l8 = G.decode_step(m, nxt, c8)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        lb = G.decode_step(m, nxt, cb)
        got.append(l8)
    assert torch.isfinite(l8).all() and c8.lens.tolist() == [26, 23]
    for b in range(2):
        _assert_quantised_twin(c8, cb, [0], b, plens[b] + 19)
    want, yard = _oracle_and_yardstick(m, orc, toks)
    got = torch.stack(got, 1).cpu()  # [2, 20, V]: positions plens[b] - 1 .. plens[b] + 18 of row b
    e_fp8 = e_q = e_loop = 0.0
    for b in range(2):
        sl = slice(plens[b] - 1, plens[b] + 19)
        exact, quant = [G.reference_logits(orc, toks[b].cpu(), cfg.num_attention_heads, cfg.num_key_value_heads,
                                           fp8_from)[sl] for fp8_from in (None, plens[b])]
        e_loop = max(e_loop, max_abs(exact, want[b, sl]))  # the CPU loop without the quantiser is the oracle
        e_q, e_fp8 = max(e_q, max_abs(quant, exact)), max(e_fp8, max_abs(got[b], want[b, sl]))
    print(f"{kind} e_fp8 {e_fp8:.3e} yard {yard[0]:.3e} e_q {e_q:.3e} (cpu loop vs oracle {e_loop:.1e})")
    assert e_loop < 1e-4 and e_fp8 <= 2 * (yard[0] + e_q), (e_fp8, yard[0], e_q)


@pytest.mark.parametrize("kind", ["gqa2", "d128"])
def test_generate_fp8_equals_manual_loop_and_graph(golden_loss, kind):
    from picotron_amd import generate as G
    m, _, cfg = _tiny(golden_loss, kind)
    prompt = torch.randint(0, cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(43)).to(DEV)
    N = 10
    toks, logits = G.generate(m, prompt, N, return_logits=True, kv_dtype=E4)
    cache = G.KVCache(m, 2, 24, kv_dtype=E4)
    lg = [G.prefill(m, prompt, cache)]
    for _ in range(N - 1):
        lg.append(G.decode_step(m, lg[-1].argmax(-1), cache))
    assert torch.equal(torch.stack(lg, 1), logits) and torch.equal(logits.argmax(-1), toks)
    tg, lgr = G.generate(m, prompt, N, return_logits=True, graph=True, cache=cache)  # captured, then replayed
    assert cache.graph_captures == 1 and torch.equal(tg, toks) and torch.equal(lgr, logits)
    tg, lgr = G.generate(m, prompt, N, return_logits=True, graph=True, cache=cache, kv_dtype=E4)  # replays only
    assert cache.graph_captures == 1 and torch.equal(tg, toks) and torch.equal(lgr, logits)
    kw = dict(return_logits=True, kv_dtype=E4, skinny_linear=True, decode_weights=G.quantize_decode_weights(m))
    (ts, ls), (tg, lgr) = G.generate(m, prompt, N, seed=1, **kw), G.generate(m, prompt, N, graph=True, **kw)
    assert torch.equal(ts, tg) and torch.equal(ls, lgr)  # skinny + FP8 weights on the FP8 cache: graph = eager
    with pytest.raises(ValueError, match="kv_dtype"):
        G.generate(m, prompt, N, cache=G.KVCache(m, 2, 24), kv_dtype=E4)
    # the default route is the parent's: the same kernels on a cache built without the argument
    t0, l0 = G.generate(m, prompt, N, return_logits=True)
    t1, l1 = G.generate(m, prompt, N, return_logits=True, cache=G.KVCache(m, 2, 24, kv_dtype=BF))
    assert torch.equal(t0, t1) and torch.equal(l0, l1)
