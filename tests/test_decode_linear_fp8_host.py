"""FP8 weight-only decode linear without a device: the plain-torch restatements of the row quantiser and of
ops.decode_linear(Fp8Weight) against fp64 (tests/decode_linear_ref.py's reference and bound on the dequantised
weight), the refusals, and the split rule. The cases here are the GPU file's too (it imports them)."""
import ctypes

import pytest
import torch

import decode_linear_ref as D

BF, E4M3 = torch.bfloat16, torch.float8_e4m3fn
QUANT_SHAPES = [(8, 64), (40, 320), (16, 2112)]
# (N, K, split_k): one step; a partial second block, a trip and a lone step, plain and cut 192 + 128; N = 8, two trips
# on wave 0 (the prefetch; unsplit); the rule's first split; more than one LDS slice (the rule cuts it in 4)
SHAPES = [(32, 64, 0), (40, 320, 0), (40, 320, 2), (8, 1280, 1), (32, 1024, 0), (40, 2112, 0)]
FORM_SHAPES = [(176, 320, 0), (272, 192, 2)]
FORMS = ["f32", "norm", "norm_res", "norm_res_noout"]
FINITE = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)  # the 254 finite e4m3 codes


def quant_input(N, K):
    """randn at K^-1/2; row 1 zeros, row 2 a single 1e4 outlier, row 3 equal magnitudes."""
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)) / K ** 0.5
    w[1] = 0
    w[2, K // 3] = 1e4
    w[3] = w[3].sign() * 0.37
    return w.to(BF)


def fp8_case(M, N, K):
    """D.inputs with the weight quantised on the CPU: (x, Fp8Weight, its exact fp64 value, norm_weight, residual)."""
    from picotron_amd import ops
    x, w, nw, res = D.inputs(M, N, K)
    q = ops.quantize_weight_fp8(w)
    return x, q, q.scale.double()[:, None] * q.codes.double(), nw, res


def one_hot_case(M, K):
    """(x, Fp8Weight, exact y): codes cycling through the 254 finite values, power-of-two scales, x rows one-hot at
    their own k: every lane group, both halves of a 16-byte load, an odd offset, (K > 64) the slice's last step."""
    from picotron_amd import ops
    N = 40
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    codes = FINITE[(k + 7 * n) % 254].view(E4M3)
    scale = 2.0 ** ((torch.arange(N) % 5) - 2).float()
    m = torch.arange(16)[16 - M:]
    ks = 16 * (m % 4) + 8 * ((m >> 2) & 1) + 5 * (m >> 3) + (K - 64) * (m & 1)
    x = torch.zeros(M, K)
    x[torch.arange(M), ks] = 1.0
    return x.to(BF), ops.Fp8Weight(codes, scale), scale[None, :] * codes.float()[:, ks].t()


def form_kwargs(form, nw, res):
    return dict(norm_weight=nw, residual=res if "res" in form else None) if "norm" in form else {}


@pytest.mark.parametrize("N,K", QUANT_SHAPES)
def test_quantiser_restatement(N, K):
    from picotron_amd import ops
    w = quant_input(N, K)
    q = ops.quantize_weight_fp8(w)
    bits, a = q.codes.view(torch.uint8), w.float().abs().amax(1)
    assert not bool((bits & 0x7f == 0x7f).any()) and q.shape == (N, K)
    assert torch.equal(q.scale, torch.where(a == 0, torch.ones_like(a), a / 448)) and q.scale[1] == 1
    assert int(bits[1].max()) == 0 and int(bits[2, K // 3]) == 0x7e and bool((bits[3] & 0x7f == 0x7e).all())
    # RNE: within half an e4m3 spacing (2^-3 relative to the binade, 2^-9 below 2^-6) of the fp64 quotient
    q64 = w.double() / q.scale.double()[:, None]
    half = torch.exp2(torch.floor(torch.log2(q64.abs().clamp(min=2.0 ** -6))) - 4)
    assert bool(((q.codes.double() - q64).abs() <= half * (1 + 2.0 ** -20)).all())
    both = ops.quantize_weight_fp8((w[:N // 2].clone(), w[N // 2:].clone()))  # the stacked view: the same rows
    assert torch.equal(both.codes.view(torch.uint8), bits) and torch.equal(both.scale, q.scale)


@pytest.mark.parametrize("M", [1, 16])
@pytest.mark.parametrize("K", [64, 320])
def test_restatement_one_hot_is_exact(M, K):
    from picotron_amd import ops
    x, q, want = one_hot_case(M, K)
    assert torch.equal(ops.decode_linear(x, q).float(), want)


@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("form,N,K", [("bf16", n, k) for n, k, s in SHAPES if s != 2] +
                         [(f, *FORM_SHAPES[0][:2]) for f in FORMS[:3]])
def test_restatement_matches_fp64(form, M, N, K):
    from picotron_amd import ops
    x, q, w64, nw, res = fp8_case(M, N, K)
    kw = form_kwargs(form, nw, res)
    out = ops.decode_linear(x, q, out_dtype=torch.float32 if form == "f32" else None, **kw)
    y, ro = out if "norm" in form else (out, None)
    D.check(f"host fp8 {form} {M}x{N}x{K}", {"y": y, "residual_out": ro if "res" in form else None},
            D.reference(x, w64, **kw))


def test_refusals():
    from picotron_amd import _lib, generate as G, ops
    from picotron_amd.model import LlamaConfig, build_llama
    x, q, _, nw, res = fp8_case(4, 32, 64)
    with pytest.raises(ValueError, match="1..16"):
        ops.decode_linear(torch.zeros(17, 64, dtype=BF), q)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.decode_linear(x[:, :32], ops.Fp8Weight(q.codes[:, :32], q.scale))
    with pytest.raises(ValueError, match="norm prologue"):
        ops.decode_linear(x, q, residual=res)
    assert _lib.load().pico_decode_linear_fp8_args_size() == ctypes.sizeof(_lib.DecodeLinearFp8Args)
    cfg = dict(hidden_size=64, intermediate_size=128, num_attention_heads=1, num_key_value_heads=1,
               num_hidden_layers=1, vocab_size=64, max_position_embeddings=32)
    m = build_llama(LlamaConfig(**cfg), device="cpu", dtype=BF)
    w, tok = G.quantize_decode_weights(m), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="skinny_linear"):
        G.decode_step(m, tok, None, decode_weights=w)
    with pytest.raises(ValueError, match="skinny_linear"):
        G.generate(m, tok[None], 2, decode_weights=w)
    other = build_llama(LlamaConfig(**{**cfg, "intermediate_size": 192}), device="cpu", dtype=BF)
    with pytest.raises(ValueError, match="does not fit"):
        G.decode_step(other, tok, None, skinny_linear=True, decode_weights=w)
    narrow = build_llama(LlamaConfig(**{**cfg, "intermediate_size": 96}), device="cpu", dtype=BF)
    with pytest.raises(ValueError, match="K = 96"):
        G.decode_step(narrow, tok, None, skinny_linear=True, decode_weights=G.quantize_decode_weights(narrow))


@pytest.mark.parametrize("epi", [0, 2])
def test_split_rule(epi):
    """Slices are multiples of 64 that cover K and fit LDS; the workspace covers the partials; M enters it alone."""
    from picotron_amd import _lib
    lib, p, p1 = _lib.load(), (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
    for N in (16, 48, 2048, 6144, 49152):
        for K in (64, 448, 512, 1024, 2048, 2112, 8192):
            for cus in (1, 64, 256, 304):
                assert lib.pico_decode_linear_fp8_plan(16, N, K, epi, 0, cus, p) == 0
                assert lib.pico_decode_linear_fp8_plan(1, N, K, epi, 0, cus, p1) == 0
                blocks, sk, ks, nbytes = p
                assert list(p1)[:3] == [blocks, sk, ks] and blocks == -(-N // 32)
                assert ks % 64 == 0 and ks <= 2048 and (sk - 1) * ks < K <= sk * ks
                assert nbytes >= sk * 16 * N * 4 if sk > 1 else nbytes == 0
                assert sk == 1 or ks >= 512
    assert lib.pico_decode_linear_fp8_plan(1, 2048, 2048, 0, 0, 256, p) == 0 and list(p)[:3] == [64, 4, 512]
    assert lib.pico_decode_linear_fp8_plan(1, 32, 8192, 0, 3, 256, p) == 1000  # slices of 2752 columns do not fit
