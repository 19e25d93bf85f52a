"""MXFP4 weight-only decode linear without a device: the plain-torch restatements of the block quantiser and of
ops.decode_linear(Mxfp4Weight) against fp64 (tests/decode_linear_ref.py on the dequantised weight), the refusals and
the split rule. The GPU file imports the cases. A K step is 128 columns, a trip 512; a slice holds at most 2048, so
no wave takes two trips of a slice (N = 8 runs four trips on four waves instead)."""
import ctypes

import pytest
import torch

import decode_linear_ref as D
from test_decode_linear_fp8_host import form_kwargs

BF = torch.bfloat16
QUANT_SHAPES = [(8, 32), (40, 320), (16, 2112)]
# (N, K, split_k): one step; a partial second block, a trip and a lone step, plain and cut 384 + 256; N = 8, four
# trips (unsplit); the rule's first split (2 x 1024); just past one LDS slice (the rule cuts 1152 + 1024)
SHAPES = [(32, 128, 0), (40, 640, 0), (40, 640, 2), (8, 2048, 1), (32, 2048, 0), (40, 2176, 0)]
FORM_SHAPES = [(176, 640, 0), (272, 384, 2)]
FORMS = ["f32", "norm", "norm_res", "norm_res_noout"]
MID = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0])  # the e2m1 midpoints and the top of the grid


def quant_input(N, K):
    """randn at K^-1/2; the first block of rows 1..6: zeros, a 1e4 outlier, equal magnitudes, 0..7 times 2^-3 (absmax
    7 * 2^-3: 5 ties to 4, 7 saturates at 6), the midpoints times 8 (ties to even), bf16 denormals (the clamp)."""
    w = (torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)) / K ** 0.5).to(BF)
    sign = 1.0 - 2.0 * (torch.arange(32) // 8 % 2)
    w[1, :32] = 0
    w[2, 11] = 1e4
    w[3, :32] = w[3, :32].sign() * 0.37
    w[4, :32] = (torch.arange(32) % 8 / 8 * sign).to(BF)
    w[5, :32] = (MID.repeat(4) * 8 * sign).to(BF)
    w[6, :32] = (torch.arange(1, 33) * 4 - 1 - 32768 * (sign < 0)).to(torch.int16).view(BF)  # bits 3 .. 127, signed
    return w


def mx_case(M, N, K):
    """D.inputs with the weight quantised on the CPU: (x, Mxfp4Weight, its exact fp64 value, norm_weight, residual)."""
    from picotron_amd import ops
    x, w, nw, res = D.inputs(M, N, K)
    q = ops.quantize_weight_mxfp4(w)
    return x, q, q.dequantize(torch.float64), nw, res


def one_hot_case(M, K):
    """(x, Mxfp4Weight, exact y): row n holds code (k + 3 n) mod 16 at column k, so every code sits at every nibble;
    scale bytes differ per block; x rows are one-hot at their own k: every lane group and dword of a 16-byte load,
    both nibbles, (K > 128) the slice's last step."""
    from picotron_amd import ops
    N = 40
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    c = (k + 3 * n) % 16
    codes = (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8)
    scales = (125 + (n + torch.arange(K // 32)[None, :]) % 5).to(torch.uint8)
    q = ops.Mxfp4Weight(codes, scales)
    m = torch.arange(16)[16 - M:]
    ks = 32 * (m % 4) + 8 * ((m >> 2) & 3) + (3 * m + 1) % 8 + (K - 128) * (m & 1)
    x = torch.zeros(M, K)
    x[torch.arange(M), ks] = 1.0
    return x.to(BF), q, q.dequantize()[:, ks].t().contiguous()


@pytest.mark.parametrize("N,K", QUANT_SHAPES)
def test_quantiser_restatement(N, K):
    from picotron_amd import ops
    w = quant_input(N, K)
    q = ops.quantize_weight_mxfp4(w)
    assert q.shape == (N, K) and q.codes.shape == (N, K // 2) and q.scales.shape == (N, K // 32)
    assert int(q.scales.min()) >= 7 and int(q.scales.max()) <= 252
    e = q.scales.int().repeat_interleave(32, 1) - 127
    v, dq = torch.ldexp(w.double(), -e), torch.ldexp(q.dequantize(torch.float64), -e)  # in units of the block's 2^e
    assert torch.equal(q.dequantize(BF).double(), q.dequantize(torch.float64))  # exactly bf16 values
    half = torch.where(v.abs() < 2, 0.25, torch.where(v.abs() < 4, 0.5, 1.0))  # half an e2m1 step at |v|
    assert bool((((dq - v).abs() <= half) | ((v.abs() > 6) & (dq == 6 * v.sign()))).all())
    # the OCP exponent: the block's absmax lands in [4, 8) 2^e unless the clamp holds it below (a zero block: e = 0)
    a = v.abs().view(N, -1, 32).amax(-1)
    assert bool(((a >= 4) & (a < 8) | (q.scales == 7) & (a < 4) | (q.scales == 127) & (a == 0)).all())
    mag = torch.stack((q.codes & 7, (q.codes >> 4) & 7), -1).flatten(1)[:, :32]
    assert int(q.scales[1, 0]) == 127 and int(q.codes[1, :16].max()) == 0
    assert int(mag[2, 11]) == 6 and int(q.scales[2, 0]) == 127 + 13 - 2  # 1e4 -> 9984 = 4.875 * 2^11 -> 4
    assert bool((mag[3] == 7).all())  # equal magnitudes: 0.369 = 5.9 * 2^-4 -> 6, every one
    assert mag[4].tolist() == [0, 2, 4, 5, 6, 6, 7, 7] * 4 and int(q.scales[4, 0]) == 124
    assert mag[5].tolist() == [0, 2, 2, 4, 4, 6, 6, 7] * 4 and int(q.scales[5, 0]) == 130
    assert int(q.scales[6, 0]) == 7 and int(mag[6].max()) == 0
    both = ops.quantize_weight_mxfp4((w[:N // 2].clone(), w[N // 2:].clone()))  # the stacked view: the same rows
    assert torch.equal(both.codes, q.codes) and torch.equal(both.scales, q.scales)


@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("form,N,K", [("bf16", n, k) for n, k, s in SHAPES if s != 2] +
                         [(f, *FORM_SHAPES[0][:2]) for f in FORMS[:3]])
def test_restatement_matches_fp64(form, M, N, K):
    from picotron_amd import ops
    x, q, w64, nw, res = mx_case(M, N, K)
    kw = form_kwargs(form, nw, res)
    out = ops.decode_linear(x, q, out_dtype=torch.float32 if form == "f32" else None, **kw)
    y, ro = out if "norm" in form else (out, None)
    D.check(f"host mxfp4 {form} {M}x{N}x{K}", {"y": y, "residual_out": ro if "res" in form else None},
            D.reference(x, w64, **kw))


def test_refusals():
    from picotron_amd import _lib, generate as G, ops
    from picotron_amd.model import LlamaConfig, build_llama
    x, q, _, nw, res = mx_case(4, 32, 128)
    with pytest.raises(ValueError, match="1..16"):
        ops.decode_linear(torch.zeros(17, 128, dtype=BF), q)
    with pytest.raises(ValueError, match="multiple of 128"):
        ops.decode_linear(x[:, :64], ops.Mxfp4Weight(q.codes[:, :32], q.scales[:, :2]))
    with pytest.raises(ValueError, match="norm prologue"):
        ops.decode_linear(x, q, residual=res)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.quantize_weight_mxfp4(torch.zeros(8, 48, dtype=BF))
    assert _lib.load().pico_decode_linear_mxfp4_args_size() == ctypes.sizeof(_lib.DecodeLinearMxfp4Args)
    cfg = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_key_value_heads=1,
               num_hidden_layers=1, vocab_size=64, max_position_embeddings=32)
    m = build_llama(LlamaConfig(**cfg), device="cpu", dtype=BF)
    tok = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="fmt"):
        G.quantize_decode_weights(m, fmt="fp4")
    for w in (G.quantize_decode_weights(m, fmt="mxfp4"), G.quantize_decode_weights(m)):
        with pytest.raises(ValueError, match="skinny_linear"):
            G.decode_step(m, tok, None, decode_weights=w)
        with pytest.raises(ValueError, match="skinny_linear"):
            G.generate(m, tok[None], 2, decode_weights=w)
    assert w.fmt == "fp8" and G.quantize_decode_weights(m, fmt="mxfp4").fmt == "mxfp4"
    other = build_llama(LlamaConfig(**{**cfg, "intermediate_size": 384}), device="cpu", dtype=BF)
    with pytest.raises(ValueError, match="does not fit"):
        G.decode_step(other, tok, None, skinny_linear=True, decode_weights=G.quantize_decode_weights(m, fmt="mxfp4"))
    narrow = build_llama(LlamaConfig(**{**cfg, "intermediate_size": 192}), device="cpu", dtype=BF)
    with pytest.raises(ValueError, match="multiple of 128.*K = 192"):
        G.decode_step(narrow, tok, None, skinny_linear=True,
                      decode_weights=G.quantize_decode_weights(narrow, fmt="mxfp4"))


@pytest.mark.parametrize("epi", [0, 2])
def test_split_rule(epi):
    """Slices are multiples of 128 that cover K and fit LDS; the workspace covers the partials; M enters it alone."""
    from picotron_amd import _lib
    lib, p, p1 = _lib.load(), (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
    for N in (16, 48, 2048, 6144, 49152):
        for K in (128, 896, 1024, 2048, 2176, 8192):
            for cus in (1, 64, 256, 304):
                assert lib.pico_decode_linear_mxfp4_plan(16, N, K, epi, 0, cus, p) == 0
                assert lib.pico_decode_linear_mxfp4_plan(1, N, K, epi, 0, cus, p1) == 0
                blocks, sk, ks, nbytes = p
                assert list(p1)[:3] == [blocks, sk, ks] and blocks == -(-N // 32)
                assert ks % 128 == 0 and ks <= 2048 and (sk - 1) * ks < K <= sk * ks
                assert nbytes >= sk * 16 * N * 4 if sk > 1 else nbytes == 0
                assert sk == 1 or ks >= 1024
    assert lib.pico_decode_linear_mxfp4_plan(1, 2048, 2048, 0, 0, 256, p) == 0 and list(p)[:3] == [64, 2, 1024]
    assert lib.pico_decode_linear_mxfp4_plan(1, 32, 8192, 0, 3, 256, p) == 1000  # slices of 2816 columns do not fit
    assert lib.pico_decode_linear_mxfp4_plan(1, 32, 192, 0, 0, 256, p) == 1000 and b"128" in lib.pico_last_error()
