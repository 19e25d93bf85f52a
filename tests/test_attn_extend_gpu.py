"""pico_attn_extend (csrc/attn_extend.hip) against the fp64 reference under the project's per-row decode bound, its
staircase mask, determinism, row independence and guard bands; extend_step / KVCache.rewind against the fp32 oracle."""
import math

import pytest
import torch

import attn_ref as A
import split_ref as SR
import test_generate_gpu as TG

pytestmark = pytest.mark.gpu
BF, DEV = torch.bfloat16, "cuda"
HKV, S_MAX, SPLIT = 2, 3 * 128 + 21, 160  # three workgroup trips and a bit; chunks of 160, 160, 85 keys
ROWS = [(1, 1), (16, 1), (4, 4), (6, 3), (4, 8), (5, 8), (16, 3), (16, 8)]  # (T, G)


def _lens(T, split):
    """One batch row per length: fresh cache, fewer keys than tokens, a staircase across a 16-key tile edge, a 32-key
    step edge and a chunk edge, one past a trip, the full cache, beyond it (clamped)."""
    h = max(1, T // 2)
    return (T, T // 2, 16 + h, 32 + h, split + h, 129, S_MAX, S_MAX + 5)


def _case(D, T, G_, split, lens=None, v_fill=None, seed=0):
    """bf16 inputs on the CPU (cache rows at and beyond each length are NaN), the fp64 reference and the bf16
    restatement with the same split_keys. v_fill: the V rows of the later new tokens ([query 0's limit, length))."""
    from picotron_amd import generate as GEN
    lens = _lens(T, split) if lens is None else lens
    gen = torch.Generator().manual_seed(seed * 7919 + D * 131 + T * 17 + G_)
    B, Hq = len(lens), HKV * G_
    qkv = torch.randn(B, T, (Hq + 2 * HKV) * D, generator=gen).to(BF)
    kv = torch.randn(2, 2, B, HKV, S_MAX, D, generator=gen).to(BF)  # (k | v) x layers
    for b, n in enumerate(lens):
        n = min(max(n, 0), S_MAX)
        kv[:, :, b, :, n:] = math.nan
        if v_fill is not None:
            kv[1, :, b, :, min(max(lens[b] - (T - 1), 0), S_MAX):n] = v_fill
    sl = torch.tensor(lens, dtype=torch.int32)
    q, k, v = qkv.view(B, T, Hq + 2 * HKV, D)[:, :, :Hq], kv[0, 1], kv[1, 1]
    scale = 1.0 / math.sqrt(D)
    o_ref, l_ref = GEN.attention_extend(q.double(), k.double(), v.double(), sl, scale, None, True)
    o_emul, _ = GEN.attention_extend(q, k, v, sl, scale, split, True)
    return {"qkv": qkv, "kv": kv, "lens": sl, "scale": scale, "o_ref": o_ref, "l_ref": l_ref, "o_emul": o_emul,
            "shape": (B, T, Hq, D)}


def _device_views(c):
    B, T, Hq, D = c["shape"]
    qkv, kv = c["qkv"].to(DEV), c["kv"].to(DEV)
    return qkv.view(B, T, Hq + 2 * HKV, D)[:, :, :Hq], kv[0, 1], kv[1, 1], c["lens"].to(DEV)


def _check(tag, o, lse, c, rows=slice(None)):
    """Per query row: ||O - ref|| <= M_ROW ||restated - ref|| + BF16_RN ||ref||, |LSE - ref| <= LSE_TOL, all finite;
    rows without a visible key: O = 0, LSE = -inf exactly. rows: the queries (t index) that are checked."""
    o, lse = o.cpu()[:, rows], lse.cpu()[:, rows]
    O, L, E = c["o_ref"][:, rows], c["l_ref"][:, rows], c["o_emul"][:, rows]
    empty = torch.isinf(L) & (L < 0)
    err = (o.double() - O).norm(dim=-1)
    bound = SR.M_ROW * (E.double() - O).norm(dim=-1) + A.BF16_RN * O.norm(dim=-1)
    dl = (lse.double() - L)[~empty].abs().max()
    print(f"EXTEND {tag}: worst O err / bound {float((err / bound.clamp_min(1e-300))[~empty].max()):.3g}, "
          f"LSE max-abs {float(dl):.3g}")
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse[~empty]).all())
    assert bool((o[empty] == 0).all()) and bool((lse[empty] == -math.inf).all())
    assert bool((err <= bound).all()), (tag, float((err - bound).max()))
    assert float(dl) <= A.LSE_TOL, (tag, float(dl))


@pytest.mark.parametrize("T,G_", ROWS)
@pytest.mark.parametrize("D", [64, 128])
def test_extend_matches_fp64(D, T, G_):
    from picotron_amd import generate as GEN
    c = _case(D, T, G_, SPLIT)
    q, k, v, sl = _device_views(c)
    o, lse = GEN.attention_extend(q, k, v, sl, split_keys=SPLIT, return_lse=True)
    _check(f"D {D} T {T} G {G_} split {SPLIT}", o, lse, c)


def test_extend_default_split():
    from picotron_amd import generate as GEN
    D, T, G_ = 64, 6, 3
    split = GEN.default_extend_split_keys(8, T, HKV * G_, HKV, S_MAX, D)
    assert split >= 256 and split % 128 == 0
    c = _case(D, T, G_, split)
    q, k, v, sl = _device_views(c)
    o, lse = GEN.attention_extend(q, k, v, sl, return_lse=True)
    _check(f"D {D} T {T} G {G_} default split {split}", o, lse, c)


@pytest.mark.parametrize("D,T,G_", [(64, 4, 4), (128, 16, 8)])
def test_extend_staircase_does_not_leak(D, T, G_):
    """The later new tokens' V rows hold 1e4 (finite: they are live for the later queries): query 0 must not see them."""
    from picotron_amd import generate as GEN
    c = _case(D, T, G_, SPLIT, v_fill=1e4)
    q, k, v, sl = _device_views(c)
    o, lse = GEN.attention_extend(q, k, v, sl, split_keys=SPLIT, return_lse=True)
    assert float(c["o_ref"][:, 0].abs().max()) < 10 < float(c["o_ref"][:, 1:].abs().max())
    _check(f"leak D {D} T {T} G {G_}", o, lse, c, rows=slice(0, 1))


def _launch(c, rows=slice(None)):
    """pico_attn_extend through the C ABI on batch rows `rows`, with O, LSE and the workspace inside guard bands."""
    from picotron_amd import _lib as L
    lib = L.load()
    q, k, v, sl = (t[rows] for t in _device_views(c))
    sl = sl.contiguous()
    B, T, Hq, D = q.shape
    Gd = A.Guards(DEV)
    o = Gd.mat("o", B * T * Hq, D)
    lse = Gd.flat("lse", B * T * Hq, torch.float32)
    nbytes = int(lib.pico_attn_extend_workspace_bytes(B, T, Hq, HKV, S_MAX, D, SPLIT))
    assert nbytes > 0, lib.pico_last_error()
    ws = Gd.flat("workspace", nbytes, torch.uint8)
    Gd.arm()
    L.check(lib.pico_attn_extend(L.ptr(q), L.i64x3(q.stride()[:3]), L.ptr(k), L.i64x3(k.stride()[:3]), L.ptr(v),
                                 L.i64x3(v.stride()[:3]), L.ptr(sl), L.ptr(o), L.ptr(lse), L.ptr(ws), B,
                                 T, Hq, HKV, S_MAX, D, c["scale"], SPLIT, L.stream_of(q)), "pico_attn_extend")
    torch.cuda.synchronize()
    Gd.check()
    return o.view(B, T, Hq, D).view(torch.int16), lse.view(B, T, Hq)


@pytest.mark.parametrize("D,T,G_", [(64, 6, 3), (128, 5, 8)])
def test_extend_is_deterministic_and_row_independent(D, T, G_):
    c = _case(D, T, G_, SPLIT, lens=(SPLIT + 2, 3, S_MAX))
    o, lse = _launch(c)
    o2, lse2 = _launch(c)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    for b in range(3):
        ob, lb = _launch(c, slice(b, b + 1))
        assert torch.equal(ob[0], o[b]) and torch.equal(lb[0], lse[b]), b


@pytest.mark.parametrize("kind,route", [("gqa2", "default"), ("d128", "default"), ("gqa2", "skinny"), ("gqa2", "fp8w")])
def test_extend_step_matches_oracle(golden_loss, kind, route):
    """prefill (ragged 5 and 3), five extend_steps of the 4 true next tokens, a step of two true and two wrong tokens,
    rewind(2), the true ones; then T = 1 beside decode_step on a copy of the cache. Every kept position within 2x the
    error of model(input_ids) against the fp32 oracle (fp8w: the oracle on the dequantised weights)."""
    from picotron_amd import generate as GEN
    kw = {}
    if route == "fp8w":
        from test_decode_linear_fp8_gpu import _fp8_models
        m, orc, cfg, w = _fp8_models(golden_loss, kind)
        kw = dict(skinny_linear=True, decode_weights=w)
    else:
        m, orc, cfg = TG._tiny(golden_loss, kind)
        kw = dict(skinny_linear=route == "skinny")
    toks = torch.randint(0, cfg.vocab_size, (2, 48), generator=torch.Generator().manual_seed(17)).to(DEV)
    want, yard = TG._oracle_and_yardstick(m, orc, toks)
    pos = [5, 3]
    prompt = toks[:, :5].clone()
    prompt[1, 3:] = 0
    cache = GEN.KVCache(m, 2, 64)
    GEN.prefill(m, prompt, cache, pos)
    got, ref = [], []

    def step(T, keep, spoil=False):
        tk = torch.stack([toks[b, pos[b]:pos[b] + T] for b in range(2)])
        if spoil:
            tk[:, keep:] = (tk[:, keep:] + 1) % cfg.vocab_size
        lg = GEN.extend_step(m, tk, cache, **kw)
        assert lg.dtype == torch.float32 and lg.shape == (2, T, cfg.vocab_size)
        got.append(lg[:, :keep].cpu())
        ref.append(torch.stack([want[b, pos[b]:pos[b] + keep] for b in range(2)]))
        for b in range(2):
            pos[b] += keep

    for _ in range(5):
        step(4, 4)
    assert cache.lens.tolist() == [25, 23]
    step(4, 2, spoil=True)
    assert cache.lens.tolist() == [29, 27]
    cache.rewind(2)
    assert cache.lens.tolist() == pos == [27, 25]
    step(4, 4)
    TG._within(torch.cat(got, 1), torch.cat(ref, 1), yard, f"{kind} {route} extend_step")
    twin = GEN.KVCache(m, 2, 64)
    twin.k.copy_(cache.k), twin.v.copy_(cache.v), twin.lens.copy_(cache.lens)
    nxt = torch.stack([toks[b, pos[b]] for b in range(2)])
    one = torch.stack([want[b, pos[b]] for b in range(2)])
    TG._within(GEN.extend_step(m, nxt[:, None], cache, **kw)[:, 0].cpu(), one, yard, f"{kind} {route} extend_step T 1")
    TG._within(GEN.decode_step(m, nxt, twin, **kw).cpu(), one, yard, f"{kind} {route} decode_step")
