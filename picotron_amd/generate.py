"""KV-cache generation: prefill, single-token decode steps, sampling.

Two gfx950 kernels carry it (include/picotron_hip.h): `pico_kv_append` (RoPE on q in place, rotated k and v into a
head-major cache, positions read from the device) and `pico_attn_decode` (one query per sequence, split over the
keys, all query heads of a kv head in one workgroup). Everything else is what training already runs: hipBLASLt
projections against the stacked weights, `ops.rms_norm` in its residual form, `ops.swiglu`, and for the prompt the
causal forward attention kernel reading K / V out of the cache through its strides. Nothing here goes through the
training wrappers: no y^T / O^T by-products, no weight-gradient hints, no autograd graph.

`kv_cache_append` and `attention_decode` call the kernels for HIP bf16 tensors; for CPU tensors of any float dtype
they run a plain-torch restatement of the same contract (fp32 arithmetic, fp64 for fp64 inputs, the kernels'
rounding points), which is the reference the tests compare the kernels with. A HIP tensor of another dtype is an
error: there is no eager path on the device.

A decode step performs no host synchronisation: positions and lengths live on the device, shapes are fixed.

An FP8 cache (`KVCache(..., kv_dtype=torch.float8_e4m3fn)`: e4m3 codes plus one fp32 scale per cached head vector)
takes `pico_kv_append_fp8` (the same rotation; k stays in qkv as bf16 and is quantised into the cache, v is quantised)
and `pico_attn_decode_fp8` (the same split, half the bytes per key); both ops dispatch on the cache's dtype.

`extend_step` runs T <= 16 tokens per row in one pass over the weights (verifying drafted tokens, continuing a cached
conversation, scoring against a long cache): `kv_cache_append` with T tokens, then `attention_extend`
(`pico_attn_extend`: the T x Hq / Hkv query rows of a kv head on the matrix unit, split over the keys like the decode
kernel, bf16 caches only). `KVCache.rewind` takes rejected tokens back on the device.

`quantize_decode_weights(model, fmt)` snapshots the decode projections for `skinny_linear=True`: `fmt="fp8"` (e4m3
codes, one fp32 scale per output row, `pico_decode_linear_fp8`) or `fmt="mxfp4"` (OCP e2m1 codes with one E8M0 scale
byte per 32 columns, 4.25 bits per weight, `pico_decode_linear_mxfp4`); `decode_step`, `extend_step` and `generate`
read either through `ops.decode_linear`.

`sample_tokens` is the fused sampler (`pico_sample`: temperature, top-k, top-p, a Philox draw, the EOS / pad rule
and the output column in one launch, every per-step value in a `SamplerState` on the device); with it a whole
iteration, decode step and sampler, is captured once as a HIP graph and replayed per token (`generate(graph=True)`).
"""
import math
import os
import struct

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from . import process_group_manager as pgm

_E4M3 = torch.float8_e4m3fn
MAX_GROUP = 8  # query heads per kv head the decode kernel serves (csrc/attn_decode_plan.h DEC_MAX_GROUP)
MAX_EXTEND_TOKENS = 16  # new tokens per row the extend kernel serves (csrc/attn_extend_plan.h EXT_MAX_TOKENS)


def _check_caches(k_cache, v_cache, B, D):
    for t, n in ((k_cache, "k_cache"), (v_cache, "v_cache")):
        if t.dim() != 4 or t.stride(-1) != 1:
            raise ValueError(f"{n} must be [batch, kv_heads, max_len, head_dim] with unit last stride")
    if k_cache.shape != v_cache.shape or k_cache.shape[0] != B or k_cache.shape[3] != D:
        raise ValueError(f"cache shapes {tuple(k_cache.shape)} / {tuple(v_cache.shape)} do not fit batch {B}, "
                         f"head_dim {D}")


def _check_scales(who, k_cache, v_cache, k_scale, v_scale, dev):
    """True for an FP8 cache (e4m3 codes with its two scale tensors [B, Hkv, S_max] fp32); False for a plain one. A
    cache of one kind with the other's arguments is refused."""
    fp8 = k_cache.dtype == _E4M3 or v_cache.dtype == _E4M3
    if not fp8:
        if k_scale is not None or v_scale is not None:
            raise ValueError(f"{who}: k_scale / v_scale belong to an FP8 (float8_e4m3fn) cache, got {k_cache.dtype}")
        return False
    if k_cache.dtype != v_cache.dtype:
        raise ValueError(f"{who}: k_cache is {k_cache.dtype}, v_cache {v_cache.dtype}")
    if k_scale is None or v_scale is None:
        raise ValueError(f"{who}: an FP8 cache needs k_scale and v_scale (one fp32 scale per cached head vector)")
    for t, c, n in ((k_scale, k_cache, "k_scale"), (v_scale, v_cache, "v_scale")):
        if not isinstance(t, torch.Tensor) or t.shape != c.shape[:3] or t.dtype != torch.float32:
            raise ValueError(f"{who}: {n} must be fp32 [batch, kv_heads, max_len] = {tuple(c.shape[:3])}")
        if t.device != c.device or c.device != dev:
            raise ValueError(f"{who}: {n} on {t.device}, its cache on {c.device}, the input on {dev}")
    return True


def _compute_dtype(t):
    return torch.float64 if t.dtype == torch.float64 else torch.float32


# --------------------------------------------------------------------------------------------
# RoPE + cache append
# --------------------------------------------------------------------------------------------
def _kv_append_reference(qkv, cos, sin, pos, k_cache, v_cache, Hq, Hkv):
    B, T = qkv.shape[:2]
    D = k_cache.shape[3]
    S = k_cache.shape[2]
    ct = _compute_dtype(qkv)
    limit = min(S, cos.shape[0])
    x = qkv.view(B, T, Hq + 2 * Hkv, D)
    for b in range(B):
        p = int(pos[b]) + torch.arange(T)
        ok = (p >= 0) & (p < limit)
        if not bool(ok.any()):
            continue
        p = p[ok]
        c = cos[p, : D // 2].to(ct)[:, None, :]
        s = sin[p, : D // 2].to(ct)[:, None, :]
        xb, kb, vb = x[b], k_cache[b], v_cache[b]
        tok = ok.nonzero().flatten()
        xr = xb[tok, : Hq + Hkv].to(ct)
        x1, x2 = xr[..., : D // 2], xr[..., D // 2:]
        rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(qkv.dtype)  # one rounding, as pico_rope
        xb[tok, :Hq] = rot[:, :Hq]
        kb[:, p] = rot[:, Hq:].transpose(0, 1).to(k_cache.dtype)
        vb[:, p] = xb[tok, Hq + Hkv:].transpose(0, 1).to(v_cache.dtype)


def _kv_append_fp8_reference(qkv, cos, sin, pos, k_cache, v_cache, k_scale, v_scale, Hq, Hkv):
    """The reference above into caches of qkv's dtype, the rotated k put back in place in qkv, then the quantiser on
    the written head vectors."""
    B, T = qkv.shape[:2]
    D, S = k_cache.shape[3], k_cache.shape[2]
    tk = torch.zeros(k_cache.shape, dtype=qkv.dtype)
    tv = torch.zeros(v_cache.shape, dtype=qkv.dtype)
    _kv_append_reference(qkv, cos, sin, pos, tk, tv, Hq, Hkv)
    x = qkv.view(B, T, Hq + 2 * Hkv, D)
    kb, vb = k_cache.view(torch.uint8), v_cache.view(torch.uint8)
    for b in range(B):
        p = int(pos[b]) + torch.arange(T)
        ok = (p >= 0) & (p < min(S, cos.shape[0]))
        tok, p = ok.nonzero().flatten(), p[ok]
        if p.numel() == 0:
            continue
        x[b][tok, Hq:Hq + Hkv] = tk[b][:, p].transpose(0, 1)
        for src, codes, scales in ((tk, kb, k_scale), (tv, vb, v_scale)):
            c, scales[b][:, p] = ops._quantize_rows_cpu(src[b][:, p].float())  # ops.quantize_weight_fp8's CPU path
            codes[b][:, p] = c.view(torch.uint8)


def kv_cache_append(qkv, cos, sin, pos, k_cache, v_cache, num_heads, num_kv_heads, k_scale=None, v_scale=None):
    """RoPE + KV-cache write for the fused q|k|v projection output `qkv` [B, T, (Hq + 2 Hkv) D].

    With p = pos[b] + t (pos: int32 [B] on qkv's device): q[b, t] is rotated IN PLACE with row p of cos / sin
    ([rows, >= D/2] tables), k[b, t] is rotated with row p and stored at k_cache[b, :, p, :], v[b, t] is copied to
    v_cache[b, :, p, :]. Caches are [B, Hkv, S_max, D] views (unit last stride, other strides multiples of 8). A
    token with p >= S_max, or beyond the tables, is skipped whole. Returns the q view [B, T, Hq, D] of qkv.

    FP8 caches (torch.float8_e4m3fn codes, with k_scale / v_scale fp32 [B, Hkv, S_max]: one scale per cached head
    vector, element = scale * e4m3(code)): the rotated k is ALSO written back in place in qkv (bf16), and those bf16
    values, and v, are quantised into the caches by ops.quantize_weight_fp8's arithmetic with the head vector as the
    row. A skipped token stores nothing at all."""
    if qkv.dim() != 3:
        raise ValueError("kv_cache_append: qkv must be [batch, tokens, (heads + 2 kv_heads) * head_dim]")
    B, T, W = qkv.shape
    Hq, Hkv = int(num_heads), int(num_kv_heads)
    if Hkv <= 0 or Hq % Hkv or W % (Hq + 2 * Hkv):
        raise ValueError(f"kv_cache_append: width {W} does not hold {Hq} + 2 x {Hkv} heads")
    D = W // (Hq + 2 * Hkv)
    _check_caches(k_cache, v_cache, B, D)
    if k_cache.shape[1] != Hkv:
        raise ValueError(f"kv_cache_append: cache has {k_cache.shape[1]} kv heads, expected {Hkv}")
    if cos.shape != sin.shape or cos.dim() != 2 or cos.shape[1] * 2 < D or cos.stride(1) != 1 or sin.stride(1) != 1 \
            or cos.stride(0) != sin.stride(0):
        raise ValueError("kv_cache_append: cos / sin must be equal-shaped [rows, >= head_dim / 2] unit-stride tables")
    if pos.shape != (B,) or pos.dtype != torch.int32 or pos.device != qkv.device:
        raise ValueError("kv_cache_append: pos must be int32 [batch] on qkv's device")
    if qkv.stride(2) != 1 or qkv.stride(1) < W:
        raise ValueError("kv_cache_append: qkv rows must be unit-stride (it is rotated in place)")
    fp8 = _check_scales("kv_cache_append", k_cache, v_cache, k_scale, v_scale, qkv.device)
    if qkv.device.type == "cpu":
        if fp8:
            _kv_append_fp8_reference(qkv, cos, sin, pos, k_cache, v_cache, k_scale, v_scale, Hq, Hkv)
        else:
            _kv_append_reference(qkv, cos, sin, pos, k_cache, v_cache, Hq, Hkv)
    elif fp8:
        for t, n in ((qkv, "qkv"), (cos, "cos"), (sin, "sin")):
            ops._need(t, n)
        _lib.check(_lib.load().pico_kv_append_fp8(
            _lib.ptr(qkv), qkv.stride(0), qkv.stride(1), _lib.ptr(cos), _lib.ptr(sin), cos.stride(0), cos.shape[0],
            _lib.ptr(pos), _lib.ptr(k_cache), _lib.i64x3(k_cache.stride()[:3]), _lib.ptr(k_scale),
            _lib.i64x3(k_scale.stride()), _lib.ptr(v_cache), _lib.i64x3(v_cache.stride()[:3]), _lib.ptr(v_scale),
            _lib.i64x3(v_scale.stride()), B, T, Hq, Hkv, k_cache.shape[2], D, _lib.stream_of(qkv)),
            "pico_kv_append_fp8")
    else:
        for t, n in ((qkv, "qkv"), (cos, "cos"), (sin, "sin"), (k_cache, "k_cache"), (v_cache, "v_cache")):
            ops._need(t, n)
        S = k_cache.shape[2]
        _lib.check(_lib.load().pico_kv_append(
            _lib.ptr(qkv), qkv.stride(0), qkv.stride(1), _lib.ptr(cos), _lib.ptr(sin), cos.stride(0), cos.shape[0],
            _lib.ptr(pos), _lib.ptr(k_cache), _lib.i64x3(k_cache.stride()[:3]), _lib.ptr(v_cache),
            _lib.i64x3(v_cache.stride()[:3]), B, T, Hq, Hkv, S, D, _lib.stream_of(qkv)), "pico_kv_append")
    return qkv.as_strided((B, T, Hq, D), (qkv.stride(0), qkv.stride(1), D, 1), qkv.storage_offset())


# --------------------------------------------------------------------------------------------
# Decode attention
# --------------------------------------------------------------------------------------------
def default_split_keys(batch, num_kv_heads, max_len, head_dim):
    """The library's host rule for the chunk length (shape and CU count only; csrc/attn_decode_plan.h)."""
    return int(_lib.load().pico_attn_decode_split_keys(batch, num_kv_heads, max_len, head_dim))


def _decode_reference(q, k_cache, v_cache, seqlens, scale, split_keys):
    B, Hq, D = q.shape
    Hkv, S = k_cache.shape[1], k_cache.shape[2]
    G = Hq // Hkv
    ct = _compute_dtype(q)
    sk = S if split_keys is None else int(split_keys)
    nsplit = (S + sk - 1) // sk
    pad = nsplit * sk - S
    lens = seqlens.to(torch.int64).clamp(0, S)
    live = torch.arange(S)[None, :] < lens[:, None]  # [B, S]
    sel = live[:, None, :, None]
    # contents at or beyond the length never reach the result (a stale NaN times p = 0 would)
    kf = torch.where(sel, k_cache.to(ct), torch.zeros((), dtype=ct))
    vf = torch.where(sel, v_cache.to(ct), torch.zeros((), dtype=ct))
    s = torch.einsum("bhgd,bhsd->bhgs", q.to(ct).view(B, Hkv, G, D), kf) * scale
    s = s.masked_fill(~live[:, None, None, :], float("-inf"))
    if pad:
        s = torch.nn.functional.pad(s, (0, pad), value=float("-inf"))
        vf = torch.nn.functional.pad(vf, (0, 0, 0, pad))
    s = s.view(B, Hkv, G, nsplit, sk)
    vf = vf.view(B, Hkv, nsplit, sk, D)
    # per chunk: (m, l, o) against the chunk's own maximum, 0 in its place where the chunk is empty
    m = s.amax(dim=-1)
    ms = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), m)
    p = torch.exp(s - ms[..., None])
    l = p.sum(dim=-1)
    o = torch.einsum("bhgcs,bhcsd->bhgcd", p, vf)
    # combine in chunk order
    mt = m.amax(dim=-1)
    mts = torch.where(torch.isinf(mt) & (mt < 0), torch.zeros_like(mt), mt)
    w = torch.exp(m - mts[..., None])
    lt = (l * w).sum(dim=-1)
    ot = (o * w[..., None]).sum(dim=-2)
    any_ = lt > 0
    out = torch.where(any_[..., None], ot / lt.clamp_min(torch.finfo(ct).tiny)[..., None], torch.zeros((), dtype=ct))
    lse = torch.where(any_, mt + torch.log(lt), torch.full((), float("-inf"), dtype=ct))
    return out.reshape(B, Hq, D).to(q.dtype), lse.reshape(B, Hq)


_WORKSPACES = {}


def _workspace(device, nbytes):
    """One grow-only workspace per (device, stream): a decode step never allocates after its first call."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        _WORKSPACES[key] = ws
    return ws


def attention_decode(q, k_cache, v_cache, seqlens, softmax_scale=None, split_keys=None, return_lse=False,
                     k_scale=None, v_scale=None):
    """softmax(scale q K^T) V for one query per sequence against a head-major cache.

    q [B, Hq, D] (unit last stride; a view of the projection output is fine), k_cache / v_cache [B, Hkv, S_max, D],
    seqlens int32 [B] on q's device: row b attends to keys [0, min(seqlens[b], S_max)). Returns O [B, Hq, D] in q's
    dtype (and LSE [B, Hq] fp32, natural log, with return_lse). seqlens[b] = 0 gives O = 0, LSE = -inf. Hq / Hkv
    may be 1..8. split_keys: keys per chunk of the split (None: the library's host rule, which never reads the
    device lengths); the result is deterministic for a given split_keys and independent of the other rows.

    FP8 caches (float8_e4m3fn codes with k_scale / v_scale fp32 [B, Hkv, S_max]) take pico_attn_decode_fp8: the same
    attention on the values scale * e4m3(code), in fp32; codes and scales beyond the length are never used."""
    if q.dim() != 3 or q.stride(-1) != 1:
        raise ValueError("attention_decode: q must be [batch, heads, head_dim] with unit last stride")
    B, Hq, D = q.shape
    _check_caches(k_cache, v_cache, B, D)
    Hkv, S = k_cache.shape[1], k_cache.shape[2]
    if Hq % Hkv:
        raise ValueError(f"attention_decode: {Hq} query heads are not a multiple of {Hkv} kv heads")
    if Hq // Hkv > MAX_GROUP:
        raise ValueError(f"attention_decode: {Hq // Hkv} query heads per kv head; at most {MAX_GROUP} are supported")
    if seqlens.shape != (B,) or seqlens.dtype != torch.int32 or seqlens.device != q.device:
        raise ValueError("attention_decode: seqlens must be int32 [batch] on q's device")
    if split_keys is not None and int(split_keys) <= 0:
        raise ValueError("attention_decode: split_keys must be positive")
    scale = 1.0 / math.sqrt(D) if softmax_scale is None else float(softmax_scale)
    fp8 = _check_scales("attention_decode", k_cache, v_cache, k_scale, v_scale, q.device)
    if q.device.type == "cpu":
        if fp8:  # dequantised exactly (fp32 holds scale * e4m3); stale NaNs are dropped by the reference
            ct = _compute_dtype(q)
            k_cache = k_cache.float().to(ct) * k_scale.to(ct)[..., None]
            v_cache = v_cache.float().to(ct) * v_scale.to(ct)[..., None]
        o, lse = _decode_reference(q, k_cache, v_cache, seqlens, scale, split_keys)
        return (o, lse) if return_lse else o
    for t, n in ((q, "q"),) if fp8 else ((q, "q"), (k_cache, "k_cache"), (v_cache, "v_cache")):
        ops._need(t, n)
    lib = _lib.load()
    sk = 0 if split_keys is None else int(split_keys)
    nbytes = int(lib.pico_attn_decode_workspace_bytes(B, Hq, Hkv, S, D, sk))
    if nbytes < 0:
        raise RuntimeError("attention_decode: " + lib.pico_last_error().decode(errors="replace"))
    ws = _workspace(q.device, nbytes)
    o = torch.empty((B, Hq, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, Hq), dtype=torch.float32, device=q.device)
    qs = (_lib.c_i64 * 2)(q.stride(0), q.stride(1))
    if fp8:
        _lib.check(lib.pico_attn_decode_fp8(
            _lib.ptr(q), qs, _lib.ptr(k_cache), _lib.i64x3(k_cache.stride()[:3]), _lib.ptr(k_scale),
            _lib.i64x3(k_scale.stride()), _lib.ptr(v_cache), _lib.i64x3(v_cache.stride()[:3]), _lib.ptr(v_scale),
            _lib.i64x3(v_scale.stride()), _lib.ptr(seqlens), _lib.ptr(o), _lib.ptr(lse), _lib.ptr(ws), B, Hq, Hkv, S,
            D, scale, sk, _lib.stream_of(q)), "pico_attn_decode_fp8")
        return (o, lse) if return_lse else o
    _lib.check(lib.pico_attn_decode(_lib.ptr(q), qs, _lib.ptr(k_cache), _lib.i64x3(k_cache.stride()[:3]),
                                    _lib.ptr(v_cache), _lib.i64x3(v_cache.stride()[:3]), _lib.ptr(seqlens),
                                    _lib.ptr(o), _lib.ptr(lse), _lib.ptr(ws), B, Hq, Hkv, S, D, scale, sk,
                                    _lib.stream_of(q)), "pico_attn_decode")
    return (o, lse) if return_lse else o


# --------------------------------------------------------------------------------------------
# Extend attention: T <= 16 new queries per sequence
# --------------------------------------------------------------------------------------------
def default_extend_split_keys(batch, tokens, num_heads, num_kv_heads, max_len, head_dim):
    """The library's host rule for pico_attn_extend's chunk length (shape and CU count only;
    csrc/attn_extend_plan.h)."""
    return int(_lib.load().pico_attn_extend_split_keys(batch, tokens, num_heads, num_kv_heads, max_len, head_dim))


def _extend_reference(q, k_cache, v_cache, seqlens, scale, split_keys):
    """attention_extend's contract in plain torch: per chunk (m, l, o) against the chunk's own maximum, combined in
    chunk order. bf16 inputs: fp32 scores, p rounded to bf16 before the PV product (l sums the unrounded p), as the
    kernel; other dtypes: their compute dtype throughout."""
    B, T, Hq, D = q.shape
    Hkv, S = k_cache.shape[1], k_cache.shape[2]
    G = Hq // Hkv
    ct = _compute_dtype(q)
    sk = S if split_keys is None else int(split_keys)
    nsplit = (S + sk - 1) // sk
    pad = nsplit * sk - S
    raw = seqlens.to(torch.int64)
    keys = torch.arange(S)
    live = keys[None, :] < raw.clamp(0, S)[:, None]                                    # [B, S]
    vis = keys[None, None, :] < (raw[:, None] - (T - 1 - torch.arange(T))[None, :]).clamp(0, S)[:, :, None]  # [B, T, S]
    sel = live[:, None, :, None]
    # contents at or beyond the length never reach the result (a stale NaN times p = 0 would)
    kf = torch.where(sel, k_cache.to(ct), torch.zeros((), dtype=ct))
    vf = torch.where(sel, v_cache.to(ct), torch.zeros((), dtype=ct))
    s = torch.einsum("bthgd,bhsd->bhtgs", q.to(ct).reshape(B, T, Hkv, G, D), kf) * scale
    s = s.masked_fill(~vis[:, None, :, None, :], float("-inf"))
    if pad:
        s = torch.nn.functional.pad(s, (0, pad), value=float("-inf"))
        vf = torch.nn.functional.pad(vf, (0, 0, 0, pad))
    s = s.view(B, Hkv, T, G, nsplit, sk)
    vf = vf.view(B, Hkv, nsplit, sk, D)
    m = s.amax(dim=-1)
    ms = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), m)
    p = torch.exp(s - ms[..., None])
    l = p.sum(dim=-1)
    if q.dtype == torch.bfloat16:
        p = p.to(torch.bfloat16).to(ct)
    o = torch.einsum("bhtgcs,bhcsd->bhtgcd", p, vf)
    mt = m.amax(dim=-1)
    mts = torch.where(torch.isinf(mt) & (mt < 0), torch.zeros_like(mt), mt)
    w = torch.exp(m - mts[..., None])
    lt = (l * w).sum(dim=-1)
    ot = (o * w[..., None]).sum(dim=-2)
    any_ = lt > 0
    out = torch.where(any_[..., None], ot / lt.clamp_min(torch.finfo(ct).tiny)[..., None], torch.zeros((), dtype=ct))
    lse = torch.where(any_, mt + torch.log(lt), torch.full((), float("-inf"), dtype=ct))
    return out.permute(0, 2, 1, 3, 4).reshape(B, T, Hq, D).to(q.dtype), lse.permute(0, 2, 1, 3).reshape(B, T, Hq)


def attention_extend(q, k_cache, v_cache, seqlens, softmax_scale=None, split_keys=None, return_lse=False):
    """softmax(scale q K^T) V for T <= 16 new queries per sequence against a head-major bf16 cache that already
    holds their keys (pico_attn_extend: split over the keys, on the matrix unit).

    q [B, T, Hq, D] (unit last stride; the view kv_cache_append returns), k_cache / v_cache [B, Hkv, S_max, D],
    seqlens int32 [B] on q's device: the keys the LAST query of the row sees, i.e. the row's length after the
    append. Query t attends to keys [0, clamp(seqlens[b] - (T - 1 - t), 0, S_max)). Returns O [B, T, Hq, D] in q's
    dtype (and LSE [B, T, Hq] fp32, natural log, with return_lse); a query with no visible key gives O = 0,
    LSE = -inf. Hq / Hkv may be 1..8. split_keys: keys per chunk (None: the library's host rule, which never reads
    the device lengths); deterministic for a given split_keys, a row independent of the other rows. CPU tensors run
    the plain-torch restatement (fp64 inputs: fp64 throughout, the reference). An FP8 cache is refused."""
    if q.dim() != 4 or q.stride(-1) != 1:
        raise ValueError("attention_extend: q must be [batch, tokens, heads, head_dim] with unit last stride")
    B, T, Hq, D = q.shape
    if not 1 <= T <= MAX_EXTEND_TOKENS:
        raise ValueError(f"attention_extend: {T} tokens per row; 1 to {MAX_EXTEND_TOKENS} are supported")
    if k_cache.dtype == _E4M3 or v_cache.dtype == _E4M3:
        raise ValueError("attention_extend: this kernel reads bf16 caches only, not an FP8 (float8_e4m3fn) cache")
    _check_caches(k_cache, v_cache, B, D)
    Hkv, S = k_cache.shape[1], k_cache.shape[2]
    if Hq % Hkv:
        raise ValueError(f"attention_extend: {Hq} query heads are not a multiple of {Hkv} kv heads")
    if Hq // Hkv > MAX_GROUP:
        raise ValueError(f"attention_extend: {Hq // Hkv} query heads per kv head; at most {MAX_GROUP} are supported")
    if seqlens.shape != (B,) or seqlens.dtype != torch.int32 or seqlens.device != q.device:
        raise ValueError("attention_extend: seqlens must be int32 [batch] on q's device")
    if split_keys is not None and int(split_keys) <= 0:
        raise ValueError("attention_extend: split_keys must be positive")
    scale = 1.0 / math.sqrt(D) if softmax_scale is None else float(softmax_scale)
    if q.device.type == "cpu":
        o, lse = _extend_reference(q, k_cache, v_cache, seqlens, scale, split_keys)
        return (o, lse) if return_lse else o
    for t, n in ((q, "q"), (k_cache, "k_cache"), (v_cache, "v_cache")):
        ops._need(t, n)
    lib = _lib.load()
    sk = 0 if split_keys is None else int(split_keys)
    nbytes = int(lib.pico_attn_extend_workspace_bytes(B, T, Hq, Hkv, S, D, sk))
    if nbytes < 0:
        raise RuntimeError("attention_extend: " + lib.pico_last_error().decode(errors="replace"))
    ws = _workspace(q.device, nbytes)
    o = torch.empty((B, T, Hq, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, T, Hq), dtype=torch.float32, device=q.device)
    _lib.check(lib.pico_attn_extend(_lib.ptr(q), _lib.i64x3(q.stride()[:3]), _lib.ptr(k_cache),
                                    _lib.i64x3(k_cache.stride()[:3]), _lib.ptr(v_cache),
                                    _lib.i64x3(v_cache.stride()[:3]), _lib.ptr(seqlens), _lib.ptr(o), _lib.ptr(lse),
                                    _lib.ptr(ws), B, T, Hq, Hkv, S, D, scale, sk, _lib.stream_of(q)),
               "pico_attn_extend")
    return (o, lse) if return_lse else o


# --------------------------------------------------------------------------------------------
# Model level
# --------------------------------------------------------------------------------------------
def _check_model(model):
    from .model import Llama
    if type(model) is not Llama:
        raise TypeError(f"generate: expected a plain picotron_amd.model.Llama, got {type(model).__name__} "
                        "(pass a data-parallel wrapper's .module)")
    m = pgm.process_group_manager
    if m is not None and (m.tp_world_size > 1 or m.pp_world_size > 1 or m.cp_world_size > 1):
        raise RuntimeError("generate: tensor / pipeline / context parallel generation is not supported")
    if os.getenv("CONTEXT_PARALLEL", "0") == "1":
        raise RuntimeError("generate: context parallel generation is not supported (CONTEXT_PARALLEL=1)")
    for layer in model.decoder_layers:
        a, f = layer.attention, layer.mlp
        for lin in (a.q_proj, a.k_proj, a.v_proj, a.out_proj, f.gate_proj, f.up_proj, f.down_proj):
            if type(lin) is not nn.Linear or lin.bias is not None:
                raise RuntimeError(f"generate: {type(lin).__name__} projection: tensor-parallel (or biased) layers "
                                   "are not supported")
    if type(model.final_proj) is not nn.Linear or model.final_proj.bias is not None:
        raise RuntimeError("generate: the LM head must be a plain bias-free nn.Linear")
    if model.num_heads // model.num_key_values > MAX_GROUP:
        raise ValueError(f"generate: {model.num_heads // model.num_key_values} query heads per kv head; the decode "
                         f"kernel supports at most {MAX_GROUP}")


class KVCache:
    """Head-major KV cache of a Llama: .k / .v [layers, batch, kv_heads, max_len, head_dim] bf16, .lens int32
    [batch] on the device (tokens held per row).

    kv_dtype=torch.float8_e4m3fn: .k / .v hold OCP e4m3 codes and .k_scale / .v_scale [layers, batch, kv_heads,
    max_len] fp32 one scale per cached head vector (element = scale * e4m3(code)): D + 4 bytes per cached row
    instead of 2 D. A row is quantised once, when it is appended. None (the default): bf16, no scales."""

    def __init__(self, model, batch, max_len, device=None, kv_dtype=None):
        _check_model(model)
        if max_len > model.max_position_embeddings:
            raise ValueError(f"KVCache: max_len {max_len} exceeds the model's RoPE table "
                             f"(max_position_embeddings {model.max_position_embeddings})")
        if batch <= 0 or max_len <= 0:
            raise ValueError("KVCache: batch and max_len must be positive")
        device = torch.device(device) if device is not None else model.final_proj.weight.device
        shape = (model.num_layers, batch, model.num_key_values, max_len, model.head_dim)
        if kv_dtype not in (None, torch.bfloat16, _E4M3):
            raise ValueError(f"KVCache: kv_dtype {kv_dtype} is not supported (None / torch.bfloat16, or "
                             "torch.float8_e4m3fn)")
        self.kv_dtype = torch.bfloat16 if kv_dtype is None else kv_dtype
        self.k_scale = self.v_scale = None
        if self.kv_dtype == _E4M3:  # code 0 with scale 1: a cache of zeros, as the bf16 one
            self.k = torch.zeros(shape, dtype=torch.uint8, device=device).view(_E4M3)
            self.v = torch.zeros(shape, dtype=torch.uint8, device=device).view(_E4M3)
            self.k_scale = torch.ones(shape[:4], dtype=torch.float32, device=device)
            self.v_scale = torch.ones(shape[:4], dtype=torch.float32, device=device)
        else:
            self.k = torch.zeros(shape, dtype=torch.bfloat16, device=device)
            self.v = torch.zeros(shape, dtype=torch.bfloat16, device=device)
        self.lens = torch.zeros(batch, dtype=torch.int32, device=device)
        self.batch, self.max_len = batch, max_len
        self._plan, self._plan_model = None, None  # prefill's per-layer table (_layer_plan)
        self._graph, self.graph_captures = None, 0  # generate(graph=True)'s captured iteration (_DecodeGraph)

    def reset(self):
        self.lens.zero_()

    def rewind(self, n):
        """Drop the last n tokens of every row (n: int >= 0), or n[b] of row b (int32 [batch] on the cache's device):
        lens = max(lens - n, 0), on the device, no synchronisation. The dropped rows stay in the cache beyond the
        length, where nothing reads them, until the next append overwrites them. With extend_step this is what a
        speculative or lookup loop needs to take back rejected drafts."""
        if isinstance(n, torch.Tensor):
            if n.shape != (self.batch,) or n.dtype != torch.int32 or n.device != self.lens.device:
                raise ValueError("KVCache.rewind: a tensor n must be int32 [batch] on the cache's device")
        elif not isinstance(n, int) or isinstance(n, bool) or n < 0:
            raise ValueError("KVCache.rewind: n must be a non-negative int or an int32 [batch] tensor")
        self.lens.sub_(n).clamp_(min=0)


def _layer_plan(model, cache, dev):
    """What a pass over the decoder stack reads, gathered once per prefill (a decode step then spends no host time on
    it): per layer the norm weights, the stacked q|k|v and gate|up weights (ops.stacked_weight: the parameters
    themselves, no copy), the other two projections, the RoPE tables and the layer's cache views (with the scale
    views of an FP8 cache, else None)."""
    plan = []
    for i, layer in enumerate(model.decoder_layers):
        a, f = layer.attention, layer.mlp
        if layer.cos.device != dev:  # the layers build their tables on the device of construction
            layer.cos, layer.sin = layer.cos.to(dev), layer.sin.to(dev)
        plan.append((layer.input_layernorm.weight, layer.input_layernorm.eps,
                     ops.stacked_weight((a.q_proj.weight, a.k_proj.weight, a.v_proj.weight)), a.out_proj.weight,
                     layer.post_attention_layernorm.weight, layer.post_attention_layernorm.eps,
                     ops.stacked_weight((f.gate_proj.weight, f.up_proj.weight)), f.down_proj.weight,
                     layer.cos, layer.sin, cache.k[i], cache.v[i],
                     cache.k_scale[i] if cache.k_scale is not None else None,
                     cache.v_scale[i] if cache.v_scale is not None else None))
    cache._plan, cache._plan_model = plan, model
    return plan


def _layers(model, plan, x, pos, attend):
    """The decoder stack on x [B, T, hidden] with the residual adds fused into the norms, exactly the training
    forward's rounding points. attend(q, k_cache, v_cache, k_scale, v_scale) -> [B, T, Hq * D], after kv_cache_append
    wrote the cache."""
    Hq, Hkv = model.num_heads, model.num_key_values
    B, T = x.shape[:2]
    linear = torch.nn.functional.linear
    delta, residual = x, None
    for w_in, eps_in, w_qkv, w_out, w_post, eps_post, w_gu, w_down, cos, sin, kc, vc, ksc, vsc in plan:
        h, residual = ops.rms_norm(delta, w_in, eps_in, residual=residual, prenorm=True)
        q = kv_cache_append(linear(h, w_qkv), cos, sin, pos, kc, vc, Hq, Hkv, ksc, vsc)
        h2, residual = ops.rms_norm(linear(attend(q, kc, vc, ksc, vsc), w_out), w_post, eps_post, residual=residual,
                                    prenorm=True)
        gu = linear(h2, w_gu).view(B * T, -1)
        inter = gu.shape[1] // 2
        act = torch.empty((B * T, inter), dtype=gu.dtype, device=gu.device)
        ops._swiglu_fwd(gu, gu[:, inter:], act, B * T, inter, 2 * inter, inter)  # the strided form: no copies
        delta = linear(act, w_down).view(B, T, -1)
    return delta, residual


def _head(model, delta, residual):
    h = ops.rms_norm(delta, model.final_norm.weight, model.final_norm.eps, residual=residual)
    return torch.nn.functional.linear(h, model.final_proj.weight).float()


def _check_skinny(model, B):
    """skinny_linear=True is refused up front where ops.decode_linear would refuse a projection: it never switches
    back to the default route by itself."""
    if B > ops.DECODE_LINEAR_MAX_ROWS:
        raise ValueError(f"generate: skinny_linear=True serves at most {ops.DECODE_LINEAR_MAX_ROWS} rows per decode "
                         f"step, got batch {B}")
    a, f = model.decoder_layers[0].attention, model.decoder_layers[0].mlp
    rows = {"q|k|v": a.q_proj.weight.shape[0] + a.k_proj.weight.shape[0] + a.v_proj.weight.shape[0],
            "out": a.out_proj.weight.shape[0], "down": f.down_proj.weight.shape[0],
            "LM head": model.final_proj.weight.shape[0]}
    cols = {"q|k|v": a.q_proj.weight.shape[1], "out": a.out_proj.weight.shape[1], "gate|up": f.gate_proj.weight.shape[1],
            "down": f.down_proj.weight.shape[1], "LM head": model.final_proj.weight.shape[1]}
    bad = [f"{n} N = {v}" for n, v in rows.items() if v % 8] + [f"{n} K = {v}" for n, v in cols.items() if v % 32]
    if f.gate_proj.weight.shape[0] % 8:
        bad.append(f"gate / up N = {f.gate_proj.weight.shape[0]}")
    if bad:
        raise ValueError("generate: skinny_linear=True needs every projection's K to be a multiple of 32 and its N of 8 "
                         f"(ops.decode_linear): {', '.join(bad)}")


class DecodeWeights:
    """The decode projections of a model as FP8 weights (ops.Fp8Weight: e4m3 codes, one fp32 scale per output row)
    or as MXFP4 weights (ops.Mxfp4Weight: e2m1 codes, one E8M0 scale byte per 32 columns), one kind throughout:
    per layer the stacked q|k|v, out, the stacked gate|up and down, plus the LM head. Norm weights and the embedding
    are not part of it: they stay the model's bf16 parameters. A snapshot: it holds what the model's weights were
    when quantize_decode_weights ran and does not follow an optimizer step or a load_state_dict; quantise again."""

    def __init__(self, layers, head):
        self.layers, self.head = layers, head

    @property
    def fmt(self):
        return "mxfp4" if isinstance(self.head, ops.Mxfp4Weight) else "fp8"

    def shapes(self):
        return [tuple(tuple(w.shape) for w in layer) for layer in self.layers] + [tuple(self.head.shape)]


def _decode_shapes(model):
    """DecodeWeights.shapes() as the model's parameters have them."""
    out = []
    for layer in model.decoder_layers:
        a, f = layer.attention, layer.mlp
        K = a.q_proj.weight.shape[1]
        qkv = a.q_proj.weight.shape[0] + a.k_proj.weight.shape[0] + a.v_proj.weight.shape[0]
        out.append(((qkv, K), tuple(a.out_proj.weight.shape), (2 * f.gate_proj.weight.shape[0], K),
                    tuple(f.down_proj.weight.shape)))
    return out + [tuple(model.final_proj.weight.shape)]


@torch.no_grad()
def quantize_decode_weights(model, fmt="fp8"):
    """DecodeWeights of `model`: every decode projection quantised once by ops.quantize_weight_fp8 (the stacked
    q|k|v and gate|up as the stacked views ops.stacked_weight gives, without a bf16 copy). Pass the result as
    decode_step / generate's decode_weights (with skinny_linear=True). It is a snapshot of the weights as they are
    now, half the bytes of the bf16 projections plus 4 bytes per output row. fmt="mxfp4": by
    ops.quantize_weight_mxfp4 instead, a quarter of the bf16 bytes plus one scale byte per 32 weights (every
    projection's K must be a multiple of 32 to quantise, of 128 to decode)."""
    _check_model(model)
    if fmt not in ("fp8", "mxfp4"):
        raise ValueError(f"quantize_decode_weights: fmt is 'fp8' or 'mxfp4', got {fmt!r}")
    q = ops.quantize_weight_fp8 if fmt == "fp8" else ops.quantize_weight_mxfp4
    layers = []
    for layer in model.decoder_layers:
        a, f = layer.attention, layer.mlp
        layers.append((q((a.q_proj.weight, a.k_proj.weight, a.v_proj.weight)), q(a.out_proj.weight),
                       q((f.gate_proj.weight, f.up_proj.weight)), q(f.down_proj.weight)))
    return DecodeWeights(layers, q(model.final_proj.weight))


def _check_decode_weights(model, w, skinny_linear):
    """decode_weights is refused without skinny_linear, for another model's shapes, and where ops.decode_linear
    would refuse a projection (an Fp8Weight needs K to be a multiple of 64, an Mxfp4Weight of 128)."""
    if not skinny_linear:
        raise ValueError("generate: decode_weights belongs to skinny_linear=True (the FP8 weights are read by "
                         "ops.decode_linear alone)")
    if not isinstance(w, DecodeWeights) or w.shapes() != _decode_shapes(model):
        raise ValueError("generate: decode_weights does not fit this model (quantize_decode_weights(model) makes it)")
    *layers, head = w.shapes()
    bad = sorted({k for layer in layers for _, k in layer} | {head[1]})
    if w.fmt == "mxfp4":
        bad = [f"K = {k}" for k in bad if k % 128]
        if bad:
            raise ValueError("generate: MXFP4 decode_weights need every projection's K to be a multiple of 128 "
                             f"(ops.decode_linear with an Mxfp4Weight): {', '.join(bad)}")
        return
    bad = [f"K = {k}" for k in bad if k % 64]
    if bad:
        raise ValueError("generate: decode_weights needs every projection's K to be a multiple of 64 "
                         f"(ops.decode_linear with an Fp8Weight): {', '.join(bad)}")


def _layers_skinny(model, plan, x, pos, attend, decode_weights=None):
    """_layers for a decode step (x [B, 1, hidden]) or an extend step (x [B, T, hidden]), B T <= 16 rows, on
    ops.decode_linear: each norm runs inside the projection after it and the SwiGLU inside gate|up, with _layers'
    rounding points. Per layer: norm + q|k|v, the cache append, the attention, the out projection, norm + gate|up +
    SwiGLU, the down projection. decode_weights: the four projections read its Fp8Weights (or Mxfp4Weights) instead
    of the plan's bf16 weights. Returns delta, residual as [B T, hidden]."""
    Hq, Hkv = model.num_heads, model.num_key_values
    B, T = x.shape[:2]
    delta, residual = x.view(B * T, -1), None
    for i, (w_in, eps_in, w_qkv, w_out, w_post, eps_post, w_gu, w_down, cos, sin, kc, vc, ksc, vsc) in enumerate(plan):
        if decode_weights is not None:
            w_qkv, w_out, w_gu, w_down = decode_weights.layers[i]
        qkv, residual = ops.decode_linear(delta, w_qkv, norm_weight=w_in, eps=eps_in, residual=residual)
        q = kv_cache_append(qkv.view(B, T, -1), cos, sin, pos, kc, vc, Hq, Hkv, ksc, vsc)
        o = ops.decode_linear(attend(q, kc, vc, ksc, vsc).view(B * T, -1), w_out)
        act, residual = ops.decode_linear(o, w_gu, norm_weight=w_post, eps=eps_post, residual=residual, swiglu=True)
        delta = ops.decode_linear(act, w_down)
    return delta, residual


def _head_skinny(model, delta, residual, decode_weights=None):
    w = model.final_proj.weight if decode_weights is None else decode_weights.head
    return ops.decode_linear(delta, w, norm_weight=model.final_norm.weight,
                             eps=model.final_norm.eps, residual=residual, out_dtype=torch.float32)[0]


@torch.no_grad()
def reference_logits(model, tokens, num_heads, num_kv_heads, fp8_from=None):
    """Teacher-forced logits [T, V] of one row of tokens [T], token by token on the CPU restatements of
    kv_cache_append and attention_decode, in the dtype of the weights (fp32 for a reference): the model-level
    counterpart of those restatements, for a CPU copy of a Llama (this package's or the oracle's: only the
    parameters, the norms' eps and the layers' RoPE tables are read). fp8_from=None: an exact cache of that dtype.
    fp8_from=p: the queries from position p on attend to an FP8 cache (every K / V through the quantiser), the
    ones before it to the exact cache, as prefill with a prompt of p tokens followed by decode steps does."""
    lin = torch.nn.functional.linear
    T, Hq, Hkv = tokens.shape[0], int(num_heads), int(num_kv_heads)
    w0 = model.embedding.weight
    D = w0.shape[1] // Hq
    shape = (len(model.decoder_layers), 1, Hkv, T, D)
    kx, vx = torch.zeros(shape, dtype=w0.dtype), torch.zeros(shape, dtype=w0.dtype)
    k8, v8 = torch.zeros(shape, dtype=torch.uint8).view(_E4M3), torch.zeros(shape, dtype=torch.uint8).view(_E4M3)
    ks, vs = torch.ones(shape[:4]), torch.ones(shape[:4])

    def norm(x, m):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + m.eps) * m.weight

    out = []
    for t in range(T):
        x = w0[tokens[t]].view(1, 1, -1)
        pos, n = torch.tensor([t], dtype=torch.int32), torch.tensor([t + 1], dtype=torch.int32)
        for i, layer in enumerate(model.decoder_layers):
            a, f, h = layer.attention, layer.mlp, norm(x, layer.input_layernorm)
            qkv = torch.cat([lin(h, a.q_proj.weight), lin(h, a.k_proj.weight), lin(h, a.v_proj.weight)], -1)
            cos, sin = layer.cos[:, : D // 2].to(w0.dtype), layer.sin[:, : D // 2].to(w0.dtype)
            if fp8_from is not None:
                kv_cache_append(qkv.clone(), cos, sin, pos, k8[i], v8[i], Hq, Hkv, k_scale=ks[i], v_scale=vs[i])
            q = kv_cache_append(qkv, cos, sin, pos, kx[i], vx[i], Hq, Hkv)[:, 0]
            if fp8_from is not None and t >= fp8_from:
                o = attention_decode(q, k8[i], v8[i], n, k_scale=ks[i], v_scale=vs[i])
            else:
                o = attention_decode(q, kx[i], vx[i], n)
            x = x + lin(o.view(1, 1, -1), a.out_proj.weight)
            h = norm(x, layer.post_attention_layernorm)
            x = x + lin(torch.nn.functional.silu(lin(h, f.gate_proj.weight)) * lin(h, f.up_proj.weight),
                        f.down_proj.weight)
        out.append(lin(norm(x, model.final_norm), model.final_proj.weight)[0, 0])
    return torch.stack(out)


def _check_cache(model, cache, B):
    if not isinstance(cache, KVCache) or cache.batch != B or cache.k.shape[0] != model.num_layers:
        raise ValueError("generate: the cache does not fit this model / batch")


@torch.no_grad()
def prefill(model, input_ids, cache, prompt_lens=None):
    """Run the prompts through the model and fill `cache` from position 0: returns the fp32 logits [B, V] of each
    row's last prompt token. input_ids [B, T] is right-padded to a common length; prompt_lens (int tensor or list,
    default T for every row) gives the rows' true lengths. The padding positions are written to the cache too, but
    lie at or beyond the row's length: decode steps overwrite them before they can be read.

    With an FP8 cache the prompt attention reads the bf16 K / V where kv_cache_append left them, in the projection
    output (strided views, through the attention kernel's stride arguments): the prompt is attended exactly as
    with a bf16 cache, and the cache receives the quantised copy."""
    _check_model(model)
    if input_ids.dim() != 2:
        raise ValueError("prefill: input_ids must be [batch, tokens]")
    B, T = input_ids.shape
    _check_cache(model, cache, B)
    if T < 1 or T > cache.max_len:
        raise ValueError(f"prefill: prompt length {T} does not fit the cache (max_len {cache.max_len})")
    dev = input_ids.device
    if prompt_lens is None:
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    else:
        lens = torch.as_tensor(prompt_lens, dtype=torch.int32).to(dev)
        if lens.shape != (B,):
            raise ValueError("prefill: prompt_lens must have one entry per row")
        if isinstance(prompt_lens, (list, tuple)) and not all(1 <= int(n) <= T for n in prompt_lens):
            raise ValueError(f"prefill: prompt_lens must lie in [1, {T}]")
    Hq, Hkv, D = model.num_heads, model.num_key_values, model.head_dim
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    scale = 1.0 / math.sqrt(D)

    def attend(q, kc, vc, ksc, vsc):
        if ksc is None:
            k, v = kc.transpose(1, 2)[:, :T], vc.transpose(1, 2)[:, :T]
        else:  # the rotated k and the v of the projection output q is a view of
            st, off = (q.stride(0), q.stride(1), D, 1), q.storage_offset()
            k = q.as_strided((B, T, Hkv, D), st, off + Hq * D)
            v = q.as_strided((B, T, Hkv, D), st, off + (Hq + Hkv) * D)
        o, _ = ops.attention_block_fwd(q, k, v, scale, True)
        return o.view(B, T, Hq * D)

    x = torch.nn.functional.embedding(input_ids, model.embedding.weight)
    delta, residual = _layers(model, _layer_plan(model, cache, dev), x, pos, attend)
    last = (lens.to(torch.int64) - 1).clamp(0, T - 1)
    rows = torch.arange(B, device=dev)
    logits = _head(model, delta[rows, last], residual[rows, last] if residual is not None else None)
    cache.lens.copy_(lens.clamp(0, T))
    return logits


@torch.no_grad()
def decode_step(model, tokens, cache, skinny_linear=False, decode_weights=None):
    """One token per row: tokens int64 [B] -> fp32 logits [B, V] of the next token; the cache grows by one. No host
    synchronisation: the positions are cache.lens on the device. A row whose cache is full writes nothing and
    attends to the full cache (generate() refuses lengths that would get there). The cache's own format decides
    the kernels: an FP8 KVCache appends through pico_kv_append_fp8 and attends through pico_attn_decode_fp8.

    skinny_linear=True (B <= 16): the projections run on ops.decode_linear, one pass over each weight with the norm
    before it and the SwiGLU after it in the same launch, instead of F.linear and the row-wise kernels beside it.

    decode_weights (quantize_decode_weights(model); with skinny_linear=True only, refused otherwise, for another
    model's shapes, or where a projection's K is not a multiple of 64): the projections stream FP8 weights, half the
    bytes. Prefill does not take it: the prompt's K/V come from the bf16 weights, the generated tokens' from the
    FP8 ones."""
    if tokens.dim() != 1:
        raise ValueError("decode_step: tokens must be [batch]")
    B = tokens.shape[0]
    if decode_weights is not None:
        _check_decode_weights(model, decode_weights, skinny_linear)
    if skinny_linear:
        _check_skinny(model, B)
    plan = cache._plan if isinstance(cache, KVCache) and cache._plan_model is model else None
    if plan is None:  # a cache this model has not prefilled: the full checks, once
        _check_model(model)
        _check_cache(model, cache, B)
        plan = _layer_plan(model, cache, tokens.device)
    elif cache.batch != B:
        raise ValueError("generate: the cache does not fit this model / batch")
    Hq, D = model.num_heads, model.head_dim
    seqlens = cache.lens + 1

    def attend(q, kc, vc, ksc, vsc):
        return attention_decode(q.view(B, Hq, D), kc, vc, seqlens, k_scale=ksc, v_scale=vsc).view(B, 1, Hq * D)

    x = torch.nn.functional.embedding(tokens.view(B, 1), model.embedding.weight)
    if skinny_linear:
        logits = _head_skinny(model, *_layers_skinny(model, plan, x, cache.lens, attend, decode_weights),
                              decode_weights)
    else:
        delta, residual = _layers(model, plan, x, cache.lens, attend)
        logits = _head(model, delta[:, 0], residual[:, 0] if residual is not None else None)
    cache.lens += 1
    return logits


@torch.no_grad()
def extend_step(model, tokens, cache, skinny_linear=False, decode_weights=None):
    """T tokens per row in one pass over the weights: tokens int64 [B, T], 1 <= T <= 16 -> fp32 logits [B, T, V],
    logits[:, t] being the next-token logits after tokens[:, t]; the cache grows by T. Positions are cache.lens on the
    device: no host synchronisation, fixed shapes. Token t of a row attends to the cache and to tokens 0..t of the
    call (attention_extend). With KVCache.rewind this is what verifying drafted tokens, continuing a cached
    conversation by a few tokens, or scoring against a long cache needs; decode_step is the T = 1 case on its own
    kernel (the two agree to rounding, not bit for bit).

    Refused before anything is written: an FP8 KVCache (the extend kernel reads bf16 caches), T outside 1..16, a
    cache shorter than T. Otherwise decode_step's rule for a full row holds: tokens past the end are skipped by the
    append and attend to the full cache.

    skinny_linear=True (B T <= 16 rows, refused beyond) and decode_weights: as in decode_step, over the B T rows."""
    if tokens.dim() != 2:
        raise ValueError("extend_step: tokens must be [batch, tokens]")
    B, T = tokens.shape
    if not 1 <= T <= MAX_EXTEND_TOKENS:
        raise ValueError(f"extend_step: {T} tokens per row; 1 to {MAX_EXTEND_TOKENS} are supported (prefill takes a "
                         "whole prompt)")
    if decode_weights is not None:
        _check_decode_weights(model, decode_weights, skinny_linear)
    if skinny_linear:
        if B * T > ops.DECODE_LINEAR_MAX_ROWS:
            raise ValueError(f"extend_step: skinny_linear=True serves at most {ops.DECODE_LINEAR_MAX_ROWS} rows "
                             f"(batch x tokens) per step, got {B} x {T}")
        _check_skinny(model, B * T)
    if isinstance(cache, KVCache) and cache.kv_dtype == _E4M3:
        raise ValueError("extend_step: an FP8 KVCache is not supported (the extend kernel reads bf16 caches only)")
    if isinstance(cache, KVCache) and cache.max_len < T:
        raise ValueError(f"extend_step: the cache (max_len {cache.max_len}) is shorter than the {T} tokens")
    plan = cache._plan if isinstance(cache, KVCache) and cache._plan_model is model else None
    if plan is None:
        _check_model(model)
        _check_cache(model, cache, B)
        plan = _layer_plan(model, cache, tokens.device)
    elif cache.batch != B:
        raise ValueError("generate: the cache does not fit this model / batch")
    Hq, D = model.num_heads, model.head_dim
    seqlens = cache.lens + T

    def attend(q, kc, vc, ksc, vsc):
        return attention_extend(q, kc, vc, seqlens).view(B, T, Hq * D)

    x = torch.nn.functional.embedding(tokens, model.embedding.weight)
    if skinny_linear:
        logits = _head_skinny(model, *_layers_skinny(model, plan, x, cache.lens, attend, decode_weights),
                              decode_weights).view(B, T, -1)
    else:
        logits = _head(model, *_layers(model, plan, x, cache.lens, attend))
    cache.lens += T
    return logits


def sample_next(logits, temperature=0.0, top_k=None, generator=None):
    """Next tokens int64 [B] from logits [B, V]: argmax at temperature 0, else a draw from
    softmax(logits / temperature), restricted to the top_k largest logits when top_k is given."""
    if logits.dim() != 2:
        raise ValueError("sample_next: logits must be [batch, vocab]")
    if temperature < 0:
        raise ValueError("sample_next: temperature must be >= 0")
    if top_k is not None and top_k < 1:
        raise ValueError("sample_next: top_k must be >= 1")
    if temperature == 0:
        return logits.argmax(dim=-1)
    x = logits.float() / temperature
    if top_k is not None and top_k < x.shape[-1]:
        vals, idx = torch.topk(x, int(top_k), dim=-1)
        draw = torch.multinomial(torch.softmax(vals, dim=-1), 1, generator=generator)
        return idx.gather(-1, draw).squeeze(-1)
    return torch.multinomial(torch.softmax(x, dim=-1), 1, generator=generator).squeeze(-1)


# --------------------------------------------------------------------------------------------
# Fused device sampler
# --------------------------------------------------------------------------------------------
_KEEP = object()
_F32_MAX = float(np.finfo(np.float32).max)
_PARAMS = struct.Struct("<ffiiiIII")  # csrc/sample.hip SampleParams


class SamplerState:
    """What pico_sample reads and writes on the device, so that a captured launch replays with the same arguments:
    .params (8 words: temperature, top_p, top_k, eos, pad, seed low / high), .draws int32 [batch] (draws made per
    row: the Philox counter and the column of .out), .done uint8 [batch] (row has emitted EOS), .tokens int64 [batch]
    (the last step's tokens), .kept int32 [batch] (size of the set the last token was drawn from) and optionally
    .out int64 [batch, cols] (unit last stride), of which step n writes column n.

    set() rewrites .params in place (a copy_ into the same tensor: a captured graph sees the new settings);
    reset() zeroes .draws and .done. seed=None takes torch.initial_seed()."""

    def __init__(self, batch, device, temperature=0.0, top_k=None, top_p=None, eos_token_id=None, pad_token_id=0,
                 seed=None, out=None):
        if batch <= 0:
            raise ValueError("SamplerState: batch must be positive")
        self.params = torch.zeros(8, dtype=torch.int32, device=device)
        device = self.params.device  # with its index
        self.batch, self.device = int(batch), device
        if out is not None and (out.dim() != 2 or out.shape[0] != batch or out.dtype != torch.int64
                                or out.device != device or (out.shape[1] > 1 and out.stride(1) != 1)):
            raise ValueError("SamplerState: out must be int64 [batch, cols] on the device with unit last stride")
        self.out = out
        self.draws = torch.zeros(batch, dtype=torch.int32, device=device)
        self.done = torch.zeros(batch, dtype=torch.uint8, device=device)
        self.tokens = torch.zeros(batch, dtype=torch.int64, device=device)
        self.kept = torch.zeros(batch, dtype=torch.int32, device=device)
        self._host = dict(temperature=0.0, top_k=None, top_p=None, eos_token_id=None, pad_token_id=0, seed=None)
        self.set(temperature=temperature, top_k=top_k, top_p=top_p, eos_token_id=eos_token_id,
                 pad_token_id=pad_token_id, seed=seed)

    def set(self, temperature=_KEEP, top_k=_KEEP, top_p=_KEEP, eos_token_id=_KEEP, pad_token_id=_KEEP, seed=_KEEP):
        h = dict(self._host)
        for k, v in (("temperature", temperature), ("top_k", top_k), ("top_p", top_p), ("eos_token_id", eos_token_id),
                     ("pad_token_id", pad_token_id), ("seed", seed)):
            if v is not _KEEP:
                h[k] = v
        if h["seed"] is None:
            h["seed"] = torch.initial_seed()
        if not h["temperature"] >= 0:
            raise ValueError("SamplerState: temperature must be >= 0")
        if h["top_k"] is not None and h["top_k"] < 1:
            raise ValueError("SamplerState: top_k must be >= 1")
        if h["top_p"] is not None and not 0 < h["top_p"] <= 1:
            raise ValueError("SamplerState: top_p must lie in (0, 1]")
        if h["eos_token_id"] is not None and h["eos_token_id"] < 0:
            raise ValueError("SamplerState: eos_token_id must be >= 0")
        seed = int(h["seed"]) & 0xFFFFFFFFFFFFFFFF
        words = _PARAMS.pack(float(h["temperature"]), 0.0 if h["top_p"] is None else float(h["top_p"]),
                             0 if h["top_k"] is None else min(int(h["top_k"]), 2 ** 31 - 1),
                             -1 if h["eos_token_id"] is None else int(h["eos_token_id"]), int(h["pad_token_id"]),
                             seed & 0xFFFFFFFF, seed >> 32, 0)
        self.params.copy_(torch.frombuffer(bytearray(words), dtype=torch.int32))
        self._host = h
        return self

    def reset(self):
        self.draws.zero_()
        self.done.zero_()
        return self


def _philox4x32_10(c0, c1, k0, k1):
    """Philox4x32-10 on uint64 numpy arrays holding 32-bit words, counter (c0, c1, 0, 0), key (k0, k1): the four output
    words (csrc/optim_common.h philox4x32_10)."""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1 = c0.astype(np.uint64) & m32, c1.astype(np.uint64) & m32
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        a, b = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = (b >> np.uint64(32)) ^ c1 ^ k0, (a >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = b & m32, a & m32, n0, n2
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def _sample_reference(logits, state):
    """pico_sample's contract in plain torch, on CPU tensors: fp64 masses (the kernel: fp32 exp, fixed-point sums),
    the same Philox draw, the same state updates."""
    B, V = logits.shape
    temperature, top_p, top_k, eos, pad, seed_lo, seed_hi, _ = _PARAMS.unpack(state.params.numpy().tobytes())
    x = logits.to(torch.float64)
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x).clamp(max=_F32_MAX)
    xmax = x.max(dim=-1, keepdim=True).values
    live = (xmax > float("-inf")).squeeze(-1)
    index = torch.arange(V)
    first_max = torch.where(x == xmax, index, V).min(dim=-1).values
    if not temperature > 0:
        tok, kept = first_max, torch.ones(B, dtype=torch.int64)
    else:
        w = torch.exp((x - torch.where(live[:, None], xmax, torch.zeros_like(xmax))) / temperature)
        keep = torch.ones(B, V, dtype=torch.bool)
        if 0 < top_k < V:
            keep &= x >= torch.topk(x, top_k, dim=-1).values[:, -1:]
        if 0 < top_p < 1:
            wk = w * keep
            xs, order = torch.sort(torch.where(keep, x, torch.full_like(x, float("-inf"))), dim=-1, descending=True,
                                   stable=True)
            csum = wk.gather(-1, order).cumsum(-1)
            target = np.float64(np.float32(top_p)).item() * wk.sum(-1, keepdim=True)
            # the first sorted position whose cumulative mass reaches the target carries the threshold value: a tie
            # group's full mass sits at its last position, so no larger value reaches the target
            j = (csum >= target).to(torch.int8).argmax(dim=-1, keepdim=True)
            keep &= x >= xs.gather(-1, j)
        rows = np.arange(B, dtype=np.uint64)
        w0, w1, _, _ = _philox4x32_10(rows, state.draws.numpy().astype(np.int64).astype(np.uint64), seed_lo, seed_hi)
        r = [(int(hi) << 32) | int(lo) for lo, hi in zip(w0, w1)]
        u = torch.tensor([ri / 2.0 ** 64 for ri in r], dtype=torch.float64)
        cum = (w * keep).cumsum(-1)
        last = torch.where(keep & (w > 0), index, -1).max(dim=-1).values.clamp(min=0)
        tok = torch.minimum(torch.searchsorted(cum, (u * cum[:, -1])[:, None], right=True).squeeze(-1), last)
        kept = keep.sum(-1)
    tok = torch.where(live, tok, torch.zeros_like(tok))
    kept = torch.where(live, kept, torch.zeros_like(kept))
    was_done = state.done != 0
    tok = torch.where(was_done, torch.full_like(tok, pad), tok)
    kept = torch.where(was_done, torch.zeros_like(kept), kept)
    state.tokens.copy_(tok)
    state.kept.copy_(kept.to(torch.int32))
    if state.out is not None:
        for b in range(B):
            n = int(state.draws[b])
            if 0 <= n < state.out.shape[1]:
                state.out[b, n] = tok[b]
    if eos >= 0:
        state.done |= (tok == eos).to(torch.uint8)
    state.draws += 1


def sample_tokens(logits, state, *, return_kept=False):
    """Next tokens int64 [B] from logits [B, V] (fp32 or bf16, unit last stride, any row stride) under the settings
    of `state` (SamplerState): temperature, then top-k, then top-p (HF's warper order, ties at either threshold
    kept), then a Philox draw with counter (row, state.draws[row]); argmax (lowest index on ties) at temperature 0.
    NaN counts as -inf, +inf as the largest finite fp32; a row with no finite logit yields token 0 (kept 0). A row
    whose state.done is set yields the pad token; a drawn EOS sets it. Step n writes column n of state.out.

    One pico_sample launch for HIP tensors, no host synchronisation; for CPU tensors the plain-torch restatement.
    Returns state.tokens (and state.kept with return_kept): the state's own buffers, overwritten by the next call."""
    if not isinstance(state, SamplerState):
        raise TypeError("sample_tokens: state must be a SamplerState")
    if logits.dim() != 2 or logits.shape[0] != state.batch or logits.shape[1] < 1:
        raise ValueError(f"sample_tokens: logits must be [batch = {state.batch}, vocab]")
    if logits.device != state.device:
        raise ValueError(f"sample_tokens: logits on {logits.device}, the state on {state.device}")
    B, V = logits.shape
    if V > 1 and logits.stride(1) != 1:
        raise ValueError("sample_tokens: logits rows must be unit-stride")
    if logits.device.type == "cpu":
        if not logits.dtype.is_floating_point:
            raise TypeError("sample_tokens: logits must be floating point")
        _sample_reference(logits, state)
    else:
        if logits.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"sample_tokens: {logits.dtype} logits on {logits.device}: the kernel takes fp32 or bf16 "
                            "(there is no eager path on the device)")
        out = state.out
        _lib.check(_lib.load().pico_sample(
            _lib.ptr(logits), 0 if logits.dtype == torch.float32 else 1, logits.stride(0), B, V,
            _lib.ptr(state.params), _lib.ptr(state.draws), _lib.ptr(state.done), _lib.ptr(state.tokens),
            _lib.ptr(out), out.stride(0) if out is not None else 0, out.shape[1] if out is not None else 0,
            _lib.ptr(state.kept), _lib.stream_of(logits)), "pico_sample")
    return (state.tokens, state.kept) if return_kept else state.tokens


class _DecodeGraph:
    """One captured decode iteration: decode_step(model, state.tokens, cache) then sample_tokens, on the state's
    static buffers. key: the batch and the data pointers the graph has baked in. It holds what those pointers point
    into and no one else keeps alive: the sampler state, the static logits, and the decode attention workspace that
    was current at capture (_WORKSPACES replaces its entry when a larger one is needed; the graph keeps its own)."""

    def __init__(self, key, model, graph, state, logits, workspace):
        self.key, self.model, self.graph, self.state, self.logits = key, model, graph, state, logits
        self.workspace = workspace

    def fits(self, model, key):
        return self.model is model and self.key == key + (self.workspace.data_ptr(),)


def _graph_key(model, cache):
    ptrs = [cache.lens.data_ptr(), model.embedding.weight.data_ptr(), model.final_norm.weight.data_ptr(),
            model.final_proj.weight.data_ptr()]
    for entry in cache._plan:
        ptrs.extend(t.data_ptr() for t in entry if isinstance(t, torch.Tensor))
    return (cache.batch, tuple(ptrs))


def _capture_stream(device):
    """The stream torch.cuda.graph captures on by default, created here if no capture has run yet: the warm-up
    iteration runs on it, so that decode_step's workspace (keyed by stream) and the GEMM library's exist before the
    capture and are the ones the graph bakes in."""
    if torch.cuda.graph.default_capture_stream is None:
        with torch.cuda.device(device):
            torch.cuda.graph.default_capture_stream = torch.cuda.Stream()
    return torch.cuda.graph.default_capture_stream


def _generate_cache(model, input_ids, max_new_tokens, cache, kv_dtype=None):
    """generate()'s checks of its arguments, and the cache it runs on: the caller's, reset, or a new one of exactly
    the needed length."""
    _check_model(model)
    if input_ids.dim() != 2:
        raise ValueError("generate: input_ids must be [batch, tokens]")
    if max_new_tokens < 1:
        raise ValueError("generate: max_new_tokens must be >= 1")
    B, T = input_ids.shape
    need = T + max_new_tokens
    if cache is None:
        if need > model.max_position_embeddings:
            raise ValueError(f"generate: prompt {T} + {max_new_tokens} new tokens exceed the model's "
                             f"max_position_embeddings {model.max_position_embeddings}")
        return KVCache(model, B, need, device=input_ids.device, kv_dtype=kv_dtype)
    _check_cache(model, cache, B)
    if kv_dtype is not None and cache.kv_dtype != kv_dtype:
        raise ValueError(f"generate: kv_dtype {kv_dtype} does not match the given cache's {cache.kv_dtype}")
    if need > cache.max_len:
        raise ValueError(f"generate: prompt {T} + {max_new_tokens} new tokens exceed the cache's max_len "
                         f"{cache.max_len}")
    cache.reset()
    return cache


def _generate_fused(model, input_ids, max_new_tokens, prompt_lens, temperature, top_k, top_p, eos_token_id,
                    pad_token_id, seed, return_logits, cache, graph, skinny_linear=False, decode_weights=None,
                    kv_dtype=None):
    cache = _generate_cache(model, input_ids, max_new_tokens, cache, kv_dtype)
    B, N = input_ids.shape[0], max_new_tokens
    dev = input_ids.device
    settings = dict(temperature=temperature, top_k=top_k, top_p=top_p, eos_token_id=eos_token_id,
                    pad_token_id=pad_token_id, seed=seed)
    keep = torch.empty((B, N, model.vocab_size), dtype=torch.float32, device=dev) if return_logits else None
    logits = prefill(model, input_ids, cache, prompt_lens)
    if keep is not None:
        keep[:, 0] = logits
    if not graph:
        state = SamplerState(B, dev, out=torch.empty((B, N), dtype=torch.int64, device=dev), **settings)
        sample_tokens(logits, state)
        for step in range(1, N):
            logits = decode_step(model, state.tokens, cache, skinny_linear, decode_weights)
            if keep is not None:
                keep[:, step] = logits
            sample_tokens(logits, state)
        return (state.out, keep) if return_logits else state.out

    from .train import _capturing
    key = _graph_key(model, cache) + (bool(skinny_linear),)  # a graph replays the route it was captured with
    if decode_weights is not None:  # ... and the FP8 weights: the held graph keeps the object, so its id stays its own
        key += (id(decode_weights),)
    held = cache._graph if cache._graph is not None and cache._graph.fits(model, key) else None
    if held is not None:
        state = held.state.set(**settings).reset()
    else:  # the graph writes column n of a static out as wide as the cache: any later call's tokens fit
        state = SamplerState(B, dev, out=torch.empty((B, cache.max_len), dtype=torch.int64, device=dev), **settings)
    sample_tokens(logits, state)
    first = 1
    if held is None and N > 1:
        # one eager iteration on the capture stream (it is generated token 1), then the capture of the same two calls
        cache._graph = None
        side = _capture_stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            logits = decode_step(model, state.tokens, cache, skinny_linear, decode_weights)
            sample_tokens(logits, state)
        torch.cuda.current_stream(dev).wait_stream(side)
        if keep is not None:
            keep[:, 1] = logits
            logits.record_stream(torch.cuda.current_stream(dev))  # allocated on `side`, read here
        g = torch.cuda.CUDAGraph()
        with _capturing(g):
            static_logits = decode_step(model, state.tokens, cache, skinny_linear, decode_weights)
            sample_tokens(static_logits, state)
        # the workspace the two passes above used on this stream (decode attention's and decode_linear's partials):
        # the graph points into it, so the graph holds it; a later, larger request replaces the dict's entry, not
        # this tensor
        workspace = _WORKSPACES[(static_logits.device, side.cuda_stream)]
        held = cache._graph = _DecodeGraph(key + (workspace.data_ptr(),), model, g, state, static_logits, workspace)
        held.decode_weights = decode_weights
        cache.graph_captures += 1
        first = 2
    for step in range(first, N):
        held.graph.replay()
        if keep is not None:
            keep[:, step] = held.logits
    out = state.out[:, :N].clone()
    return (out, keep) if return_logits else out


@torch.no_grad()
def generate(model, input_ids, max_new_tokens, prompt_lens=None, temperature=0.0, top_k=None, eos_token_id=None,
             pad_token_id=0, generator=None, return_logits=False, cache=None, top_p=None, seed=None, graph=False,
             skinny_linear=False, decode_weights=None, kv_dtype=None):
    """Sample max_new_tokens tokens per row after the (right-padded) prompts: int64 [B, max_new_tokens], and with
    return_logits the fp32 [B, max_new_tokens, V] each token was drawn from. One prefill, then max_new_tokens - 1
    decode steps. A row that has emitted eos_token_id yields pad_token_id from then on (masked on the device; no
    early exit, no per-step synchronisation). cache: a KVCache to reuse (reset here), else one of exactly the
    needed length is allocated.

    top_p, seed or graph=True select the fused device sampler (sample_tokens: one launch per token, temperature /
    top_k / top_p in HF's order, Philox draws keyed by `seed`, default torch.initial_seed(); the tokens are a pure
    function of the logits and the seed). graph=True also captures one decode iteration (decode_step + the sampler)
    as a HIP graph and replays it per token; the graph lives on `cache` and is reused by later calls with the same
    model and batch, whatever their settings. generator= belongs to the default path only.

    skinny_linear=True (batch <= 16, refused beyond) runs every decode step's projections on ops.decode_linear
    (decode_step); the prefill is untouched. A captured graph is captured with, and keyed by, the setting.

    decode_weights (quantize_decode_weights(model), with skinny_linear=True only): the decode steps' projections
    stream FP8 (e4m3) weights, half the bytes of the bf16 ones. Prefill keeps running on the bf16 weights and the
    training kernels: the prompt's K/V come from the bf16 weights, the generated tokens' from the FP8 ones. The
    object is a snapshot of the model's weights; a captured graph is keyed by its identity as well.

    kv_dtype=torch.float8_e4m3fn: the cache generate() allocates is an FP8 KVCache (about half the K / V bytes per
    decode step); with cache= given it must match that cache's. The prompt is attended on the bf16 K / V."""
    if decode_weights is not None:
        _check_decode_weights(model, decode_weights, skinny_linear)
    if skinny_linear:
        _check_skinny(model, input_ids.shape[0] if input_ids.dim() == 2 else 1)
    if top_p is not None or seed is not None or graph:
        if generator is not None:
            raise ValueError("generate: generator= cannot be combined with top_p / seed / graph (the fused sampler "
                             "draws from its seed)")
        return _generate_fused(model, input_ids, max_new_tokens, prompt_lens, temperature, top_k, top_p,
                               eos_token_id, pad_token_id, seed, return_logits, cache, graph, skinny_linear,
                               decode_weights, kv_dtype)
    cache = _generate_cache(model, input_ids, max_new_tokens, cache, kv_dtype)
    B = input_ids.shape[0]
    dev = input_ids.device
    out = torch.empty((B, max_new_tokens), dtype=torch.int64, device=dev)
    keep = torch.empty((B, max_new_tokens, model.vocab_size), dtype=torch.float32, device=dev) if return_logits \
        else None
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    logits = prefill(model, input_ids, cache, prompt_lens)
    for step in range(max_new_tokens):
        if step:
            logits = decode_step(model, tok, cache, skinny_linear, decode_weights)
        if keep is not None:
            keep[:, step] = logits
        tok = sample_next(logits, temperature, top_k, generator)
        if eos_token_id is not None:
            tok = torch.where(done, torch.full_like(tok, pad_token_id), tok)
            done = done | (tok == eos_token_id)
        out[:, step] = tok
    return (out, keep) if return_logits else out
