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

MAX_GROUP = 8  # query heads per kv head the decode kernel serves (csrc/attn_decode_plan.h DEC_MAX_GROUP)


def _check_caches(k_cache, v_cache, B, D):
    for t, n in ((k_cache, "k_cache"), (v_cache, "v_cache")):
        if t.dim() != 4 or t.stride(-1) != 1:
            raise ValueError(f"{n} must be [batch, kv_heads, max_len, head_dim] with unit last stride")
    if k_cache.shape != v_cache.shape or k_cache.shape[0] != B or k_cache.shape[3] != D:
        raise ValueError(f"cache shapes {tuple(k_cache.shape)} / {tuple(v_cache.shape)} do not fit batch {B}, "
                         f"head_dim {D}")


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


def kv_cache_append(qkv, cos, sin, pos, k_cache, v_cache, num_heads, num_kv_heads):
    """RoPE + KV-cache write for the fused q|k|v projection output `qkv` [B, T, (Hq + 2 Hkv) D].

    With p = pos[b] + t (pos: int32 [B] on qkv's device): q[b, t] is rotated IN PLACE with row p of cos / sin
    ([rows, >= D/2] tables), k[b, t] is rotated with row p and stored at k_cache[b, :, p, :], v[b, t] is copied to
    v_cache[b, :, p, :]. Caches are [B, Hkv, S_max, D] views (unit last stride, other strides multiples of 8). A
    token with p >= S_max, or beyond the tables, is skipped whole. Returns the q view [B, T, Hq, D] of qkv."""
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
    if qkv.device.type == "cpu":
        _kv_append_reference(qkv, cos, sin, pos, k_cache, v_cache, Hq, Hkv)
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


def attention_decode(q, k_cache, v_cache, seqlens, softmax_scale=None, split_keys=None, return_lse=False):
    """softmax(scale q K^T) V for one query per sequence against a head-major cache.

    q [B, Hq, D] (unit last stride; a view of the projection output is fine), k_cache / v_cache [B, Hkv, S_max, D],
    seqlens int32 [B] on q's device: row b attends to keys [0, min(seqlens[b], S_max)). Returns O [B, Hq, D] in q's
    dtype (and LSE [B, Hq] fp32, natural log, with return_lse). seqlens[b] = 0 gives O = 0, LSE = -inf. Hq / Hkv
    may be 1..8. split_keys: keys per chunk of the split (None: the library's host rule, which never reads the
    device lengths); the result is deterministic for a given split_keys and independent of the other rows."""
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
    if q.device.type == "cpu":
        o, lse = _decode_reference(q, k_cache, v_cache, seqlens, scale, split_keys)
        return (o, lse) if return_lse else o
    for t, n in ((q, "q"), (k_cache, "k_cache"), (v_cache, "v_cache")):
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
    _lib.check(lib.pico_attn_decode(_lib.ptr(q), qs, _lib.ptr(k_cache), _lib.i64x3(k_cache.stride()[:3]),
                                    _lib.ptr(v_cache), _lib.i64x3(v_cache.stride()[:3]), _lib.ptr(seqlens),
                                    _lib.ptr(o), _lib.ptr(lse), _lib.ptr(ws), B, Hq, Hkv, S, D, scale, sk,
                                    _lib.stream_of(q)), "pico_attn_decode")
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
    [batch] on the device (tokens held per row)."""

    def __init__(self, model, batch, max_len, device=None):
        _check_model(model)
        if max_len > model.max_position_embeddings:
            raise ValueError(f"KVCache: max_len {max_len} exceeds the model's RoPE table "
                             f"(max_position_embeddings {model.max_position_embeddings})")
        if batch <= 0 or max_len <= 0:
            raise ValueError("KVCache: batch and max_len must be positive")
        device = torch.device(device) if device is not None else model.final_proj.weight.device
        shape = (model.num_layers, batch, model.num_key_values, max_len, model.head_dim)
        self.k = torch.zeros(shape, dtype=torch.bfloat16, device=device)
        self.v = torch.zeros(shape, dtype=torch.bfloat16, device=device)
        self.lens = torch.zeros(batch, dtype=torch.int32, device=device)
        self.batch, self.max_len = batch, max_len
        self._plan, self._plan_model = None, None  # prefill's per-layer table (_layer_plan)
        self._graph, self.graph_captures = None, 0  # generate(graph=True)'s captured iteration (_DecodeGraph)

    def reset(self):
        self.lens.zero_()


def _layer_plan(model, cache, dev):
    """What a pass over the decoder stack reads, gathered once per prefill (a decode step then spends no host time on
    it): per layer the norm weights, the stacked q|k|v and gate|up weights (ops.stacked_weight: the parameters
    themselves, no copy), the other two projections, the RoPE tables and the layer's cache views."""
    plan = []
    for i, layer in enumerate(model.decoder_layers):
        a, f = layer.attention, layer.mlp
        if layer.cos.device != dev:  # the layers build their tables on the device of construction
            layer.cos, layer.sin = layer.cos.to(dev), layer.sin.to(dev)
        plan.append((layer.input_layernorm.weight, layer.input_layernorm.eps,
                     ops.stacked_weight((a.q_proj.weight, a.k_proj.weight, a.v_proj.weight)), a.out_proj.weight,
                     layer.post_attention_layernorm.weight, layer.post_attention_layernorm.eps,
                     ops.stacked_weight((f.gate_proj.weight, f.up_proj.weight)), f.down_proj.weight,
                     layer.cos, layer.sin, cache.k[i], cache.v[i]))
    cache._plan, cache._plan_model = plan, model
    return plan


def _layers(model, plan, x, pos, attend):
    """The decoder stack on x [B, T, hidden] with the residual adds fused into the norms, exactly the training
    forward's rounding points. attend(q, k_cache, v_cache) -> [B, T, Hq * D], after kv_cache_append wrote the
    cache."""
    Hq, Hkv = model.num_heads, model.num_key_values
    B, T = x.shape[:2]
    linear = torch.nn.functional.linear
    delta, residual = x, None
    for w_in, eps_in, w_qkv, w_out, w_post, eps_post, w_gu, w_down, cos, sin, kc, vc in plan:
        h, residual = ops.rms_norm(delta, w_in, eps_in, residual=residual, prenorm=True)
        q = kv_cache_append(linear(h, w_qkv), cos, sin, pos, kc, vc, Hq, Hkv)
        h2, residual = ops.rms_norm(linear(attend(q, kc, vc), w_out), w_post, eps_post, residual=residual,
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


def _check_cache(model, cache, B):
    if not isinstance(cache, KVCache) or cache.batch != B or cache.k.shape[0] != model.num_layers:
        raise ValueError("generate: the cache does not fit this model / batch")


@torch.no_grad()
def prefill(model, input_ids, cache, prompt_lens=None):
    """Run the prompts through the model and fill `cache` from position 0: returns the fp32 logits [B, V] of each
    row's last prompt token. input_ids [B, T] is right-padded to a common length; prompt_lens (int tensor or list,
    default T for every row) gives the rows' true lengths. The padding positions are written to the cache too, but
    lie at or beyond the row's length: decode steps overwrite them before they can be read."""
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
    Hq, D = model.num_heads, model.head_dim
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    scale = 1.0 / math.sqrt(D)

    def attend(q, kc, vc):
        o, _ = ops.attention_block_fwd(q, kc.transpose(1, 2)[:, :T], vc.transpose(1, 2)[:, :T], scale, True)
        return o.view(B, T, Hq * D)

    x = torch.nn.functional.embedding(input_ids, model.embedding.weight)
    delta, residual = _layers(model, _layer_plan(model, cache, dev), x, pos, attend)
    last = (lens.to(torch.int64) - 1).clamp(0, T - 1)
    rows = torch.arange(B, device=dev)
    logits = _head(model, delta[rows, last], residual[rows, last] if residual is not None else None)
    cache.lens.copy_(lens.clamp(0, T))
    return logits


@torch.no_grad()
def decode_step(model, tokens, cache):
    """One token per row: tokens int64 [B] -> fp32 logits [B, V] of the next token; the cache grows by one. No host
    synchronisation: the positions are cache.lens on the device. A row whose cache is full writes nothing and
    attends to the full cache (generate() refuses lengths that would get there)."""
    if tokens.dim() != 1:
        raise ValueError("decode_step: tokens must be [batch]")
    B = tokens.shape[0]
    plan = cache._plan if isinstance(cache, KVCache) and cache._plan_model is model else None
    if plan is None:  # a cache this model has not prefilled: the full checks, once
        _check_model(model)
        _check_cache(model, cache, B)
        plan = _layer_plan(model, cache, tokens.device)
    elif cache.batch != B:
        raise ValueError("generate: the cache does not fit this model / batch")
    Hq, D = model.num_heads, model.head_dim
    seqlens = cache.lens + 1

    def attend(q, kc, vc):
        return attention_decode(q.view(B, Hq, D), kc, vc, seqlens).view(B, 1, Hq * D)

    x = torch.nn.functional.embedding(tokens.view(B, 1), model.embedding.weight)
    delta, residual = _layers(model, plan, x, cache.lens, attend)
    logits = _head(model, delta[:, 0], residual[:, 0] if residual is not None else None)
    cache.lens += 1
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


def _generate_cache(model, input_ids, max_new_tokens, cache):
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
        return KVCache(model, B, need, device=input_ids.device)
    _check_cache(model, cache, B)
    if need > cache.max_len:
        raise ValueError(f"generate: prompt {T} + {max_new_tokens} new tokens exceed the cache's max_len "
                         f"{cache.max_len}")
    cache.reset()
    return cache


def _generate_fused(model, input_ids, max_new_tokens, prompt_lens, temperature, top_k, top_p, eos_token_id,
                    pad_token_id, seed, return_logits, cache, graph):
    cache = _generate_cache(model, input_ids, max_new_tokens, cache)
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
            logits = decode_step(model, state.tokens, cache)
            if keep is not None:
                keep[:, step] = logits
            sample_tokens(logits, state)
        return (state.out, keep) if return_logits else state.out

    from .train import _capturing
    key = _graph_key(model, cache)
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
            logits = decode_step(model, state.tokens, cache)
            sample_tokens(logits, state)
        torch.cuda.current_stream(dev).wait_stream(side)
        if keep is not None:
            keep[:, 1] = logits
            logits.record_stream(torch.cuda.current_stream(dev))  # allocated on `side`, read here
        g = torch.cuda.CUDAGraph()
        with _capturing(g):
            static_logits = decode_step(model, state.tokens, cache)
            sample_tokens(static_logits, state)
        # the workspace the two passes above used on this stream (decode attention's partials): the graph points
        # into it, so the graph holds it; a later, larger request replaces the dict's entry, not this tensor
        workspace = _WORKSPACES[(static_logits.device, side.cuda_stream)]
        held = cache._graph = _DecodeGraph(key + (workspace.data_ptr(),), model, g, state, static_logits, workspace)
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
             pad_token_id=0, generator=None, return_logits=False, cache=None, top_p=None, seed=None, graph=False):
    """Sample max_new_tokens tokens per row after the (right-padded) prompts: int64 [B, max_new_tokens], and with
    return_logits the fp32 [B, max_new_tokens, V] each token was drawn from. One prefill, then max_new_tokens - 1
    decode steps. A row that has emitted eos_token_id yields pad_token_id from then on (masked on the device; no
    early exit, no per-step synchronisation). cache: a KVCache to reuse (reset here), else one of exactly the
    needed length is allocated.

    top_p, seed or graph=True select the fused device sampler (sample_tokens: one launch per token, temperature /
    top_k / top_p in HF's order, Philox draws keyed by `seed`, default torch.initial_seed(); the tokens are a pure
    function of the logits and the seed). graph=True also captures one decode iteration (decode_step + the sampler)
    as a HIP graph and replays it per token; the graph lives on `cache` and is reused by later calls with the same
    model and batch, whatever their settings. generator= belongs to the default path only."""
    if top_p is not None or seed is not None or graph:
        if generator is not None:
            raise ValueError("generate: generator= cannot be combined with top_p / seed / graph (the fused sampler "
                             "draws from its seed)")
        return _generate_fused(model, input_ids, max_new_tokens, prompt_lens, temperature, top_k, top_p,
                               eos_token_id, pad_token_id, seed, return_logits, cache, graph)
    cache = _generate_cache(model, input_ids, max_new_tokens, cache)
    B = input_ids.shape[0]
    dev = input_ids.device
    out = torch.empty((B, max_new_tokens), dtype=torch.int64, device=dev)
    keep = torch.empty((B, max_new_tokens, model.vocab_size), dtype=torch.float32, device=dev) if return_logits \
        else None
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    logits = prefill(model, input_ids, cache, prompt_lens)
    for step in range(max_new_tokens):
        if step:
            logits = decode_step(model, tok, cache)
        if keep is not None:
            keep[:, step] = logits
        tok = sample_next(logits, temperature, top_k, generator)
        if eos_token_id is not None:
            tok = torch.where(done, torch.full_like(tok, pad_token_id), tok)
            done = done | (tok == eos_token_id)
        out[:, step] = tok
    return (out, keep) if return_logits else out
