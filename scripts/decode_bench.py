"""KV-cache generation measurements (picotron_amd/generate.py). Needs a HIP device; reads nothing outside the
repository.

  kernels  attention_decode (pico_attn_decode: the chunk kernel + the combine kernel) at (Hq, Hkv, D) = (32, 32, 64)
           and (32, 8, 128), B in {1, 8, 32}, context in {1024, 8192} (cache length = context, every row full), and
           torch.nn.functional.scaled_dot_product_attention on the same cache views, alternated for --rounds rounds.
           Device events around --iters launches after warm-up; the launches rotate over enough copies of the cache
           (>= --rotate-mb in total) that K / V come from HBM, as they do between the layers of a model, not from
           the 256 MB last-level cache. One JSON line per shape: us per call for both, the algorithmic bytes (K + V
           of the live context, q, O) over the time, as GB/s and as a share of the 8 TB/s HBM peak, the default
           split, and, from a pass of its own with the library's per-launch events (pico_prof_*), the time of the
           two kernels alone with the same two rates.
  e2e      SmolLM-1.7B geometry, --layers layers (15), B in {1, 8}, a 128-token prompt, 128 new tokens, greedy:
           generate() against what the training forward alone offers, model(prefix) recomputed for every token
           (host clock around the whole loop, ending in a synchronise, after one warm pass of each). Reports ms per
           generated token for both, prefill and decode step separately, and the floor of streaming the weights
           (decoder matrices + LM head, bf16) once per step at 8 TB/s.

Usage: python scripts/decode_bench.py kernels|e2e [--out profiles/decode_bench.jsonl] [--iters 200] [--rounds 3]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (8 TB/s)


def _log(msg):
    print(f"[decode_bench] {msg}", file=sys.stderr, flush=True)


def _emit(args, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def _events_us(fn, iters):
    """us per call: device events around `iters` calls (fn(i) enqueues call i)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def kernels(args):
    import torch.nn.functional as F
    from picotron_amd import _lib as L
    from picotron_amd import generate as G
    dev = torch.device("cuda", 0)
    for Hq, Hkv, D in ((32, 32, 64), (32, 8, 128)):
        for B in (1, 8, 32):
            for ctx in (1024, 8192):
                kv_bytes = 2 * B * Hkv * ctx * D * 2
                nbuf = max(1, min(64, math.ceil(args.rotate_mb * (1 << 20) / kv_bytes)))
                k = torch.empty(nbuf, B, Hkv, ctx, D, device=dev, dtype=torch.bfloat16).normal_()
                v = torch.empty(nbuf, B, Hkv, ctx, D, device=dev, dtype=torch.bfloat16).normal_()
                q = torch.randn(B, Hq, D, device=dev).to(torch.bfloat16)
                lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
                scale = 1.0 / math.sqrt(D)

                def ours(i):
                    G.attention_decode(q, k[i % nbuf], v[i % nbuf], lens, softmax_scale=scale)

                q4 = q.view(B, Hq, 1, D)
                sdpa_form = "enable_gqa" if Hq != Hkv else "plain"

                def sdpa(i):
                    F.scaled_dot_product_attention(q4, k[i % nbuf], v[i % nbuf], scale=scale,
                                                   **({"enable_gqa": True} if Hq != Hkv else {}))

                forms = {"pico": ours}
                try:
                    o_ref = F.scaled_dot_product_attention(q4, k[0], v[0], scale=scale,
                                                           **({"enable_gqa": True} if Hq != Hkv else {}))
                    torch.cuda.synchronize()
                    forms["sdpa"] = sdpa
                    o = G.attention_decode(q, k[0], v[0], lens, softmax_scale=scale)
                    diff = float((o.float() - o_ref.view(B, Hq, D).float()).abs().max())
                except Exception as e:  # the comparison is optional; the kernel row is not
                    _log(f"SDPA unavailable at this shape: {e!r}")
                    sdpa_form, diff = f"failed: {type(e).__name__}", None
                for fn in forms.values():  # warm-up of every buffer the window touches
                    for i in range(max(nbuf, 8)):
                        fn(i)
                us = {name: [] for name in forms}
                for _ in range(args.rounds):
                    for name, fn in forms.items():
                        us[name].append(_events_us(fn, args.iters))
                med = {name: sorted(x)[len(x) // 2] for name, x in us.items()}
                algo = kv_bytes + 2 * B * Hq * D * 2
                # the two kernels alone: the library's per-launch events (dispatch timestamps), in a pass of its own
                kern = {}
                for kid in (L.K_ATTN_FWD, L.K_ATTN_MERGE):
                    L.prof_enable(kid, args.iters)
                for i in range(args.iters):
                    ours(i)
                for kid, name in ((L.K_ATTN_FWD, "chunk_kernel_us"), (L.K_ATTN_MERGE, "combine_kernel_us")):
                    tot, cnt = L.prof_collect(kid)
                    assert cnt == args.iters, (name, cnt)
                    kern[name] = 1e3 * tot / cnt
                L.load().pico_prof_enable(0, 0)
                kus = kern["chunk_kernel_us"] + kern["combine_kernel_us"]
                rec = {"mode": "kernels", "Hq": Hq, "Hkv": Hkv, "D": D, "B": B, "context": ctx,
                       "split_keys": G.default_split_keys(B, Hkv, ctx, D), "cache_copies": nbuf,
                       "algorithmic_bytes": algo, "pico_us_rounds": [round(x, 2) for x in us["pico"]],
                       "pico_us": round(med["pico"], 2), "pico_GB_s": round(algo / (med["pico"] * 1e-6) / 1e9, 1),
                       "pico_frac_of_8TBs": round(algo / (med["pico"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                       "chunk_kernel_us": round(kern["chunk_kernel_us"], 2),
                       "combine_kernel_us": round(kern["combine_kernel_us"], 2),
                       "kernels_GB_s": round(algo / (kus * 1e-6) / 1e9, 1),
                       "kernels_frac_of_8TBs": round(algo / (kus * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                       "sdpa_form": sdpa_form, "max_abs_diff_vs_sdpa": diff}
                if "sdpa" in med:
                    rec.update({"sdpa_us_rounds": [round(x, 2) for x in us["sdpa"]], "sdpa_us": round(med["sdpa"], 2),
                                "sdpa_over_pico": round(med["sdpa"] / med["pico"], 3)})
                _emit(args, rec)
                del k, v


def _clock_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def e2e(args):
    from picotron_amd import generate as G
    from picotron_amd.model import build_llama, smollm_1_7b
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = smollm_1_7b(num_hidden_layers=args.layers, seq_length=2048)
    torch.manual_seed(0)
    model = build_llama(cfg, device=dev)
    with torch.no_grad():
        model.final_proj.weight.normal_(0.0, 0.02)
    weights = sum(p.numel() for layer in model.decoder_layers for p in layer.parameters() if p.dim() == 2)
    weights += model.final_proj.weight.numel()
    floor_ms = 1e3 * weights * 2 / (HBM_PEAK_GBS * 1e9)
    P, N = 128, 128
    for B in (1, 8):
        prompt = torch.randint(0, cfg.vocab_size, (B, P), generator=torch.Generator().manual_seed(B)).to(dev)
        cache = G.KVCache(model, B, P + N)
        out = {}

        def ours():
            out["pico"] = G.generate(model, prompt, N, cache=cache)

        @torch.no_grad()
        def recompute():
            ids = prompt
            for _ in range(N):
                nxt = model(ids)[:, -1].float().argmax(-1)
                ids = torch.cat([ids, nxt[:, None]], 1)
            out["recompute"] = ids[:, P:]

        def prefill_only():
            cache.reset()
            G.prefill(model, prompt, cache)

        tok = torch.zeros(B, dtype=torch.int64, device=dev)

        def steps_only():  # N - 1 decode steps from a prefilled cache
            prefill_only()
            for _ in range(N - 1):
                G.decode_step(model, tok, cache)

        forms = {"pico": ours, "recompute": recompute, "prefill": prefill_only, "prefill_plus_steps": steps_only}
        for name, fn in forms.items():  # one warm pass: code objects, GEMM algorithms of every shape
            _clock_ms(fn)
            _log(f"B={B} warm {name} done")
        ms = {name: [] for name in forms}
        for _ in range(args.rounds):
            for name, fn in forms.items():
                ms[name].append(_clock_ms(fn))
        med = {name: sorted(x)[len(x) // 2] for name, x in ms.items()}
        step_ms = (med["prefill_plus_steps"] - med["prefill"]) / (N - 1)
        agree = float((out["pico"] == out["recompute"]).float().mean())
        _emit(args, {"mode": "e2e", "model": f"SmolLM-1.7B geometry, {args.layers} layers", "B": B, "prompt": P,
                     "new_tokens": N, "pico_ms_rounds": [round(x, 1) for x in ms["pico"]],
                     "pico_ms_per_token": round(med["pico"] / N, 3),
                     "recompute_ms_rounds": [round(x, 1) for x in ms["recompute"]],
                     "recompute_ms_per_token": round(med["recompute"] / N, 3),
                     "recompute_over_pico": round(med["recompute"] / med["pico"], 2),
                     "prefill_ms": round(med["prefill"], 3), "decode_step_ms": round(step_ms, 3),
                     "weight_bytes_per_step": weights * 2, "weights_floor_ms_per_step": round(floor_ms, 4),
                     "decode_step_over_floor": round(step_ms / floor_ms, 2),
                     "greedy_tokens_equal_fraction": round(agree, 4)})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "e2e"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_bench.jsonl"),
                    help="append the JSON lines to this file")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=15)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_bench: needs a HIP device (no measurement without one)")
    kernels(a) if a.mode == "kernels" else e2e(a)
