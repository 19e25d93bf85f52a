"""Multi-token extend measurements (picotron_amd/generate.py: attention_extend, extend_step). Needs a HIP device;
reads nothing outside the repository.

  kernels  pico_attn_extend (chunk kernel + combine) for T in {4, 8, 16} beside T calls of pico_attn_decode at the
           same lengths (query t of the extend call sees ctx - (T - 1 - t) keys; decode call t the same), at
           (Hq, Hkv, D) = (32, 32, 64) and (32, 8, 128), B in {1, 8}, ctx in {2048, 8192}. The launches rotate over
           enough copies of the cache (>= --rotate-mb in total) that K / V come from HBM. Kernel time is the
           library's per-launch events (pico_prof_*: the dispatch packet's timestamps, what a kernel trace reports),
           both kernels of a call added, each form in a pass of its own; run the script under
           `rocprofv3 --kernel-trace --stats -- python scripts/extend_bench.py kernels` for the trace's own table.
           One JSON line per shape: us per extend call, us of the T decode calls, the algorithmic bytes of the
           extend call (K + V of the context once, q, O) over its time as GB/s and as a share of the 8 TB/s HBM peak,
           and its MFMA flops (4 rows ctx D, padding rows not counted) over its time.
  e2e      SmolLM-1.7B geometry, --layers layers (15), B in {1, 8}, a 128-token prompt: ms per extend_step(T), T in
           {4, 8, 16}, beside T x ms per eager decode_step, alternated in one process for --rounds rounds (host clock
           ending in a synchronise; every timed call rewinds the cache to the prompt first, on the device).

Usage: python scripts/extend_bench.py kernels|e2e [--out profiles/extend_bench.jsonl] [--iters 100] [--rounds 5]
"""
import argparse
import math
import os
import sys

import torch

from decode_bench import HBM_PEAK_GBS, ROOT, _clock_ms, _emit


def _kernel_us(L, fn, iters, calls):
    """us per fn(i): the chunk and combine kernels of its `calls` launches each, from the per-launch events."""
    for kid in (L.K_ATTN_FWD, L.K_ATTN_MERGE):
        L.prof_enable(kid, iters * calls)
    for i in range(iters):
        fn(i)
    tot = 0.0
    for kid in (L.K_ATTN_FWD, L.K_ATTN_MERGE):
        ms, cnt = L.prof_collect(kid)
        assert cnt == iters * calls, (kid, cnt)
        tot += ms
    L.load().pico_prof_enable(0, 0)
    return 1e3 * tot / iters


def kernels(args):
    from picotron_amd import _lib as L
    from picotron_amd import generate as G
    dev = torch.device("cuda", 0)
    for Hq, Hkv, D in ((32, 32, 64), (32, 8, 128)):
        for B in (1, 8):
            for ctx in (2048, 8192):
                kv_bytes = 2 * B * Hkv * ctx * D * 2
                nbuf = max(1, min(64, math.ceil(args.rotate_mb * (1 << 20) / kv_bytes)))
                k = torch.empty(nbuf, B, Hkv, ctx, D, device=dev, dtype=torch.bfloat16).normal_()
                v = torch.empty(nbuf, B, Hkv, ctx, D, device=dev, dtype=torch.bfloat16).normal_()
                scale = 1.0 / math.sqrt(D)
                for T in (4, 8, 16):
                    q = torch.randn(B, T, Hq, D, device=dev).to(torch.bfloat16)
                    lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
                    lens_t = [lens - (T - 1 - t) for t in range(T)]

                    def extend(i):
                        return G.attention_extend(q, k[i % nbuf], v[i % nbuf], lens, softmax_scale=scale)

                    def decode(i):
                        return [G.attention_decode(q[:, t], k[i % nbuf], v[i % nbuf], lens_t[t], softmax_scale=scale)
                                for t in range(T)]

                    diff = float((extend(0).float() - torch.stack(decode(0), 1).float()).abs().max())
                    for i in range(max(nbuf, 8)):
                        extend(i), decode(i)
                    ext = sorted(_kernel_us(L, extend, args.iters, 1) for _ in range(args.rounds))
                    dec = sorted(_kernel_us(L, decode, args.iters, T) for _ in range(args.rounds))
                    e_us, d_us = ext[len(ext) // 2], dec[len(dec) // 2]
                    algo = kv_bytes + 2 * B * T * Hq * D * 2
                    flops = 4 * B * T * Hq * ctx * D
                    _emit(args, {"mode": "kernels", "Hq": Hq, "Hkv": Hkv, "D": D, "B": B, "context": ctx, "T": T,
                                 "query_rows_per_kv_head": T * Hq // Hkv, "cache_copies": nbuf,
                                 "split_keys": G.default_extend_split_keys(B, T, Hq, Hkv, ctx, D),
                                 "extend_kernels_us_rounds": [round(x, 2) for x in ext],
                                 "decode_xT_kernels_us_rounds": [round(x, 2) for x in dec],
                                 "extend_kernels_us": round(e_us, 2), "decode_xT_kernels_us": round(d_us, 2),
                                 "decode_xT_over_extend": round(d_us / e_us, 2), "algorithmic_bytes": algo,
                                 "extend_GB_s": round(algo / e_us / 1e3, 1),
                                 "extend_frac_of_8TBs": round(algo / e_us / 1e3 / HBM_PEAK_GBS, 4),
                                 "extend_TFLOP_s": round(flops / e_us / 1e6, 2), "max_abs_diff_vs_decode": diff})
                del k, v


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
    P, reps = 128, 8
    for B in (1, 8):
        prompt = torch.randint(0, cfg.vocab_size, (B, P), generator=torch.Generator().manual_seed(B)).to(dev)
        cache = G.KVCache(model, B, P + 16)
        G.prefill(model, prompt, cache)
        for T in (4, 8, 16):
            tok = torch.randint(0, cfg.vocab_size, (B, T), generator=torch.Generator().manual_seed(T)).to(dev)

            def extend():
                for _ in range(reps):
                    G.extend_step(model, tok, cache)
                    cache.rewind(T)

            def decode():
                for _ in range(reps):
                    for t in range(T):
                        G.decode_step(model, tok[:, t], cache)
                    cache.rewind(T)

            forms = {"extend": extend, "decode": decode}
            for fn in forms.values():
                _clock_ms(fn)
            ms = {name: [] for name in forms}
            for _ in range(args.rounds):
                for name, fn in forms.items():
                    ms[name].append(_clock_ms(fn) / reps)
            med = {name: sorted(x)[len(x) // 2] for name, x in ms.items()}
            _emit(args, {"mode": "e2e", "model": f"SmolLM-1.7B geometry, {args.layers} layers", "B": B, "prompt": P,
                         "T": T, "extend_step_ms_rounds": [round(x, 3) for x in ms["extend"]],
                         "decode_steps_xT_ms_rounds": [round(x, 3) for x in ms["decode"]],
                         "extend_step_ms": round(med["extend"], 3), "decode_steps_xT_ms": round(med["decode"], 3),
                         "decode_xT_over_extend": round(med["decode"] / med["extend"], 2)})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "e2e"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extend_bench.jsonl"),
                    help="append the JSON lines to this file")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=15)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("extend_bench: needs a HIP device (no measurement without one)")
    {"kernels": kernels, "e2e": e2e}[a.mode](a)
