"""Generation with the fused device sampler and the replayed decode graph (picotron_amd/generate.py). Needs a HIP
device; reads nothing outside the repository.

  sampler  us per sampling step at V = 49152, B in {1, 8, 32}, fp32 logits, for greedy, top-k 50 and top-p 0.9:
           one pico_sample launch (sample_tokens) against the default path's step, sample_next plus generate()'s
           EOS masking and column store (torch launches; it has no top-p, so top-p 0.9 is compared with its plain
           temperature draw). Device events around --iters steps after warm-up, the two alternated for --rounds
           rounds, medians reported; the time of the kernel alone from the library's per-launch events.
  e2e      SmolLM-1.7B geometry, --layers layers (15), B in {1, 8}, 128-token prompt, 128 new tokens: ms per
           generated token of generate() on its default path (the loop as it was before the fused sampler), of the
           fused sampler run eagerly, and of graph=True (captured before the clock starts), greedy and with
           T 0.8 / top-k 50 / top-p 0.9; host clock around the whole call ending in a synchronise, alternated for
           --rounds rounds, medians. The decode step over the weight-streaming floor as scripts/decode_bench.py
           defines it (prefill taken from the same rounds).

Usage: python scripts/generate_bench.py sampler|e2e [--out profiles/generate_bench.jsonl] [--iters 200] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def _log(msg):
    print(f"[generate_bench] {msg}", file=sys.stderr, flush=True)


def _emit(args, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def _median(x):
    return sorted(x)[len(x) // 2]


def _events_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def _clock_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def sampler(args):
    from picotron_amd import _lib
    from picotron_amd import generate as G
    dev = torch.device("cuda", 0)
    V, COLS = 49152, 128
    settings = {"greedy": dict(temperature=0.0), "top_k50": dict(temperature=1.0, top_k=50),
                "top_p0.9": dict(temperature=1.0, top_p=0.9)}
    for B in (1, 8, 32):
        g = torch.Generator().manual_seed(B)
        # a few logit tensors in rotation, as a decode loop sees new logits every step
        logits = [(torch.randn(B, V, generator=g) * 4).to(dev) for _ in range(4)]
        for name, kw in settings.items():
            st = G.SamplerState(B, dev, eos_token_id=2, pad_token_id=0, seed=1,
                                out=torch.zeros((B, COLS), dtype=torch.int64, device=dev), **kw)

            def fused(i):
                if i % COLS == 0:
                    st.reset()
                G.sample_tokens(logits[i % 4], st)

            gen = torch.Generator(dev).manual_seed(1)
            out = torch.zeros((B, COLS), dtype=torch.int64, device=dev)
            done = [torch.zeros(B, dtype=torch.bool, device=dev)]

            def eager(i):  # generate()'s default loop body after the logits
                tok = G.sample_next(logits[i % 4], kw["temperature"], kw.get("top_k"), gen)
                tok = torch.where(done[0], torch.full_like(tok, 0), tok)
                done[0] = done[0] | (tok == 2)
                out[:, i % COLS] = tok

            for fn in (fused, eager):
                _events_us(fn, 20)
            us = {"fused": [], "eager": []}
            for _ in range(args.rounds):
                us["fused"].append(_events_us(fused, args.iters))
                us["eager"].append(_events_us(eager, args.iters))
            _lib.prof_enable(_lib.K_CE_FWD, args.iters)
            for i in range(args.iters):
                fused(i)
            torch.cuda.synchronize()
            tot_ms, n = _lib.prof_collect(_lib.K_CE_FWD)
            _lib.load().pico_prof_enable(0, 0)
            _emit(args, {"mode": "sampler", "V": V, "B": B, "setting": name,
                         "pico_sample_us_rounds": [round(x, 2) for x in us["fused"]],
                         "pico_sample_us": round(_median(us["fused"]), 2),
                         "kernel_alone_us": round(1e3 * tot_ms / max(n, 1), 2),
                         "sample_next_us_rounds": [round(x, 2) for x in us["eager"]],
                         "sample_next_us": round(_median(us["eager"]), 2),
                         "sample_next_over_pico": round(_median(us["eager"]) / _median(us["fused"]), 2)})


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
    sampled = dict(temperature=0.8, top_k=50, top_p=0.9, seed=1)
    for B in (1, 8):
        prompt = torch.randint(0, cfg.vocab_size, (B, P), generator=torch.Generator().manual_seed(B)).to(dev)
        cache = G.KVCache(model, B, P + N)
        out = {}

        def run(name, **kw):
            def fn():
                out[name] = G.generate(model, prompt, N, cache=cache, **kw)
            return fn

        def prefill_only():
            cache.reset()
            G.prefill(model, prompt, cache)

        forms = {"default_greedy": run("default_greedy"),
                 "fused_eager_greedy": run("fused_eager_greedy", seed=1),
                 "graph_greedy": run("graph_greedy", graph=True),
                 "default_top_k": run("default_top_k", temperature=0.8, top_k=50,
                                      generator=torch.Generator(dev).manual_seed(1)),
                 "fused_eager_sampled": run("fused_eager_sampled", **sampled),
                 "graph_sampled": run("graph_sampled", graph=True, **sampled),
                 "prefill": prefill_only}
        for name, fn in forms.items():  # one warm pass: code objects, GEMM algorithms, the capture
            _clock_ms(fn)
            _log(f"B={B} warm {name} done")
        ms = {name: [] for name in forms}
        for _ in range(args.rounds):
            for name, fn in forms.items():
                ms[name].append(_clock_ms(fn))
        med = {name: _median(x) for name, x in ms.items()}
        rec = {"mode": "e2e", "model": f"SmolLM-1.7B geometry, {args.layers} layers", "B": B, "prompt": P,
               "new_tokens": N, "graph_captures": cache.graph_captures,
               "weights_floor_ms_per_step": round(floor_ms, 4), "prefill_ms": round(med["prefill"], 3)}
        for name in forms:
            if name == "prefill":
                continue
            rec[name + "_ms_rounds"] = [round(x, 1) for x in ms[name]]
            rec[name + "_ms_per_token"] = round(med[name] / N, 3)
            rec[name + "_step_over_floor"] = round((med[name] - med["prefill"]) / (N - 1) / floor_ms, 2)
        rec["graph_greedy_over_default"] = round(med["graph_greedy"] / med["default_greedy"], 3)
        rec["graph_sampled_over_default_top_k"] = round(med["graph_sampled"] / med["default_top_k"], 3)
        rec["greedy_tokens_equal_fraction_graph_vs_default"] = round(
            float((out["graph_greedy"] == out["default_greedy"]).float().mean()), 4)
        rec["graph_equals_fused_eager"] = bool(torch.equal(out["graph_greedy"], out["fused_eager_greedy"]) and
                                               torch.equal(out["graph_sampled"], out["fused_eager_sampled"]))
        _emit(args, rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["sampler", "e2e"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_bench.jsonl"),
                    help="append the JSON lines to this file")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("generate_bench: needs a HIP device (no measurement without one)")
    sampler(a) if a.mode == "sampler" else e2e(a)
