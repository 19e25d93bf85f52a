"""Kernel times of the vocab-parallel cross-entropy (pico_ce_vp_partial / _combine / _grad) beside the existing
full-vocabulary fused kernel (pico_cross_entropy_fwd_grad), one process, timed by the library's per-launch
events (pico_prof_*: the dispatch packet's timestamps).

Rows 4096 (SmolLM's micro-batch). The shard of one tp rank at vocab_local 24576 (tp 2) and 6144 (tp 8) of
V = 49152, in place as the fused LM head uses it; pico_cross_entropy_fwd_grad at V = 49152 in the same run.
The forms are alternated for --rounds rounds so that a drifting clock shows in all of them alike; every form
works on --bufs separate logits buffers in turn (default: enough to exceed the 256 MiB Infinity Cache between two
uses of a buffer, so the reads come from HBM as they do in a training step, where the GEMMs run in between;
--bufs 1 shows the cache-resident case of partial -> grad back to back).

Bytes (algorithmic): partial reads the shard once, grad reads and writes it once: 3 * rows * vocab_local * 2
for the three launches (combine moves 3 * tp + 2 floats per row, counted on its own line); the full-vocabulary
kernel reads and writes the logits once: 2 * rows * V * 2. Prints one JSON line per kernel and a summary line.

Usage: python scripts/ce_vp_kernels.py [--rows 4096] [--iters 20] [--rounds 3] [--bufs N]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
V = 49152


def main(args):
    from picotron_amd import _lib as L
    from picotron_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("ce_vp_kernels.py: no HIP device: kernel times are measured on the GPU only")
    dev = torch.device("cuda", 0)
    rows = args.rows
    g = torch.Generator(device="cuda").manual_seed(0)
    tgt = torch.randint(0, V, (rows,), device=dev, generator=g)
    tgt[::7] = -100
    stats = ops.ce_count(tgt)
    gscale = stats[1:]
    res = {}

    def buffers(cols):
        n = args.bufs or max(2, -(-(320 << 20) // (rows * cols * 2)))
        return [(torch.randn(rows, cols, device=dev, generator=g) * 3).to(torch.bfloat16) for _ in range(n)]

    def timed(name, kid, fns, nbytes):
        for fn in fns:  # warm-up on every buffer
            fn()
        L.prof_enable(kid, 4 * args.iters * len(fns))
        for _ in range(args.iters):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        tot, cnt = L.prof_collect(kid)
        L.load().pico_prof_enable(0, 0)
        assert cnt == args.iters * len(fns), (name, cnt)
        res.setdefault(name, {"bytes": nbytes, "us": []})["us"].append(1e3 * tot / cnt)

    lse = torch.empty(rows, dtype=torch.float32, device=dev)
    loss = torch.empty(rows, dtype=torch.float32, device=dev)

    def full_fwd_grad(b):
        # the gradient overwrites the logits: later iterations time the same sweep on other values
        L.check(L.load().pico_cross_entropy_fwd_grad(L.ptr(b), b.stride(0), L.ptr(tgt), L.ptr(lse), L.ptr(loss),
                                                     L.ptr(gscale), rows, V, -100, L.stream_of(b)), "fwd_grad")

    full = buffers(V)
    shards = {tp: buffers(V // tp) for tp in (2, 8)}
    parts = {tp: torch.stack([ops.ce_vp_partial(shards[tp][0], tgt, r * (V // tp), V) for r in range(tp)])
             for tp in (2, 8)}
    lses = {tp: ops.ce_vp_combine(parts[tp], tgt, V)[0] for tp in (2, 8)}
    for _ in range(args.rounds):
        timed("cross_entropy_fwd_grad V=49152", L.K_CE_FWD, [lambda b=b: full_fwd_grad(b) for b in full],
              2 * rows * V * 2)
        for tp in (2, 8):
            vl = V // tp
            tag = f"tp={tp} vocab_local={vl}"
            timed(f"ce_vp_partial {tag}", L.K_CE_FWD,
                  [lambda b=b: ops.ce_vp_partial(b, tgt, 0, V) for b in shards[tp]], rows * vl * 2)
            timed(f"ce_vp_combine {tag}", L.K_CE_FWD, [lambda: ops.ce_vp_combine(parts[tp], tgt, V)],
                  rows * (3 * tp + 2) * 4)
            timed(f"ce_vp_grad {tag}", L.K_CE_BWD,
                  [lambda b=b: ops.ce_vp_grad(b, tgt, lses[tp], gscale, 0, V, out=b) for b in shards[tp]],
                  2 * rows * vl * 2)
    med = {}
    for name, r in res.items():
        us = med[name] = sorted(r["us"])[len(r["us"]) // 2]
        gbs = r["bytes"] / (us * 1e-6) / 1e9
        print(json.dumps({"kernel": name, "rows": rows, "bytes": r["bytes"],
                          "avg_us_rounds": [round(u, 1) for u in r["us"]], "avg_us": round(us, 1),
                          "GB_s": round(gbs, 1), "frac_of_8TBs": round(gbs / HBM_PEAK_GBS, 4)}), flush=True)
    out = {"full_us": round(med["cross_entropy_fwd_grad V=49152"], 1), "bufs_full": len(full)}
    for tp in (2, 8):
        tag = f"tp={tp} vocab_local={V // tp}"
        out[f"vp_sum_us tp={tp}"] = round(sum(med[f"{k} {tag}"]
                                              for k in ("ce_vp_partial", "ce_vp_combine", "ce_vp_grad")), 1)
        out[f"bufs tp={tp}"] = len(shards[tp])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bufs", type=int, default=0,
                    help="logits buffers each form cycles through (0: past the Infinity Cache)")
    main(ap.parse_args())
