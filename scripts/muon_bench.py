"""picotron_amd.optim.Muon measurements on the bench model's decoder matrices (SmolLM-1.7B geometry, 15 layers;
bench.setup; muon_param_split picks the 7 matrices of each layer).

  kernels  the three HIP kernels of csrc/muon.hip (pico_muon_momentum 8 B per element, pico_muon_normalize 4,
           pico_muon_update 6) and pico_adamw_bf16 (14) on the same matrices, alternated in one process and timed by
           the library's per-launch events (pico_prof_*, all under PICO_K_ADAMW; the normalize call's small per-tensor
           finalize launch is not timed). One JSON line per kernel: avg_us, GB/s at its algorithmic bytes, its
           fraction of 8 TB/s and the ratio of its GB/s to pico_adamw_bf16's in the same run.
  step     Muon.step() and torch.optim.Muon.step() on clones of the same parameters and gradients, alternated for
           --rounds rounds; host clock around --steps steps ending in a synchronise, after warm-up. Reports ms per
           step for both, the Newton-Schulz GEMMs alone (the same clock around the GEMM calls of --steps steps), their
           share of the step, and the achieved FLOP/s from 2 * (2 m m n + m^3) * ns_steps per matrix, m = min(A, B),
           n = max(A, B).

Usage: python scripts/muon_bench.py kernels|step [--layers 15] [--iters 10] [--rounds 3] [--steps 3]
                                                 [--out profiles/muon_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES = {"muon_momentum": 8, "muon_normalize": 4, "muon_update": 6, "adamw_bf16": 14}


def _setup(layers):
    import torch.distributed as dist
    import bench
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.optim import muon_param_split
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29574")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    pgm.setup_process_group_manager(tp_size=1, cp_size=1, pp_size=1, dp_size=1)
    dev = torch.device("cuda", 0)
    _, model, _, _, _ = bench.setup(layers, 1, 1, dev, "pico", True)
    params, _ = muon_param_split(model)
    g = torch.Generator(device="cuda").manual_seed(0)
    for p in params:
        p.grad = (torch.randn(p.shape, device=dev, generator=g) * 1e-3).to(torch.bfloat16)
    torch.cuda.synchronize()
    _log(f"{len(params)} matrices, {sum(p.numel() for p in params)} parameters, gradients ready")
    return bench, dev, params


def _log(msg):
    print(f"[muon_bench] {msg}", file=sys.stderr, flush=True)


def _emit(args, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def kernels(args):
    from picotron_amd import _lib as L
    from picotron_amd.optim import AdamW, Muon
    bench, dev, params = _setup(args.layers)
    n = sum(p.numel() for p in params)
    muon = Muon(params, lr=0.02, adjust_lr_fn="match_rms_adamw")
    adamw = AdamW(params, lr=3e-4)
    for i in range(2):  # warm-up: tables, states, code objects
        muon.step()
        adamw.step()
        torch.cuda.synchronize()
        _log(f"warm-up {i}: Muon.step and AdamW.step done")
    lib, P = L.load(), L.ptr
    (ent,) = muon._tables.values()
    group = muon.param_groups[0]
    stream = L.stream_of(params[0])
    tab = (P(ent["tens"]), P(ent["sizes"]), P(ent["chunks"]), ent["n_chunks"])

    def momentum():
        L.check(lib.pico_muon_momentum(*tab, group["momentum"], 1, P(ent["partials"]), stream), "pico_muon_momentum")

    def normalize():
        L.check(lib.pico_muon_normalize(*tab, P(ent["chunk_start"]), len(params), P(ent["partials"]), group["eps"],
                                        P(ent["norms"]), stream), "pico_muon_normalize")

    def update():
        L.check(lib.pico_muon_update(tab[0], P(ent["out"]), *tab[1:], group["lr"], group["weight_decay"],
                                     P(ent["ratios"]), stream), "pico_muon_update")

    forms = {"muon_momentum": momentum, "muon_normalize": normalize, "muon_update": update, "adamw_bf16": adamw.step}
    us = {name: [] for name in forms}
    for _ in range(args.rounds):  # alternate, so a drifting clock shows up in every kernel alike
        for name, fn in forms.items():
            momentum()  # fresh u and partials in the work buffer (outside the timed window)
            L.prof_enable(L.K_ADAMW, 4 * args.iters)
            for _ in range(args.iters):
                fn()
            tot, cnt = L.prof_collect(L.K_ADAMW)
            L.load().pico_prof_enable(0, 0)
            assert cnt == args.iters, (name, cnt)
            us[name].append(1e3 * tot / cnt)
            _log(f"{name}: {us[name][-1]:.1f} us")
    med = {name: sorted(v)[len(v) // 2] for name, v in us.items()}
    gbs = {name: BYTES[name] * n / (med[name] * 1e-6) / 1e9 for name in forms}
    for name in forms:
        _emit(args, {"mode": "kernels", "kernel": name, "matrices": len(params), "params": n,
                     "bytes_per_param": BYTES[name], "avg_us_rounds": [round(u, 1) for u in us[name]],
                     "avg_us": round(med[name], 1), "GB_s": round(gbs[name], 1),
                     "frac_of_8TBs": round(gbs[name] / bench.HBM_PEAK_GBS, 4),
                     "bandwidth_over_adamw": round(gbs[name] / gbs["adamw_bf16"], 4)})


def step(args):
    from picotron_amd.optim import Muon, _newton_schulz
    bench, dev, params = _setup(args.layers)
    n = sum(p.numel() for p in params)
    ref_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for q, p in zip(ref_params, params):
        q.grad = p.grad.clone()
    kw = dict(lr=0.02, adjust_lr_fn="match_rms_adamw")
    ours, ref = Muon(params, **kw), torch.optim.Muon(ref_params, **kw)
    for i in range(2):
        ours.step()
        torch.cuda.synchronize()
        _log(f"warm-up {i}: Muon.step done")
        ref.step()
        torch.cuda.synchronize()
        _log(f"warm-up {i}: torch.optim.Muon.step done")
    (ent,) = ours._tables.values()
    group = ours.param_groups[0]
    ns_steps = group["ns_steps"]
    forms = {"pico": ours.step, "torch": ref.step,
             "pico_gemms": lambda: _newton_schulz(ent["ns_plan"], group["ns_coefficients"], ns_steps)}
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(args.rounds):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
    flop = sum(2 * (2 * min(p.shape) ** 2 * max(p.shape) + min(p.shape) ** 3) * ns_steps for p in params)
    work = sum(t.numel() * 2 for t in ent["work"].values())
    ns_ws = sum(t.numel() * 2 for t in ent["ns_flat"])
    _emit(args, {"mode": "step", "matrices": len(params), "params": n, "ns_steps": ns_steps,
                 "gemm_calls_per_step": 3 * ns_steps * len(ent["ns_plan"]),
                 "pico_ms_rounds": [round(x, 2) for x in ms["pico"]], "pico_ms_per_step": round(med["pico"], 2),
                 "torch_ms_rounds": [round(x, 2) for x in ms["torch"]], "torch_ms_per_step": round(med["torch"], 2),
                 "torch_over_pico": round(med["torch"] / med["pico"], 3),
                 "pico_gemms_ms_rounds": [round(x, 2) for x in ms["pico_gemms"]],
                 "pico_gemms_ms": round(med["pico_gemms"], 2),
                 "gemm_share": round(med["pico_gemms"] / med["pico"], 4), "ns_flop_per_step": flop,
                 "pico_step_TFLOPs": round(flop / (med["pico"] * 1e-3) / 1e12, 1),
                 "pico_gemms_TFLOPs": round(flop / (med["pico_gemms"] * 1e-3) / 1e12, 1),
                 "torch_step_TFLOPs": round(flop / (med["torch"] * 1e-3) / 1e12, 1),
                 "work_bytes": work, "ns_workspace_bytes": ns_ws,
                 "device_memory_allocated": torch.cuda.memory_allocated()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "step"])
    ap.add_argument("--layers", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    kernels(a) if a.mode == "kernels" else step(a)
