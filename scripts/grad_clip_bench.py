"""Gradient-norm / clip measurements on the bench model (SmolLM-1.7B geometry, 15 layers; bench.setup).

  kernels  the isolated kernels on the model's parameter list, timed by the library's per-launch events
           (pico_prof_*): grad_sqnorm, grad_scale, and adamw plain vs adamw with the clip folded in, alternated in
           one process. Prints one JSON line per kernel: avg_us, algorithmic GB/s and its fraction of 8 TB/s
           (bench.py's kernels-table convention: every input read once + every output written once).
  e2e      TrainingStep at the bench configuration (grad_acc 32, graphs), three optimizer forms alternated A/B/C
           for --rounds rounds: the plain step, AdamW(max_grad_norm=1.0), and torch.nn.utils.clip_grad_norm_ +
           the plain step (what users had before). Host clock around --steps steps ending in a synchronise.

Usage: python scripts/grad_clip_bench.py kernels|e2e [--layers 15] [--iters 10] [--rounds 3] [--steps 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _setup(layers, grad_acc):
    import torch.distributed as dist
    import bench
    from picotron_amd import process_group_manager as pgm
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29571")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    pgm.setup_process_group_manager(tp_size=1, cp_size=1, pp_size=1, dp_size=1)
    dev = torch.device("cuda", 0)
    return bench, dev, bench.setup(layers, grad_acc, 1, dev, "pico", True)


def kernels(args):
    from picotron_amd import _lib as L
    from picotron_amd.optim import AdamW, clip_grad_norm_, get_grad_norm
    bench, dev, (cfg, model, _, _, n) = _setup(args.layers, 1)
    params = list(model.parameters())
    g = torch.Generator(device="cuda").manual_seed(0)
    for p in params:
        p.grad = (torch.randn(p.shape, device=dev, generator=g) * 1e-3).to(torch.bfloat16)
    plain, clip = AdamW(params, lr=3e-4), AdamW(params, lr=3e-4, max_grad_norm=1.0)
    for _ in range(2):  # warm-up: tables, states, code objects
        plain.step()
        clip.step()
        get_grad_norm(params, groups=())
    res = {}

    def timed(name, kid, fn, bytes_per_param):
        L.prof_enable(kid, 4 * args.iters)
        for _ in range(args.iters):
            fn()
        tot, cnt = L.prof_collect(kid)
        L.load().pico_prof_enable(0, 0)
        res.setdefault(name, {"bytes": bytes_per_param * n, "us": []})["us"].append(1e3 * tot / cnt)

    scale_norm = [float(get_grad_norm(params, groups=()))]

    def scale():  # every call clips to half the current norm, so the kernel always rewrites the gradients
        scale_norm[0] *= 0.5
        clip_grad_norm_(params, scale_norm[0], groups=())

    for _ in range(args.rounds):  # alternate, so a drifting clock shows up in every kernel alike
        timed("adamw", L.K_ADAMW, plain.step, 14)
        timed("adamw_clip", L.K_ADAMW, lambda: clip.step(), 14)
        timed("grad_sqnorm", L.K_GRAD_SQNORM, lambda: get_grad_norm(params, groups=()), 2)
        timed("grad_scale", L.K_GRAD_SCALE, scale, 4)
    for name, r in res.items():
        us = sorted(r["us"])[len(r["us"]) // 2]
        gbs = r["bytes"] / (us * 1e-6) / 1e9
        print(json.dumps({"kernel": name, "params": n, "bytes": r["bytes"], "avg_us_rounds": [round(u, 1) for u in r["us"]],
                          "avg_us": round(us, 1), "GB_s": round(gbs, 1),
                          "frac_of_8TBs": round(gbs / bench.HBM_PEAK_GBS, 4)}), flush=True)


class TorchClipThenStep:
    """torch.nn.utils.clip_grad_norm_ followed by the plain step: the optimizer interface TrainingStep uses."""

    def __init__(self, opt, params, max_norm):
        self.opt, self.params, self.max_norm = opt, params, max_norm

    def zero_grad(self, set_to_none=True):
        self.opt.zero_grad(set_to_none=set_to_none)

    def step(self):
        torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
        self.opt.step()


def e2e(args):
    from picotron_amd.optim import AdamW
    from picotron_amd.train import TrainingStep
    bench, dev, (cfg, model, opt, loader, n) = _setup(args.layers, args.grad_acc)
    params = list(model.parameters())
    forms = {"plain": opt, "fused_clip": AdamW(params, lr=3e-4, max_grad_norm=1.0),
             "torch_clip": TorchClipThenStep(opt, params, 1.0)}
    step = TrainingStep(model, opt, loader, dev, graphs=True)
    for name, o in forms.items():  # warm-up every form
        step.optimizer = o
        for _ in range(2):
            step(sync_loss=False)
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(args.rounds):
        for name, o in forms.items():
            step.optimizer = o
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(sync_loss=False)
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    grad_bytes = 2 * n
    for name, v in ms.items():
        med = sorted(v)[len(v) // 2]
        print(json.dumps({"form": name, "ms_per_step_rounds": [round(x, 2) for x in v], "ms_per_step": round(med, 2),
                          "over_plain_ms": round(med - sorted(ms["plain"])[len(v) // 2], 2), "params": n,
                          "grad_bytes": grad_bytes, "grad_norm": (float(forms[name].grad_norm)
                                                                  if name == "fused_clip" else None)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "e2e"])
    ap.add_argument("--layers", type=int, default=15)
    ap.add_argument("--grad-acc", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    kernels(a) if a.mode == "kernels" else e2e(a)
