"""Per-projection time of ops.decode_linear against torch.nn.functional.linear (hipBLASLt, plus the row-wise kernels
the fused forms replace) at the five decode projections of the SmolLM-1.7B geometry, M = 1 and 8. Needs a HIP device.

Every call reads another copy of the weight, out of a ring of copies larger than the 256 MB last-level cache, so
that the weight comes from HBM as it does in a decode step. `calls`: device events around --iters eager calls,
medians of --rounds alternated rounds.

The figures of that mode are call times (an eager call cannot be issued faster than the host allows), never shares
of a peak. Kernel times come from a kernel trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/decode_linear_bench.py trace
  python scripts/decode_linear_bench.py table --trace DIR/.../*_kernel_trace.csv [--out profiles/...jsonl]

`trace` quantises every weight of the ring once (ops.quantize_weight_fp8, ops.quantize_weight_mxfp4), warms every
form up, then runs, per shape and M, a marker launch (pico_scale_f32), --iters decode_linear calls, a marker, --iters
F.linear calls (the GEMM alone: what hipBLASLt launches for the shape), a marker, --iters decode_linear calls on the
Fp8Weights, a marker, --iters decode_linear calls on the Mxfp4Weights (their ring filled up with clones to the bf16
ring's bytes, so that it does not fit the last-level cache either); nothing else runs on the device in between. `table` cuts the trace at the markers and reports, per shape and M, the median kernel
time per call of the stream kernel, of the finishing launch and of hipBLASLt's kernels, with the weight's bytes over
the stream + finish time as a share of the HBM peak; the same for the FP8 kernels (share on the FP8 bytes, N K) and the
MXFP4 kernels (share on N K / 2 + N K / 32 bytes, and their time over the FP8 kernels'), and the quantisers' time per
matrix.

Usage: python scripts/decode_linear_bench.py [calls|trace|table] [--out FILE] [--iters 40] [--rounds 3] [--trace CSV]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
RING_BYTES = 640 << 20
# name, N, K, norm prologue, swiglu, fp32 output
SHAPES = [("qkv", 6144, 2048, True, False, False), ("out", 2048, 2048, False, False, False),
          ("gate_up", 16384, 2048, True, True, False), ("down", 2048, 8192, False, False, False),
          ("lm_head", 49152, 2048, True, False, True)]


def _events_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def main(args):
    from picotron_amd import ops
    dev = torch.device("cuda", 0)
    F = torch.nn.functional
    for name, N, K, norm, swiglu, f32 in SHAPES:
        copies = max(2, RING_BYTES // (N * K * 2) + 1)
        ws = [torch.randn(N, K, device=dev).mul_(K ** -0.5).bfloat16() for _ in range(copies)]
        gamma = torch.ones(K, dtype=torch.bfloat16, device=dev)
        for M in (1, 8):
            x = torch.randn(M, K, device=dev).bfloat16()
            res = torch.randn(M, K, device=dev).bfloat16()

            def skinny(i):
                kw = dict(norm_weight=gamma, eps=1e-5, residual=res) if norm else {}
                ops.decode_linear(x, ws[i % copies], swiglu=swiglu, out_dtype=torch.float32 if f32 else None, **kw)

            def baseline(i):  # what decode_step runs today for the same work
                h = ops.rms_norm(x, gamma, 1e-5, residual=res, prenorm=True)[0] if norm else x
                y = F.linear(h, ws[i % copies])
                if swiglu:
                    act = torch.empty((M, N // 2), dtype=y.dtype, device=dev)
                    ops._swiglu_fwd(y, y[:, N // 2:], act, M, N // 2, N, N // 2)
                elif f32:
                    y.float()

            def gemm_only(i):
                F.linear(x, ws[i % copies])

            fns = {"decode_linear": skinny, "baseline": baseline, "linear_only": gemm_only}
            with torch.no_grad():
                for fn in fns.values():
                    _events_us(fn, 5)
                us = {k: [] for k in fns}
                for _ in range(args.rounds):
                    for k, fn in fns.items():
                        us[k].append(_events_us(fn, args.iters))
            rec = {"shape": name, "N": N, "K": K, "M": M, "weight_MB": round(N * K * 2 / 1e6, 1)}
            for k in fns:
                med = sorted(us[k])[len(us[k]) // 2]
                rec[k + "_us"] = round(med, 2)
                rec[k + "_us_rounds"] = [round(v, 2) for v in us[k]]
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        del ws


def _cases(dev):
    for name, N, K, norm, swiglu, f32 in SHAPES:
        copies = max(2, RING_BYTES // (N * K * 2) + 1)
        ws = [torch.randn(N, K, device=dev).mul_(K ** -0.5).bfloat16() for _ in range(copies)]
        for M in (1, 8):
            yield name, N, K, norm, swiglu, f32, M, ws


def trace(args):
    from picotron_amd import _lib, ops
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    mark = torch.zeros(256, dtype=torch.float32, device=dev)
    gamma = {K: torch.ones(K, dtype=torch.bfloat16, device=dev) for K in (2048, 8192)}
    cases = list(_cases(dev))
    xs = {(c[0], c[6]): (torch.randn(c[6], c[2], device=dev).bfloat16(), torch.randn(c[6], c[2], device=dev).bfloat16())
          for c in cases}

    def skinny(c, i):
        name, N, K, norm, swiglu, f32, M, ws = c
        x, res = xs[(name, M)]
        kw = dict(norm_weight=gamma[K], eps=1e-5, residual=res) if norm else {}
        ops.decode_linear(x, ws[i % len(ws)], swiglu=swiglu, out_dtype=torch.float32 if f32 else None, **kw)

    def gemm(c, i):
        torch.nn.functional.linear(xs[(c[0], c[6])][0], c[7][i % len(c[7])])

    # every copy of the ring quantised once (pico_quantize_rows_fp8: the trace holds one launch per matrix)
    q8 = {}
    for c in cases:
        if c[0] not in q8:
            q8[c[0]] = [ops.quantize_weight_fp8(w) for w in c[7]]

    def fp8(c, i):
        name, N, K, norm, swiglu, f32, M, ws = c
        x, res = xs[(name, M)]
        kw = dict(norm_weight=gamma[K], eps=1e-5, residual=res) if norm else {}
        ops.decode_linear(x, q8[name][i % len(ws)], swiglu=swiglu, out_dtype=torch.float32 if f32 else None, **kw)

    # ... and as MXFP4; that ring is filled up with clones until it, too, is RING_BYTES of codes and scales: the
    # quantised copies alone (17 / 64 of the bf16 bytes) would fit the last-level cache
    q4 = {}
    for c in cases:
        if c[0] not in q4:
            q4[c[0]] = ring = [ops.quantize_weight_mxfp4(w) for w in c[7]]
            each = ring[0].codes.numel() + ring[0].scales.numel()
            for j in range(RING_BYTES // each + 1 - len(ring)):
                ring.append(ops.Mxfp4Weight(ring[j % len(c[7])].codes.clone(), ring[j % len(c[7])].scales.clone()))

    def mx4(c, i):
        name, N, K, norm, swiglu, f32, M, ws = c
        x, res = xs[(name, M)]
        kw = dict(norm_weight=gamma[K], eps=1e-5, residual=res) if norm else {}
        ops.decode_linear(x, q4[name][i % len(q4[name])], swiglu=swiglu, out_dtype=torch.float32 if f32 else None, **kw)

    def marker():
        _lib.check(lib.pico_scale_f32(_lib.ptr(mark), mark.numel(), 2.0, _lib.stream_of(mark)), "pico_scale_f32")

    with torch.no_grad():
        for c in cases:
            for i in range(3):
                skinny(c, i)
                gemm(c, i)
                fp8(c, i)
                mx4(c, i)
        torch.cuda.synchronize()
        for c in cases:
            for fn in (skinny, gemm, fp8, mx4):
                marker()
                for i in range(args.iters):
                    fn(c, i)
        marker()
        torch.cuda.synchronize()


def table(args):
    import csv
    with open(args.trace) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    segs, cur = [], None
    for r in rows:
        if "scale_kernel" in r["Kernel_Name"]:
            cur = []
            segs.append(cur)
        elif cur is not None:
            cur.append((r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    segs = segs[:-1]  # the closing marker opens nothing
    combos = [(s[0], s[1], s[2], M) for s in SHAPES for M in (1, 8)]
    assert len(segs) == 4 * len(combos), (len(segs), len(combos))
    med = lambda v: sorted(v)[len(v) // 2] if v else 0.0
    quant = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows
             if "quantize_rows_fp8" in r["Kernel_Name"]]
    quant4 = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows
              if "quantize_rows_mxfp4" in r["Kernel_Name"]]
    quant_us, quant4_us = {}, {}
    for name, N, K, *_ in SHAPES:  # one launch per matrix of the ring, shape after shape
        copies = max(2, RING_BYTES // (N * K * 2) + 1)
        quant_us[name], quant = round(med(quant[:copies]), 2), quant[copies:]
        quant4_us[name], quant4 = round(med(quant4[:copies]), 2), quant4[copies:]
    for i, (name, N, K, M) in enumerate(combos):
        ours, theirs, eight, four = segs[4 * i:4 * i + 4]
        stream4 = [t for n, t in four if "decode_linear_mxfp4_kernel" in n]
        finish4 = [t for n, t in four if "decode_linear_mxfp4_finish" in n]
        assert len(stream4) + len(finish4) == len(four) and len(stream4) == args.iters, (name, M, len(four))
        total4 = med(stream4) + med(finish4)
        stream8 = [t for n, t in eight if "decode_linear_fp8_kernel" in n]
        finish8 = [t for n, t in eight if "decode_linear_fp8_finish" in n]
        assert len(stream8) + len(finish8) == len(eight) and len(stream8) == args.iters, (name, M, len(eight))
        total8 = med(stream8) + med(finish8)
        stream = [t for n, t in ours if "decode_linear_kernel" in n]
        finish = [t for n, t in ours if "decode_linear_finish" in n]
        assert len(stream) + len(finish) == len(ours) and len(stream) == args.iters, (name, M, len(ours))
        per_call = len(theirs) // args.iters
        assert per_call * args.iters == len(theirs), (name, M, len(theirs))
        gemm_us = med([sum(t for _, t in theirs[j * per_call:(j + 1) * per_call]) for j in range(args.iters)])
        total = med(stream) + med(finish)
        share = lambda us: round(N * K * 2 / (us * 1e-6) / (HBM_PEAK_GBS * 1e9), 3)
        rec = {"shape": name, "N": N, "K": K, "M": M, "weight_MB": round(N * K * 2 / 1e6, 1),
               "stream_us": round(med(stream), 2), "finish_us": round(med(finish), 2), "decode_linear_us": round(total, 2),
               "decode_linear_hbm_share": share(total), "hipblaslt_us": round(gemm_us, 2),
               "hipblaslt_kernels_per_call": per_call, "hipblaslt_hbm_share": share(gemm_us),
               "hipblaslt_kernel": theirs[0][0][:80],
               "fp8_stream_us": round(med(stream8), 2), "fp8_finish_us": round(med(finish8), 2),
               "fp8_us": round(total8, 2), "fp8_hbm_share": round(share(total8) / 2, 3),  # on the FP8 bytes: N K
               "fp8_over_bf16": round(total8 / total, 3), "quantize_us": quant_us[name],
               "mxfp4_stream_us": round(med(stream4), 2), "mxfp4_finish_us": round(med(finish4), 2),
               "mxfp4_us": round(total4, 2),  # the share on the MXFP4 bytes: N K / 2 + N K / 32
               "mxfp4_hbm_share": round(share(total4) * (0.5 + 1 / 32) / 2, 3),
               "mxfp4_over_fp8": round(total4 / total8, 3), "quantize_mxfp4_us": quant4_us[name]}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="calls", choices=["calls", "trace", "table"])
    ap.add_argument("--trace", help="table: the kernel trace CSV of a trace run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_linear_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.mode == "table":
        table(a)
    elif not torch.cuda.is_available():
        sys.exit("decode_linear_bench: needs a HIP device (no measurement without one)")
    else:
        trace(a) if a.mode == "trace" else main(a)
