"""The per-tile attention check (tests/attn_ref.py) proves itself on the CPU: honest implementations pass it on every
input set, mutants that today's whole-tensor rel_l2 tolerances accept fail it, and the GPU file's case table reaches
every kernel path of the backward plan at 256 CUs (the plan printed by tests/attn_bwd_plan_check.cpp). CPU only."""
import functools
import math
import os
import subprocess

import pytest
import torch

import attn_ref as R

# B, Sq, Sk, Hq, Hkv, D, causal: D 64 and 128, causal and not, ragged 257, GQA 4
HONEST = [
    (2, 257, 257, 4, 1, 64, True),
    (1, 200, 200, 2, 2, 128, True),
    (2, 96, 200, 4, 4, 64, False),
    (1, 300, 77, 4, 1, 128, False),
    (1, 257, 257, 2, 2, 64, False),
]


@pytest.mark.parametrize("kind", ["randn", "diag", "bait"])
@pytest.mark.parametrize("B,Sq,Sk,Hq,Hkv,D,causal", HONEST)
def test_honest_implementations_pass(B, Sq, Sk, Hq, Hkv, D, causal, kind):
    """The blockwise emulation (64-key tiles, online softmax) against the dense one's bound: no honest implementation
    may be flagged, on any input set. Both also meet the suite's whole-tensor tolerances."""
    q, k, v, do = R.make_inputs(kind, B, Sq, Sk, Hq, Hkv, D, causal)
    sc = 1.0 / math.sqrt(D)
    O, L = R.reference_fwd(q, k, v, sc, causal)
    od, ld = R.emulate_fwd(q, k, v, sc, causal)
    ob, lb = R.emulate_fwd(q, k, v, sc, causal, block=64)
    res = [R.tile_check("O", ob, od, O)]
    assert R.lse_check(ld, L)["ok"] and R.lse_check(lb, L)["ok"]
    assert R.rel_l2(od, O) < R.FWD_TOL and R.rel_l2(ob, O) < R.FWD_TOL
    rope = R.rope_tables(max(Sq, Sk), D) if causal else None
    ref = R.reference_bwd(do, q, k, v, od, ld, sc, causal, rope=rope)
    ed = R.emulate_bwd(do, q, k, v, od, ld, sc, causal, rope=rope)
    eb = R.emulate_bwd(do, q, k, v, od, ld, sc, causal, rope=rope, block=64)
    for n, b_, d_, r_ in zip(("dQ", "dK", "dV"), eb, ed, ref):
        res.append(R.tile_check(n, b_, d_, r_))
        assert R.rel_l2(d_, r_) < R.BWD_TOL and R.rel_l2(b_, r_) < R.BWD_TOL
    # the fp32-accumulate dQ: no bf16 term
    e32 = R.emulate_bwd(do, q, k, v, od, ld, sc, causal, dq_f32=True)[0]
    b32 = R.emulate_bwd(do, q, k, v, od, ld, sc, causal, dq_f32=True, block=64)[0]
    r32 = R.reference_bwd(do, q, k, v, od, ld, sc, causal)[0]
    res.append(R.tile_check("dQ fp32", b32, e32, r32, bf16_term=False))
    worst = R.worst_of(res)
    print("worst tile:", worst)
    assert all(r_["ok"] for r_ in res), worst


def test_planted_keys_lead_their_rows():
    """diag: the planted diagonal key leads every other visible score of its row by at least 8 nats (first query
    head of the group); bait: the planted key above the diagonal would lead row r by as much if it were visible."""
    for D in (64, 128):
        B, S, Hq, Hkv = 2, 1024, 4, 2
        sc = 1.0 / math.sqrt(D)
        for kind, off in (("diag", 0), ("bait", 1)):
            q, k, _, _ = R.make_inputs(kind, B, S, S, Hq, Hkv, D, True)
            s = torch.einsum("bqhd,bkhd->bhqk", q[:, :, ::Hq // Hkv].double(), k.double()) * sc
            vis = torch.tril(torch.ones(S, S, dtype=torch.bool))
            rows = [r_ for r_ in R.edge_rows(S) if r_ + off < S]
            for r_ in rows:
                planted = s[:, :, r_, r_ + off]
                others = s[:, :, r_].masked_fill(~vis[r_], -math.inf)
                others[:, :, r_ + off] = -math.inf
                assert float((planted - others.amax(-1)).min()) >= 8.0, (D, kind, r_)


def _dq_two_half_sums(do, q, k, v, o, lse, sc, causal):
    """A third honest fp32-accumulate dQ: the dense emulation's arithmetic with every fp32 dot product over D summed
    in two halves (another accumulation order, nothing else)."""
    Q, K, V, DO, O = [t.float().permute(0, 2, 1, 3) for t in (q, k, v, do, o)]
    G, h = Q.shape[1] // K.shape[1], Q.shape[-1] // 2
    K, V = K.repeat_interleave(G, 1), V.repeat_interleave(G, 1)
    s = (Q[..., :h] @ K[..., :h].transpose(-1, -2) + Q[..., h:] @ K[..., h:].transpose(-1, -2)) * sc
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(s.shape[-2:], dtype=torch.bool)), -math.inf)
    p = torch.exp(s - lse.float()[..., None])
    dp = DO[..., h:] @ V[..., h:].transpose(-1, -2) + DO[..., :h] @ V[..., :h].transpose(-1, -2)
    delta = (DO[..., h:] * O[..., h:]).sum(-1, keepdim=True) + (DO[..., :h] * O[..., :h]).sum(-1, keepdim=True)
    ds = (p * (dp - delta)).to(R.BF).float()
    return (ds @ K * sc).permute(0, 2, 1, 3)


@pytest.mark.parametrize("B,S,Hq,Hkv,D", [(2, 257, 4, 2, 128), (2, 129, 2, 2, 64), (2, 65, 2, 2, 128)])
def test_tail_tile_is_32_consecutive_rows(B, S, Hq, Hkv, D):
    """Why a ragged tail's tile is the last 32 rows (attn_ref.tile_rows) and not the one-row stub: on `diag` inputs
    the stub is one planted, saturated row whose dQ is what is left after P (dO V^T - delta) cancels, and an honest
    implementation that only sums its fp32 dot products in another order misses the bound on that stub (measured
    here: 10.1x at S 257, D 128; 1.15x at S 129, D 64; 1.34x at S 65, D 128 -- printed, not asserted: it is
    summation noise) while every tile of 32 consecutive rows sits at 0.50 of it."""
    q, k, v, do = R.make_inputs("diag", B, S, S, Hq, Hkv, D, True)
    sc = 1.0 / math.sqrt(D)
    o, lse = R.emulate_fwd(q, k, v, sc, True)
    ref = R.reference_bwd(do, q, k, v, o, lse, sc, True)[0]
    emu = R.emulate_bwd(do, q, k, v, o, lse, sc, True, dq_f32=True)[0]
    alt = _dq_two_half_sums(do, q, k, v, o, lse, sc, True)
    n = S % R.TILE
    err = (alt.double() - ref)[:, S - n:].pow(2).sum((1, 3)).sqrt()
    bound = R.M_TILE * (emu.double() - ref)[:, S - n:].pow(2).sum((1, 3)).sqrt()
    print(f"one-row stub of S {S}, D {D}: worst err / bound {float((err / bound).max()):.2f}")
    res = R.tile_check("dQ fp32", alt, emu, ref, bf16_term=False)
    assert res["ok"], res


# ------------------------------------------------------------------------------------------ mutants
FWD_C = (2, 1024, 1024, 4, 4, 64, True)    # the issue's own shape: B 2, S 1024, H 4, D 64, causal
FWD_N = (2, 993, 993, 8, 8, 64, False)     # ragged tail, non-causal
BWD_C = (2, 1024, 1024, 32, 4, 64, True)   # GQA 8
BWD_G = (4, 1024, 1024, 128, 16, 64, True)  # GQA 8, enlarged until one O(1)-wrong query tile hides in the whole tensor


@functools.lru_cache(maxsize=None)
def _fwd_base(shape):
    B, Sq, Sk, Hq, Hkv, D, causal = shape
    q, k, v, do = R.make_inputs("randn", B, Sq, Sk, Hq, Hkv, D, causal)
    sc = 1.0 / math.sqrt(D)
    O, _ = R.reference_fwd(q, k, v, sc, causal)
    od, ld = R.emulate_fwd(q, k, v, sc, causal)
    ob, _ = R.emulate_fwd(q, k, v, sc, causal, block=64)
    return {"q": q, "k": k, "v": v, "do": do, "sc": sc, "ref": O, "dense": od, "lse": ld, "block": ob}


@functools.lru_cache(maxsize=None)
def _bwd_base(shape):
    B, Sq, Sk, Hq, Hkv, D, causal = shape
    if shape == BWD_G:  # the large shape: dense emulation only (it stands in for the kernel too)
        q, k, v, do = R.make_inputs("randn", B, Sq, Sk, Hq, Hkv, D, causal)
        f = {"q": q, "k": k, "v": v, "do": do, "sc": 1.0 / math.sqrt(D)}
        f["dense"], f["lse"] = R.emulate_fwd(q, k, v, f["sc"], causal)
    else:
        f = dict(_fwd_base(shape))
    args = (f["do"], f["q"], f["k"], f["v"], f["dense"], f["lse"], f["sc"], causal)
    f["bref"] = R.reference_bwd(*args)
    f["bdense"] = R.emulate_bwd(*args)
    f["bblock"] = R.emulate_bwd(*args, block=64) if shape != BWD_G else f["bdense"]
    return f


def _fwd_mutant(shape, b, h, allow, extra_key=False):
    """The blockwise emulation's O with the mask of (b, h) replaced by `allow` (MHA shapes); extra_key: a key Sk (the
    clamp duplicate of key Sk - 1) exists, visible only where allow says."""
    f = _fwd_base(shape)
    q, k, v = [f[n][b:b + 1, :, h:h + 1] for n in ("q", "k", "v")]
    if extra_key:
        k, v = torch.cat((k, k[:, -1:]), 1), torch.cat((v, v[:, -1:]), 1)
    o, _ = R.emulate_fwd(q, k, v, f["sc"], False, block=64, allow={(0, 0): allow})
    out = f["block"].clone()
    out[b, :, h] = o[0, :, 0]
    return out


def _gap(name, mutant, dense, ref, tol, tile=None):
    """A mutant must pass today's whole-tensor tolerance and fail the per-tile check (at `tile`, if given)."""
    whole = R.rel_l2(mutant, ref)
    res = R.tile_check(name, mutant, dense, ref)
    print(f"{name}: whole-tensor rel_l2 {whole:.2e} (tolerance {tol:g}), worst tile ratio {res['ratio']:.2f} at "
          f"(batch {res['batch']}, head {res['head']}, row block {res['row_block']})")
    assert whole < tol, f"{name}: the whole-tensor tolerance already sees this mutant ({whole:.2e}); enlarge the shape"
    assert not res["ok"], f"{name}: the per-tile check missed the mutant (ratio {res['ratio']:.2f})"
    if tile is not None:
        assert (res["batch"], res["head"], res["row_block"]) == tile, res
    return whole, res["ratio"]


def test_honest_blockwise_passes_at_the_mutant_shapes():
    for shape in (FWD_C, FWD_N):
        f = _fwd_base(shape)
        assert R.tile_check("O", f["block"], f["dense"], f["ref"])["ok"]
    f = _bwd_base(BWD_C)
    for n, b_, d_, r_ in zip(("dQ", "dK", "dV"), f["bblock"], f["bdense"], f["bref"]):
        assert R.tile_check(n, b_, d_, r_)["ok"]


def test_mutant_key_above_diagonal_visible():
    """Key i + 1 visible to the 32 rows of one tile."""
    S = FWD_C[1]
    allow = torch.tril(torch.ones(S, S, dtype=torch.bool))
    for r_ in range(512, 544):
        allow[r_, r_ + 1] = True
    f = _fwd_base(FWD_C)
    _gap("O", _fwd_mutant(FWD_C, 1, 2, allow), f["dense"], f["ref"], R.FWD_TOL, tile=(1, 2, 16))


def test_mutant_diagonal_key_dropped():
    """The diagonal key dropped for the last 32 rows of one head."""
    S = FWD_C[1]
    allow = torch.tril(torch.ones(S, S, dtype=torch.bool))
    for r_ in range(S - 32, S):
        allow[r_, r_] = False
    f = _fwd_base(FWD_C)
    _gap("O", _fwd_mutant(FWD_C, 0, 3, allow), f["dense"], f["ref"], R.FWD_TOL, tile=(0, 3, S // 32 - 1))


def test_mutant_ragged_tail_key_dropped():
    """Key Sk - 1 of a ragged tail dropped for one tile."""
    S = FWD_N[1]
    allow = torch.ones(S, S, dtype=torch.bool)
    allow[64:96, S - 1] = False
    f = _fwd_base(FWD_N)
    _gap("O", _fwd_mutant(FWD_N, 1, 0, allow), f["dense"], f["ref"], R.FWD_TOL, tile=(1, 0, 2))


def test_mutant_key_past_the_end_added():
    """Key Sk (a clamp duplicate of key Sk - 1: what a clamped load returns) added for one tile."""
    S = FWD_N[1]
    allow = torch.ones(S, S + 1, dtype=torch.bool)
    allow[:, S] = False
    allow[S - 32:S, S] = True
    f = _fwd_base(FWD_N)
    _gap("O", _fwd_mutant(FWD_N, 0, 1, allow, extra_key=True), f["dense"], f["ref"], R.FWD_TOL,
         tile=(0, 1, len(R.tile_rows(S)) - 1))


def _bwd_mutant(b, shape=BWD_C, **mut):
    """dK, dV of the blockwise emulation with batch b recomputed under a mutation (drop=... or swapped inputs)."""
    f = _bwd_base(shape)
    t = {n: mut.pop(n, f[n])[b:b + 1] for n in ("do", "q", "k", "v", "dense", "lse")}
    _, dk, dv = R.emulate_bwd(t["do"], t["q"], t["k"], t["v"], t["dense"], t["lse"], f["sc"], True, block=64, **mut)
    out = [f["bblock"][1].clone(), f["bblock"][2].clone()]
    out[0][b], out[1][b] = dk[0], dv[0]
    return out


def _bwd_gap(mutant, shape=BWD_C):
    f = _bwd_base(shape)
    for i, n in ((1, "dK"), (2, "dV")):
        _gap(n, mutant[i - 1], f["bdense"][i], f["bref"][i], R.BWD_TOL)


def test_mutant_gqa_neighbouring_kv_head():
    """One query head of a GQA group reading the neighbouring kv head for one 32-row query tile: seen from the
    key-major dK / dV kernels, that tile of query head hq lands in the neighbouring group's key blocks and the
    neighbour's tile lands here (the tile's q, dO, O and LSE rows swapped between hq and hq + group size)."""
    f = _bwd_base(BWD_G)
    S, G = BWD_G[1], BWD_G[3] // BWD_G[4]
    hq, rows = 5, slice(S - 64, S - 32)
    swapped = {}
    for n in ("do", "q", "dense"):
        x = f[n].clone()
        x[1, rows, hq], x[1, rows, hq + G] = f[n][1, rows, hq + G], f[n][1, rows, hq]
        swapped[n] = x
    lse = f["lse"].clone()
    lse[1, hq, rows], lse[1, hq + G, rows] = f["lse"][1, hq + G, rows], f["lse"][1, hq, rows]
    _bwd_gap(_bwd_mutant(1, BWD_G, lse=lse, **swapped), BWD_G)


def test_mutant_query_tile_missing_from_a_key_block():
    """One 32-row query tile missing from one 128-key block's dK / dV."""
    S = BWD_C[1]
    drop = torch.zeros(S, S, dtype=torch.bool)
    drop[S - 32:S, S - 128:S] = True
    _bwd_gap(_bwd_mutant(0, drop={(0, 9): drop}))


def test_mutant_hsplit_part_missing():
    """One hsplit part missing: the last 128-key block's dK / dV lack the query heads of one of 8 parts (GQA 8: one
    query head of the group, every query tile of the block)."""
    S, G = BWD_C[1], BWD_C[3] // BWD_C[4]
    drop = torch.zeros(S, S, dtype=torch.bool)
    drop[:, S - 128:S] = True
    _bwd_gap(_bwd_mutant(1, drop={(0, 2 * G + 3): drop}))


# ------------------------------------------------------------------------------------------ plan coverage
def _plans(tmp_path, rows, cus=256):
    """SplitPlan fields of (D, causal, B, Sq, Sk, Hq, Hkv, kvp, waves, groups) rows, from the plan header itself
    (tests/attn_bwd_plan_check.cpp in its printing mode, built as tests/test_attn_bwd_plan.py builds it)."""
    from picotron_amd import build
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_bwd_plan_check.cpp")
    exe = str(tmp_path / "attn_bwd_plan_check")
    subprocess.run([build.HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-nogpuinc", "-nogpulib",
                    "-o", exe, src], check=True)
    args = [str(int(x)) for row in rows for x in (*row, cus)]
    out = subprocess.run([exe, *args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    names = ("kvp", "waves", "kvb", "minb", "hsplit", "grp_n", "q_front", "q_grid", "kv_grid", "bytes")
    return [dict(zip(names, map(int, line.split()))) for line in out.stdout.splitlines()]


def test_case_table_reaches_every_plan_path(tmp_path):
    """At 256 CUs the GPU file's backward cases reach, for each of the five dK/dV kernels: the plain grid with
    hsplit 1, hsplit 2, 4 and 8, the causal block groups and the plain grid of the same shape
    (PICO_SEL_ATTN_GROUPS = 0); the 32-row D = 64 kernel at 3 (causal) and 2 (non-causal) workgroups per CU; the dQ
    kernel with and without a lightest-first front at both head dims, the front in all three output forms; and the
    persistent forward's cases reach single, unpaired and paired items."""
    import test_attn_tiles_gpu as T
    rows, meta = [], []
    for kern, causal, B, Sq, Sk, Hq, Hkv, groups, mode, _ in T.BWD_CASES:
        D, kvp, waves = T.KV_KERNELS_ALL[kern]
        for grp in ((T.AUTO, 0) if groups == "pair" else (groups,)):
            rows.append((D, causal, B, Sq, Sk, Hq, Hkv, kvp, waves, grp))
            meta.append((kern, causal, grp, mode, D))
    plans = _plans(tmp_path, rows)
    assert len(plans) == len(rows)
    print("kernel   causal B Sq Sk Hq Hkv groups mode | kvb minb hsplit grp.n q_front kv_grid")
    seen = set()
    for row, (kern, causal, grp, mode, D), p in zip(rows, meta, plans):
        print(f"{kern:9s}", int(causal), *row[2:7], grp, mode, "|", p["kvb"], p["minb"], p["hsplit"], p["grp_n"],
              p["q_front"], p["kv_grid"])
        seen.add(("front" if p["q_front"] > 0 else "nofront", D))
        if p["q_front"] > 0:
            seen.add(("front", D, mode))
        if kern not in T.KV_KERNELS:
            continue
        _, kvp, waves = T.KV_KERNELS[kern]
        assert p["kvp"] == kvp and p["kvb"] == (256 if waves == 8 else 128), (kern, row, p)
        seen.add((kern, "hsplit", p["hsplit"]))
        seen.add((kern, "minb", p["minb"]))
        if p["hsplit"] == 1 and p["grp_n"] == 0:
            seen.add((kern, "plain"))
        if p["hsplit"] > 1 and mode == "rope":
            seen.add((kern, "rope in attn_bwd_dkv_kernel"))
        if p["hsplit"] == 1 and mode == "rope":
            seen.add((kern, "rope direct"))
        if p["grp_n"] > 0:
            seen.add((kern, "grouped"))
            twin = rows.index(row[:9] + (0,))  # the same shape with the groups switched off
            assert plans[twin]["grp_n"] == 0 and plans[twin]["hsplit"] == 1 and plans[twin]["kv_grid"] > p["kv_grid"]
            seen.add((kern, "ungrouped twin"))
    want = set()
    for kern in T.KV_KERNELS:
        want |= {(kern, "plain"), (kern, "grouped"), (kern, "ungrouped twin"), (kern, "rope direct"),
                 (kern, "rope in attn_bwd_dkv_kernel")} | {(kern, "hsplit", h) for h in (1, 2, 4, 8)}
    want |= {("kv32d64", "minb", 3), ("kv32d64", "minb", 2), ("kvp64w4", "minb", 2), ("kvp64w8", "minb", 1),
             ("kvp128", "minb", 1), ("kv32d128", "minb", 1)}
    want |= {(f, D) for f in ("front", "nofront") for D in (64, 128)}
    want |= {("front", D, mode) for D in (64, 128) for mode in ("bf16", "f32acc", "rope")}
    assert not want - seen, sorted(want - seen, key=str)
    # the persistent forward: nJ = ceil(Sq / 256) items per head, paired when nbh * ceil(nJ / 2) >= CUs (attn_fwdp.hip)
    kinds = set()
    for B, Sq, Sk, Hq, Hkv, causal in T.FWDP_CASES:
        assert Sq % 64 == 0 and Sk % 64 == 0 and (Sq == Sk or not causal)  # accepted by pico_attn_fwdp
        nJ = -(-Sq // 256)
        paired = causal and nJ > 1 and B * Hq * ((nJ + 1) // 2) >= 256
        kinds.add("paired" if paired else "one item" if nJ == 1 else "unpaired")
        if causal and (Sq // 64) % 2 == 1 and nJ > 1 and Sq % 256:  # an odd number of 64-key tiles, a partial last item
            kinds.add("odd blocks, partial last")
        if not causal:
            kinds.add("full" if Sq == Sk else "cross")
        if paired and Hq != Hkv:
            kinds.add("paired GQA")
    assert kinds >= {"paired", "paired GQA", "one item", "unpaired", "odd blocks, partial last", "full", "cross"}, kinds
    for D, B, Sq, Sk, H, causal in T.FWDP_FALLBACK:
        assert D != 64 or Sq % 64 or Sk % 64  # refused by pico_attn_fwdp: the 32-row kernel runs
