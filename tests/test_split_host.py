"""The checks of tests/test_split_gpu.py, tried on the CPU first (tests/split_ref.py): the fp32 restatements of the
ring merge and of split-KV decode pass their bounds with half the budget, restatements with one deliberate mistake
fail them (and many of those pass the criteria the suite had before: printed per mutant), the case tables reach every
kernel instance and loop path (asserted from csrc/attn_decode_plan.h and csrc/attn_merge_plan.h through
tests/attn_merge_plan_check.cpp), the merge's lane mapping never splits a row over two waves, and the entry points
refuse misaligned pointers, bad strides and bad head dims. CPU only."""
import ctypes
import math
import os
import subprocess

import pytest
import torch

import split_ref as SR
from picotron_amd import build

BF, F32 = torch.bfloat16, torch.float32
HERE = os.path.dirname(os.path.abspath(__file__))


def compile_check(tmp_path):
    exe = str(tmp_path / "attn_merge_plan_check")
    # host only: the plan headers must compile without the HIP headers
    subprocess.run([build.HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-nogpuinc", "-nogpulib",
                    "-o", exe, os.path.join(HERE, "attn_merge_plan_check.cpp")], check=True)
    return exe


def _describe(exe, cases):
    r = subprocess.run([exe, *cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        head, *kv = line.split()
        out[head] = {k: int(v) for k, v in (p.split("=") for p in kv)}
    return out


# ------------------------------------------------------------------------------------------ the merge plan
def test_merge_plan_sweep(tmp_path):
    r = subprocess.run([compile_check(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout


# ------------------------------------------------------------------------------------------ merge: restatement
@pytest.mark.parametrize("f32_block", [False, True])
@pytest.mark.parametrize("kind", SR.MERGE_KINDS)
def test_restated_merge(kind, f32_block):
    worst = {}
    for D in SR.MERGE_DIMS:
        out, lse, bo, bl = SR.make_merge(kind, *SR.MERGE_SHAPE, D, f32_block)
        got = SR.restate_merge(out, lse, bo, bl)
        assert torch.isfinite(got["out"]).all() and torch.isfinite(got["lse"]).all()
        SR.check_merge(f"merge {kind} D={D}", got, SR.ref_merge(out, lse, bo, bl), SR.K_ELEM / 2, worst)
        if kind == "empty":
            assert torch.equal(got["out"].view(torch.int32), out.view(torch.int32))
            assert torch.equal(got["lse"].view(torch.int32), lse.view(torch.int32))
    print("worst K", worst)


def test_convex_condition_term_is_wrong_for_the_sigmoid_form():
    """(1 - w) |out| + w |block_out|, the condition term of the convex form, does not bound the kernel's form
    out - w (out - block_out): where w is ~1 and block_out ~0 the result is tiny and the error stays an ulp of
    |out - block_out|. The honest restatement then needs K in the thousands; with cond_out it needs under 4."""
    out, lse, bo, bl = SR.make_merge("gaps", *SR.MERGE_SHAPE, 8)
    bo = (bo.float() * torch.where(torch.arange(bo.shape[1])[None, :, None, None] % 2 == 0, 1.0, 1e-4)).to(BF)
    ref, cond = SR.ref_merge(out, lse, bo, bl)["out"]
    got = SR.restate_merge(out, lse, bo, bl)["out"]
    w = (cond - out.double().abs()) / (out.double() - bo.double()).abs().clamp_min(1e-300)
    convex = (1 - w) * out.double().abs() + w * bo.double().abs()
    k_convex = SR.R.elem_check("out", got, ref, convex, F32)["k"]
    k_cond = SR.R.elem_check("out", got, ref, cond, F32)["k"]
    print(f"restated merge: K needed with the convex term {k_convex:.0f}, with cond_out {k_cond:.2f}")
    assert k_convex > 1000 and k_cond < SR.K_ELEM / 2


def test_restated_merge_first():
    out, lse, bo, bl = SR.make_merge("gaps", 1, 33, 3, 40)
    got = SR.restate_merge(out, lse, bo, bl, first=True)
    assert torch.equal(got["out"], bo.float()) and torch.equal(got["lse"], bl)


def test_gaps_reach_every_wave_position():
    """Every signed gap occurs at a row that straddled a wave under the unpadded mapping, and at one that did not,
    for every D of the table whose rows straddled at all."""
    rows = math.prod(SR.MERGE_SHAPE)
    gi = SR.gap_of_rows(rows)
    n = len(SR.SIGNED_GAPS)
    odd = []
    for D in SR.MERGE_DIMS:
        st = SR.straddles(rows, D).any(-1)
        if not bool(st.any()):
            assert (D // 8) & (D // 8 - 1) == 0
            continue
        odd.append(D)
        assert int(st.sum()) >= 100, (D, int(st.sum()))
        assert set(gi[st].tolist()) == set(range(n)) and set(gi[~st].tolist()) == set(range(n)), D
    assert odd == [24, 40, 96, 136]
    _, lse, _, bl = SR.make_merge("gaps", *SR.MERGE_SHAPE, 8)
    d = (bl.double() - lse.double()).permute(0, 2, 1).reshape(-1)
    want = torch.tensor(SR.SIGNED_GAPS, dtype=torch.float64)[gi]
    assert float((d - want).abs().max()) < 1e-3  # the fp32 rounding of lse + 1e4


def test_chain_reference_is_the_whole_softmax():
    """The fp64 chain over exact partial results is the whole softmax; on the rounded partials it is the reference
    of the chain check, which the restated chain meets with half the budget K_ELEM (N - 1)."""
    n = 8
    blocks, whole = SR.make_chain(n, 1, 67, 3, 40)
    r_ = SR.ref_chain(blocks)
    assert float((r_["out"][0] - whole[0]).abs().max()) < 1e-12 and float((r_["lse"][0] - whole[1]).abs().max()) < 1e-12
    rounded = [(bo.to(BF), bl.float()) for bo, bl in blocks]
    worst = {}
    SR.check_merge(f"chain N={n}", SR.restate_chain(rounded), SR.ref_chain(rounded), SR.K_ELEM * (n - 1) / 2, worst)
    print("worst K over the chain", worst, "per merge", {k: v / (n - 1) for k, v in worst.items()})


# ------------------------------------------------------------------------------------------ merge: mutants
def _merge_old_ok(got, ref):
    return all(float((got[n].double() - ref[n][0]).abs().max()) < SR.OLD_MERGE_TOL for n in ref)


@pytest.mark.parametrize("mut", SR.MERGE_MUTANTS)
def test_mutant_merge(mut):
    D = 96  # 12 lanes per row: rows 5 and 10 of every 16 straddled a wave
    first = mut == "first_ignored"
    new_fails, old_passes = [], []
    for kind in ("randn", "gaps"):
        out, lse, bo, bl = SR.make_merge(kind, *SR.MERGE_SHAPE, D)
        if first:
            ref = {"out": (bo.double(), bo.double().abs()), "lse": (bl.double(), bl.double().abs())}
        else:
            ref = SR.ref_merge(out, lse, bo, bl)
        assert all(r_["ok"] for r_ in SR.merge_results(SR.restate_merge(out, lse, bo, bl, first=first), ref))
        got = SR.restate_merge(out, lse, bo, bl, first=first, mut=mut)
        res = SR.merge_results(got, ref)
        new_fails.append(not all(r_["ok"] for r_ in res))
        old_passes.append(_merge_old_ok(got, ref))
        print(f"MUTANT merge {mut} {kind}: new check worst ratio {max(r_['ratio'] for r_ in res):.3g} "
              f"({'fails' if new_fails[-1] else 'passes'}); old criterion max_abs < 1e-5 on the same data "
              f"{'passes' if old_passes[-1] else 'fails'}")
    assert all(new_fails)
    if mut == "race":
        # what the suite ran before: D = 64 and 128 only, where no row straddles: the mutant is the kernel itself
        for D2 in (64, 128):
            out, lse, bo, bl = SR.make_merge("randn", 2, 33, 4, D2)
            a, b = SR.restate_merge(out, lse, bo, bl), SR.restate_merge(out, lse, bo, bl, mut=mut)
            assert torch.equal(a["out"], b["out"]) and torch.equal(a["lse"], b["lse"])
        print("MUTANT merge race: invisible at D = 64 and 128, the only head dims the suite ran")


# ------------------------------------------------------------------------------------------ decode: restatement
HOST_DECODE = [(D, G, split, kind) for D in SR.DEC_DIMS for G, split, kind in (
    (1, 7, "randn"), (3, "t+1", "ascending"), (5, "2t+5", "descending"), (8, "2t+5", "ascending"), (2, 32, "large"),
    (7, None, "randn"), (4, "s8", "large"))]


def _split(D, split):
    t = SR.dec_trip(D)
    return {"t+1": t + 1, "2t+5": 2 * t + 5, "s8": SR.dec_split8(D), None: SR.DEC_DEFAULT}.get(split, split)


@pytest.mark.parametrize("D,G,split,kind", HOST_DECODE)
def test_restated_decode(D, G, split, kind):
    """The fp32 restatement of the kernels, at the case's own split, against the bound built from the emulation at
    split_keys = 32: half the margin's room (ratio <= 0.5) and half of K_ELEM."""
    split = _split(D, split)
    lens = SR.dec_lens(D, split)
    q, k, v, lt = SR.make_decode(kind, G, D, lens)
    scale = 1.0 / math.sqrt(D)
    ref = SR.decode_ref(q, k, v, lt, scale, 32)
    o, lse = SR.restate_decode(q, k, v, lt, scale, split)
    res = SR.decode_check(f"restated D={D} G={G} split={split} {kind}", o, lse, ref, k=SR.K_ELEM / 2)
    assert res["ok"] and res["ratio"] <= 0.5, res


def test_inputs_do_what_they_say():
    D, G = 64, 4
    lens = (SR.dec_smax(D),)
    scale = 1.0 / math.sqrt(D)
    for kind in ("ascending", "descending"):
        q, k, v, _ = SR.make_decode(kind, G, D, lens, stale_nan=False)
        s = torch.einsum("bhd,bhsd->bhs", q[:, ::G].double(), k.double()) * scale
        d = s[..., 1:] - s[..., :-1]
        assert float(s.max()) > 29 and float(s.min()) < -29
        assert bool((d > 0).all()) if kind == "ascending" else bool((d < 0).all()), kind
    q, k, v, _ = SR.make_decode("large", G, D, lens, stale_nan=False)
    s = torch.einsum("bhgd,bhsd->bhgs", q.double().view(1, 2, G, D), k.double()) * scale
    assert float(s.abs().max()) > 45
    q, k, v, lt = SR.make_decode("randn", G, D, (-3, 0, 5, 400))
    assert torch.isnan(k[0]).all() and torch.isnan(v[1]).all() and torch.isnan(k[2, :, 5:]).all()
    assert not torch.isnan(k[2, :, :5]).any() and not torch.isnan(k[3]).any()


# ------------------------------------------------------------------------------------------ decode: mutants
@pytest.mark.parametrize("mut,split,kind", [
    ("drop_chunk_start", 32, "randn"), ("drop_trip", "2t+5", "randn"), ("drop_group", "t+1", "randn"),
    ("leak_len", 32, "randn"), ("no_alpha", "2t+5", "ascending"), ("kv_neighbour", 32, "randn"),
    ("combine8", 7, "randn"), ("empty_o", 32, "randn")])
def test_mutant_decode(mut, split, kind):
    D, G = 64, 2
    split = _split(D, split)
    lens = SR.dec_lens(D, split)
    scale = 1.0 / math.sqrt(D)
    q, k, v, lt = SR.make_decode(kind, G, D, lens, stale_nan=mut != "leak_len")
    ref = SR.decode_ref(q, k, v, lt, scale, 32)
    assert SR.decode_check(f"restated for {mut}", *SR.restate_decode(q, k, v, lt, scale, split), ref)["ok"]
    o, lse = SR.restate_decode(q, k, v, lt, scale, split, mut=mut)
    res = SR.decode_check(f"mutant {mut}", o, lse, ref)
    # the suite's earlier decode tests: randn, lengths (1, 31, 32, 33, 160) of a 160-key cache, split_keys = 32
    q2, k2, v2, lt2 = SR.make_decode("randn", G, D, (1, 31, 32, 33, 160), S=160, stale_nan=False)
    ref2 = SR.decode_ref(q2, k2, v2, lt2, scale, 32)
    old = SR.decode_old_ok(*SR.restate_decode(q2, k2, v2, lt2, scale, 32, mut=mut), ref2)
    print(f"MUTANT decode {mut}: new check O ratio {res['ratio']:.3g}, LSE K {res['k']:.3g} "
          f"({'passes' if res['ok'] else 'fails'}); old criterion on the new inputs "
          f"{'passes' if SR.decode_old_ok(o, lse, ref) else 'fails'}, on the old tests' inputs "
          f"{'passes' if old else 'fails'}")
    assert not res["ok"]


# ------------------------------------------------------------------------------------------ every path is reached
def test_case_tables_reach_every_path(tmp_path):
    exe = compile_check(tmp_path)
    consts = _describe(exe, ["decode_consts"])["decode_consts"]
    assert consts["unroll"] == SR.DEC_UNROLL and consts["threads"] == 256
    cases = SR.dec_cases()
    # all <D, G> instances of attn_decode_kernel: D in {64, 128} x G in 1..DEC_MAX_GROUP
    instances = {(D, G) for D in SR.DEC_DIMS for G in range(1, consts["max_group"] + 1)}
    assert len(instances) == 16 and {(D, G) for D, G, _, _ in cases} == instances
    plan = {}
    for D in SR.DEC_DIMS:
        splits = [s for s in SR.dec_splits(D) if s is not None] + [SR.DEC_DEFAULT]
        d = _describe(exe, [f"decode:{D}:{s}:{SR.dec_smax(D)}" for s in splits])
        for s in splits:
            plan[(D, s)] = d[f"decode:{D}:{s}:{SR.dec_smax(D)}"]
            assert plan[(D, s)]["trip"] == SR.dec_trip(D) and plan[(D, s)]["groups"] == SR.dec_ng(D)
        assert SR.dec_smax(D) == 2 * SR.dec_trip(D) + 37
    for inst in instances:
        mine = [(s, kind) for D, G, s, kind in cases if (D, G) == inst]
        D = inst[0]
        at = lambda s: plan[(D, SR.DEC_DEFAULT if s is None else s)]  # noqa: E731
        # ascending at a split whose chunks take two and three loop trips; randn at split 7 (many chunks)
        assert {at(s)["chunk_trips"] for s, kind in mine if kind == "ascending"} >= {2, 3}, inst
        assert any(s == 7 and kind == "randn" and at(s)["nsplit"] > 8 for s, kind in mine), inst
    for D in SR.DEC_DIMS:  # both combine instances: fewer chunks than its unroll of 8, exactly 8, whole trips, a tail
        ns = {plan[(D, SR.DEC_DEFAULT if s is None else s)]["nsplit"] for d_, _, s, _ in cases if d_ == D}
        assert 8 in ns and any(n < 8 for n in ns) and any(n > 8 and n % 8 for n in ns), (D, ns)
        assert {s for d_, _, s, _ in cases if d_ == D} == set(SR.dec_splits(D))
        assert {kind for d_, _, _, kind in cases if d_ == D} == set(SR.DEC_KINDS)
    # merge: both BO_F32 instances x first x both layouts; every D; the lane groups of the plan header
    mc = SR.merge_cases()
    assert {(f32, first, layout) for _, _, f32, first, layout in mc} == {(a, b, c) for a in (False, True)
                                                                          for b in (False, True) for c in ("bshd", "bhsd")}
    assert {(D, kind) for D, kind, *_ in mc} >= {(D, kind) for D in SR.MERGE_DIMS for kind in SR.MERGE_KINDS}
    rows = math.prod(SR.MERGE_SHAPE)
    assert rows >= 4096
    d = _describe(exe, [f"merge:{rows}:{D}" for D in SR.MERGE_DIMS])
    for D in SR.MERGE_DIMS:
        p = d[f"merge:{rows}:{D}"]
        row, sub, live = SR.plan_lanes(rows, D)
        assert p["lpr"] == D // 8 and p["grid"] * 256 == row.numel() and p["grid"] > 1
        assert p["straddle"] == int(SR.straddles(rows, D).any(-1).sum())
        pow2 = (D // 8) & (D // 8 - 1) == 0
        assert (p["group"] == p["lpr"]) == pow2 and (p["straddle"] == 0) == pow2
        if not pow2:
            assert p["straddle"] >= 100  # hundreds of rows that the unpadded mapping split over two waves
        prow, psub = SR.parent_lanes(rows, D)
        same = bool(live[:prow.numel()].all()) and torch.equal(row[:prow.numel()], prow) and \
            torch.equal(sub[:psub.numel()], psub) and not bool(live[prow.numel():].any())
        assert same == pow2, D  # D = 64, 128: every lane does what it did before; the odd D are remapped
    assert {p["group"] for p in d.values()} == {1, 4, 8, 16, 32}


# ------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def lib():
    from picotron_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def _merge_call(lib, out=4096, lse=4096, bo=4096, bl=4096, ost=(4096, 512, 64), bst=(4096, 512, 64), f32=0, D=64,
                B=2, S=8, H=8):
    from picotron_amd import _lib
    vp = ctypes.c_void_p
    lst = _lib.i64x3((64, 8, 1))
    return lib.pico_attn_merge(vp(out), _lib.i64x3(ost), vp(lse), lst, vp(bo), _lib.i64x3(bst), f32, vp(bl), lst, B, S, H,
                               D, 0, None)


def test_merge_refusals(lib):
    """Fake pointers, never dereferenced: the entry point returns before any launch."""
    err = lib.pico_last_error
    assert _merge_call(lib, out=None) == 1000 and b"null" in err()
    assert _merge_call(lib, out=4096 + 8) == 1000 and b"16-byte aligned" in err()
    assert _merge_call(lib, bo=4096 + 8) == 1000 and b"16-byte aligned" in err()
    assert _merge_call(lib, bo=4096 + 8, f32=1) == 1000 and b"16-byte aligned" in err()
    assert _merge_call(lib, ost=(4096, 512, 66)) == 1000 and b"strides" in err()
    assert _merge_call(lib, bst=(4096, 516, 64)) == 1000 and b"strides" in err()       # bf16: multiples of 8
    assert _merge_call(lib, bst=(4098, 512, 64), f32=1) == 1000 and b"strides" in err()  # fp32: multiples of 4
    for D in (0, -8, 4, 12, 100, 264, 512):
        assert _merge_call(lib, D=D) == 1000 and b"head_dim" in err(), D
    assert _merge_call(lib, B=-1) == 1000 and _merge_call(lib, B=1 << 20, S=1 << 20) == 1000
    assert _merge_call(lib, B=0) == 0  # nothing to do, nothing launched


def test_decode_refuses_misaligned_pointers(lib):
    from picotron_amd import _lib
    vp = ctypes.c_void_p
    st = _lib.i64x3((16384, 8192, 64))
    for i in range(5):  # q, k_cache, v_cache, o, workspace
        a = [vp(4096 + 8 if j == i else 4096) for j in range(5)]
        rc = lib.pico_attn_decode(a[0], (_lib.c_i64 * 2)(256, 64), a[1], st, a[2], st, vp(4096), a[3], vp(4096), a[4], 2,
                                  4, 2, 128, 64, 0.125, 0, None)
        assert rc == 1000 and b"16-byte aligned" in lib.pico_last_error(), i
