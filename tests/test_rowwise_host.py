"""The per-element check of the row-wise kernels (tests/rowwise_ref.py) proves itself on the CPU: every restatement
passes it against its fp64 reference on every input set at the shapes of the GPU tables with the K term halved,
mutants (a restatement with one planted mistake) fail it — several of them while passing the whole-tensor rel_l2
thresholds the kernels were judged by — the GPU case tables reach every instantiation and every second loop trip
(printed by tests/rowwise_plan_check.cpp), and the entry points refuse misaligned pointers, short row strides and a
negative gradient scale. CPU only."""
import ctypes
import os
import subprocess

import pytest
import torch

import rowwise_ref as R
from test_rowwise_plan import compile_check

HALF = R.K_ELEM / 2
EPS = 1e-5
BF, F32 = R.BF, R.F32


def _fails(got, ref, k=R.K_ELEM):
    """True when at least one output of the mutant misses the bound."""
    res = [R.elem_check(n, got[n], r_, c_, got[n].dtype, k) for n, (r_, c_) in ref.items() if n in got]
    return any(not r_["ok"] for r_ in res), max(r_["ratio"] for r_ in res)


# ------------------------------------------------------------------------------------------ restatements pass
@pytest.mark.parametrize("cols", R.RMS_FWD_COLS)
def test_restated_rmsnorm_fwd(cols):
    for rows in R.RMS_FWD_ROWS:
        for kind in R.KINDS:
            x, res, w = R.make(kind, rows, cols), R.make(kind, rows, cols, 1), R.make("randn", 1, cols, 2)[0]
            for rr in (None, res):
                R.check_all(f"rms_fwd {rows}x{cols} {kind} res{rr is not None}", R.restate_rmsnorm_fwd(x, w, EPS, rr),
                            R.ref_rmsnorm_fwd(x, w, EPS, rr), HALF)
    for rows, c in R.RMS_FWD_T:
        if c == cols:
            x, w = R.make("randn", rows, c), R.make("randn", 1, c, 2)[0]
            R.check_all(f"rms_fwd_t {rows}x{c}", R.restate_rmsnorm_fwd(x, w, EPS), R.ref_rmsnorm_fwd(x, w, EPS), HALF)


def _bwd_inputs(kind, rows, cols):
    x, dy, dres = R.make(kind, rows, cols), R.make(kind, rows, cols, 1), R.make(kind, rows, cols, 3)
    w = R.make("randn", 1, cols, 2)[0]
    rstd = R.restate_rmsnorm_fwd(x, w, EPS)["rstd"]
    g0 = R.make("randn", 1, cols, 4)[0]
    return x, dy, dres, w, rstd, g0


@pytest.mark.parametrize("cols", R.RMS_BWD_COLS)
def test_restated_rmsnorm_bwd(cols):
    for rows in R.rms_bwd_rows(cols):
        for kind in R.KINDS:
            x, dy, dres, w, rstd, g0 = _bwd_inputs(kind, rows, cols)
            for dr in (None, dres):
                got = R.restate_rmsnorm_bwd(dy, x, w, rstd, dr)
                t = R.dw_reduce_separate(got["part"])
                for mode, g in ((0, None), (1, g0), (2, g0.float())):
                    got["dw"] = R.dw_finish(t, mode, g, 0.25)
                    R.check_all(f"rms_bwd {rows}x{cols} {kind} dres{dr is not None} mode{mode}", got,
                                R.ref_rmsnorm_bwd(dy, x, w, rstd, dr, mode, g, 0.25), HALF)


def test_restated_chained_dw():
    for rows, cols, pc in R.RMS_CHAIN:
        nw = R.bwd_waves(R.maxc_for(cols))
        for nb in R.CHAIN_NB:
            for kind in R.KINDS:
                part = R.make(kind, nb, pc, 5).float() * 1.37
                g0 = R.make("randn", 1, pc, 4)[0]
                for mode, g in ((0, None), (1, g0), (2, g0.float())):
                    ref = R.ref_dw_reduce(part, mode, g, 0.25)
                    for name, t in (("chained", R.dw_reduce_chained(part, nw)), ("separate", R.dw_reduce_separate(part))):
                        R.check_all(f"dw {name} nw{nw} nb{nb} cols{pc} {kind} mode{mode}",
                                    {"dw": R.dw_finish(t, mode, g, 0.25)}, ref, HALF)
                if nb == 1:  # one partial row: both orders add it to zero, the same bits
                    assert torch.equal(R.dw_reduce_chained(part, nw), R.dw_reduce_separate(part))


def _rope_inputs(kind, B, S, Hh, D, rows=None):
    x = R.make(kind, B * S * Hh, D).view(B, S, Hh, D)
    cos, sin = R.A.rope_tables(rows or S, D, base=10000.0)
    return x, cos, sin


@pytest.mark.parametrize("D", R.ROPE_D)
def test_restated_rope(D):
    for Hh in R.ROPE_H:
        for S in R.ROPE_S:
            for B in R.ROPE_B:
                for kind in R.KINDS:
                    x, cos, sin = _rope_inputs(kind, B, S, Hh, D)
                    for conj in (False, True):
                        got = R.restate_rope(x, cos, sin, conj)
                        assert torch.equal(got["out"], R.H.rope_fused(x, cos, sin, conj))
                        R.check_all(f"rope D{D} H{Hh} S{S} B{B} {kind} conj{conj}", got, R.ref_rope(x, cos, sin, conj), 0.0)


def test_restated_rope_big_slice():
    """The large case, on the slice the GPU test holds against fp64: the last batch's last 8 positions."""
    B, S, Hh, D = R.ROPE_BIG
    x = R.make("randn", 8 * Hh, D).view(1, 8, Hh, D)
    cos, sin = R.A.rope_tables(S, D, base=10000.0)
    got = R.restate_rope(x, cos[S - 8:], sin[S - 8:])
    R.check_all("rope big slice", got, R.ref_rope(x, cos[S - 8:], sin[S - 8:]), 0.0)


@pytest.mark.parametrize("rows,cols,fused,shift", R.SWIGLU_CASES + list(R.SWIGLU_BIG))
def test_restated_swiglu(rows, cols, fused, shift):
    for kind in R.KINDS:
        g, u, dh = R.make(kind, rows, cols), R.make(kind, rows, cols, 1), R.make(kind, rows, cols, 2)
        R.check_all(f"swiglu fwd {rows}x{cols} {kind}", R.restate_swiglu_fwd(g, u), R.ref_swiglu_fwd(g, u), HALF)
        R.check_all(f"swiglu bwd {rows}x{cols} {kind}", R.restate_swiglu_bwd(dh, g, u), R.ref_swiglu_bwd(dh, g, u), HALF)


@pytest.mark.parametrize("rows,cols", R.SWIGLU_T)
def test_restated_swiglu_t(rows, cols):
    for kind in R.KINDS:
        g, u = R.make(kind, rows, cols), R.make(kind, rows, cols, 1)
        R.check_all(f"swiglu fwd_t {rows}x{cols} {kind}", R.restate_swiglu_fwd(g, u), R.ref_swiglu_fwd(g, u), HALF)


@pytest.mark.parametrize("V", sorted(set(R.CE_VOCABS_256 + R.CE_VOCABS_512)))
def test_restated_ce(V):
    for kind in R.KINDS:
        x, t = R.make_ce(kind, V)
        if V in R.CE_VOCABS_512:
            got = R.restate_ce(x, t, R.CE_GSCALE, "fwd_grad")
            R.check_all(f"ce fwd_grad V{V} {kind}", got, R.ref_ce(x, t, R.CE_GSCALE), HALF)
        if V in R.CE_VOCABS_256:
            got = R.restate_ce(x, t, R.CE_GSCALE, "bwd")
            ref = R.ref_ce(x, t, R.CE_GSCALE, lse_in=got["lse"])
            R.check_all(f"ce fwd+bwd V{V} {kind}", got, ref, HALF)
            for splits in ((0, V), (0, max(8, V // 16 * 8), V)):
                if len(set(splits)) != len(splits):
                    continue
                got = R.restate_ce_vp(x, t, splits, R.CE_GSCALE)
                ref = R.ref_ce(x, t, R.CE_GSCALE, lse_in=got["lse"])
                R.check_all(f"ce vp V{V} {splits} {kind}", got, ref, HALF)


def test_restated_scale():
    x = R.make("wide", 1, R.SCALE_N)[0]
    for s in (0.3, -1.7):
        R.check_all(f"scale {s}", R.restate_scale(x, s), R.ref_scale(x, s), HALF)


@pytest.mark.parametrize("dim", R.EMB_DIMS)
def test_restated_embedding(dim):
    for n in R.EMB_N:
        for dt in (BF, F32):
            for kind in R.ID_KINDS:
                ids = R.make_ids(kind, n, R.EMB_V)
                dy = R.make("randn" if kind == "random" else "bait", n, dim, 1)
                g0 = R.make("randn", R.EMB_V, dim, 2).to(dt)
                got = R.restate_embedding(g0, ids, dy, 0.5)
                R.check_all(f"emb n{n} dim{dim} {dt} {kind}", got, R.ref_embedding(g0, ids, dy, 0.5), HALF)
                untouched = torch.ones(R.EMB_V, dtype=torch.bool)
                untouched[ids] = False
                assert torch.equal(got["grad"][untouched], g0[untouched])


# ------------------------------------------------------------------------------------------ mutants fail
def _old_ok(got, ref, tol=R.OLD_TOL):
    return all(R.rel_l2(got[n], r_) < tol for n, (r_, _) in ref.items() if n in got and n != "rstd")


@pytest.mark.parametrize("mut,cols,old", [("tail", 16, True), ("mean512", 520, True), ("rstd_next", 8, False),
                                          ("res_unrounded", 64, True)])
def test_mutant_rmsnorm_fwd(mut, cols, old):
    rows = 5
    res = R.make("bait", rows, cols, 1)
    x, w = R.make("bait", rows, cols), R.make("randn", 1, cols, 2)[0]
    rr = res if mut == "res_unrounded" else None
    ref = R.ref_rmsnorm_fwd(x, w, EPS, rr)
    assert not _fails(R.restate_rmsnorm_fwd(x, w, EPS, rr), ref)[0]
    bad, ratio = _fails(R.restate_rmsnorm_fwd(x, w, EPS, rr, mut=mut), ref)
    print(f"mutant {mut}: worst ratio {ratio:.3g}")
    assert bad
    if old:  # the workload's 2048 columns, randn, judged by rel_l2 < 4e-3 over the whole tensor: the mutant passes
        x, w, res = R.make("randn", 64, 2048), R.make("randn", 1, 2048, 2)[0], R.make("randn", 64, 2048, 1)
        rr = res if mut == "res_unrounded" else None
        assert _old_ok(R.restate_rmsnorm_fwd(x, w, EPS, rr, mut=mut), R.ref_rmsnorm_fwd(x, w, EPS, rr))


@pytest.mark.parametrize("mut", ["part_missing", "mode1_as_2"])
def test_mutant_rmsnorm_bwd(mut):
    rows, cols = 33, 8  # 16 waves: three workgroups, the last with one row
    x, dy, _, w, rstd, g0 = _bwd_inputs("bait", rows, cols)
    mode, g = (2, g0.float()) if mut == "mode1_as_2" else (0, None)
    ref = R.ref_rmsnorm_bwd(dy, x, w, rstd, None, mode, g, 0.25)
    assert not _fails(R.restate_rmsnorm_bwd(dy, x, w, rstd, None, mode, g, 0.25), ref)[0]
    bad, ratio = _fails(R.restate_rmsnorm_bwd(dy, x, w, rstd, None, mode, g, 0.25, mut=mut), ref)
    print(f"mutant {mut}: worst ratio {ratio:.3g}")
    assert bad


@pytest.mark.parametrize("mut", ["no_conj", "flat_pos", "fma"])
def test_mutant_rope(mut):
    if mut != "fma":
        B, S, Hh, D = 2, 3, 1, 16
        x, cos, sin = _rope_inputs("randn", B, S, Hh, D, rows=B * S)
        good = R.restate_rope(x, cos, sin, True)
        got = R.restate_rope(x, cos, sin, True, mut=mut)
        assert not torch.equal(got["out"], good["out"])  # the bit-equality check of the GPU test
        assert not _fails(good, R.ref_rope(x, cos, sin, True), 0.0)[0]
        assert _fails(got, R.ref_rope(x, cos, sin, True), 0.0)[0]
    else:
        # The products of two bf16 values have 16-bit significands: exact in fp32, rounded or not. Contracting one of
        # them into a fused multiply-add therefore changes no bit, for any bf16 x and bf16 tables: there is nothing
        # for the bit-equality check to see, and no rounding that the kernel's __fmul_rn could lose.
        for kind in R.KINDS:
            x, cos, sin = _rope_inputs(kind, 2, 37, 3, 64)
            assert torch.equal(R.restate_rope(x, cos, sin, mut=mut)["out"], R.restate_rope(x, cos, sin)["out"])


@pytest.mark.parametrize("mut", ["no_term", "swapped", "halves"])
def test_mutant_swiglu(mut):
    g, u, dh = R.make("randn", 1, 8), R.make("randn", 1, 8, 1), R.make("randn", 1, 8, 2)
    if mut == "halves":
        assert not _fails(R.restate_swiglu_fwd(g, u), R.ref_swiglu_fwd(g, u))[0]
        assert _fails(R.restate_swiglu_fwd(g, u, mut=mut), R.ref_swiglu_fwd(g, u))[0]
    else:
        assert not _fails(R.restate_swiglu_bwd(dh, g, u), R.ref_swiglu_bwd(dh, g, u))[0]
        assert _fails(R.restate_swiglu_bwd(dh, g, u, mut=mut), R.ref_swiglu_bwd(dh, g, u))[0]


@pytest.mark.parametrize("mut,V,old", [("t_plus_1", 8, False), ("ignored_grad", 8, False),
                                       ("max_first_pass", 4104, True), ("tail_chunk", 4104, True)])
def test_mutant_ce(mut, V, old):
    x, t = R.make_ce("bait", V)
    for form in ("fwd_grad", "bwd"):
        ref = R.ref_ce(x, t, R.CE_GSCALE)
        good = R.restate_ce(x, t, R.CE_GSCALE, form)
        if form == "bwd":
            ref = R.ref_ce(x, t, R.CE_GSCALE, lse_in=good["lse"])
        assert not _fails(good, ref)[0]
        bad, ratio = _fails(R.restate_ce(x, t, R.CE_GSCALE, form, mut=mut), ref)
        print(f"mutant {mut} {form}: worst ratio {ratio:.3g}")
        assert bad
    if old:  # the workload's vocabulary, randn logits, rel_l2 < 8e-3 over the whole tensor: the mutant passes
        x, t = R.make_ce("randn", 49152)
        t = torch.tensor([5, R.IGNORE, 0, 77])  # no target inside the skipped chunk
        got, ref = R.restate_ce(x, t, 1.0, "fwd_grad", mut=mut, nt=512), R.ref_ce(x, t, 1.0)
        assert _old_ok(got, ref, R.OLD_TOL_CE)


def test_mutant_ce_vp_wrong_shard():
    V = 32
    x, t = R.make_ce("bait", V)
    splits = (0, 16, 32)
    good = R.restate_ce_vp(x, t, splits, R.CE_GSCALE)
    ref = R.ref_ce(x, t, R.CE_GSCALE, lse_in=good["lse"])
    assert not _fails(good, ref)[0]
    assert _fails(R.restate_ce_vp(x, t, splits, R.CE_GSCALE, mut="wrong_shard"), ref)[0]


@pytest.mark.parametrize("mut,dim,old", [("drop_last", 8, False), ("scale_untouched", 8, False),
                                         ("cols_2048", 2056, True)])
def test_mutant_embedding(mut, dim, old):
    n = 16
    ids, dy = R.make_ids("bait_a", n, R.EMB_V), R.make("bait", n, dim, 1)
    g0 = R.make("randn", R.EMB_V, dim, 2).float()
    ref = R.ref_embedding(g0, ids, dy, 0.5)
    assert not _fails(R.restate_embedding(g0, ids, dy, 0.5), ref)[0]
    assert _fails(R.restate_embedding(g0, ids, dy, 0.5, mut=mut), ref)[0]
    if old:  # the only embedding test had dim 256 (the workload's is 2048): the column loop never made a second trip
        dy, g0 = R.make("randn", n, 2048, 1), R.make("randn", R.EMB_V, 2048, 2).float()
        assert _old_ok(R.restate_embedding(g0, ids, dy, 0.5, mut=mut), R.ref_embedding(g0, ids, dy, 0.5), R.OLD_TOL_CE)


def test_one_wrong_vector_passes_rel_l2_and_fails_the_check():
    """The reason for the per-element check: one completely wrong 16-byte vector in a 4096 x 2048 output moves the
    whole-tensor rel_l2 by about 1e-3 (threshold 4e-3) and misses the per-element bound by orders of magnitude."""
    g, u = R.make("randn", 4096, 2048), R.make("randn", 4096, 2048, 1)
    ref = R.ref_swiglu_fwd(g, u)
    got = R.restate_swiglu_fwd(g, u)
    got["h"][4095, 2040:] = got["h"][4094, 2040:]
    assert R.rel_l2(got["h"], ref["h"][0]) < R.OLD_TOL
    r_ = R.elem_check("h", got["h"], *ref["h"], BF)
    assert not r_["ok"] and r_["index"][0] == 4095 and r_["index"][1] >= 2040 and r_["ratio"] > 10


# ------------------------------------------------------------------------------------------ every path is reached
def test_case_tables_reach_every_path(tmp_path):
    exe = compile_check(tmp_path)
    r = subprocess.run([exe, "-"], input="\n".join(R.plan_cases()) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = []
    for line in r.stdout.splitlines():
        head, *kv = line.split()
        d = dict(p.split("=") for p in kv)
        rec.append((head.split(":")[0], head, {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in d.items()}))

    def of(name):
        return [(h, d) for n, h, d in rec if n == name]

    assert {d["maxc"] for _, d in of("rms_fwd")} == {1, 2, 4, 8, 16}
    assert any(d["grid"] > 1 for _, d in of("rms_fwd"))  # and a partial last workgroup (rows 5: 4 + 1)
    bwd = of("rms_bwd")
    want = {(m, R.bwd_waves(m), f, rs) for m in (1, 2, 4, 8) for f in (0, 1) for rs in (0, 1)}
    assert {(d["maxc"], d["nw"], d["full"], d["res"]) for _, d in bwd} == want
    assert {d["nw"] for _, d in bwd} == {16, 8, 4}
    for m in (1, 2, 4, 8):  # per MAXC: waves with no row, and a ragged second pass in every workgroup
        assert any(d["maxc"] == m and d["idle_waves"] for _, d in bwd)
        assert any(d["maxc"] == m and d["trips"] == 2 and d["ragged"] and d["nb"] == 256 for _, d in bwd)
    for h, d in bwd:  # the Python restatement of the plan agrees with the header
        rows, cols = int(h.split(":")[1]), int(h.split(":")[2])
        assert (d["maxc"], d["nw"], d["nb"]) == (R.maxc_for(cols), R.bwd_waves(R.maxc_for(cols)), R.bwd_blocks(rows, cols))
    chain = of("rms_chain")
    assert {d["nw"] for _, d in chain if d["fused"]} == {16, 8, 4}
    assert any(d["cpw"] == 16 and d["fused"] for _, d in chain) and any(d["cpw"] == 17 and not d["fused"] for _, d in chain)
    assert any(d["maxc"] == 2 and d["nw"] == 16 and d["fused"] for _, d in chain)
    nchs = {2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64}
    for nt in (256, 512):
        got = {}
        for h, d in of("ce"):
            if int(h.split(":")[1]) == nt:
                got.setdefault(d["nch"], []).append(int(h.split(":")[2]))
                assert d["nch"] == R.nch_for(int(h.split(":")[2]), nt)
        assert set(got) == nchs, (nt, sorted(got))
        for n, vs in got.items():  # the first and the last vocabulary of every NCH
            lo = 8 if n == 2 else max(v for v in (2, 3, 4, 6, 8, 12, 16, 24, 32, 48) if v < n) * nt * 8 + 8
            assert min(vs) == lo and max(vs) == n * nt * 8, (nt, n, vs)
    sw = of("swiglu")
    assert {d["family"] for _, d in sw} == {"vec", "scalar"}
    assert any(d["family"] == "vec" and d["trips"] == 2 for _, d in sw)
    assert any(d["family"] == "scalar" and d["trips"] == 2 for _, d in sw)
    assert any(d["trips"] == 2 for _, d in of("rope"))
    assert all(d["trips"] == 2 and d["tail"] == 3 for _, d in of("scale"))
    assert {d["trips"] for _, d in of("emb")} == {1, 2}


# ------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def lib():
    from picotron_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from picotron_amd.build import build
        build()
    return _lib.load()


def test_misaligned_pointers_are_refused(lib):
    """Fake pointers, never dereferenced: the entry points return before any launch."""
    P = ctypes.c_void_p
    ok, odd = 4096, 4096 + 8

    def refused(rc, word):
        msg = lib.pico_last_error()
        assert rc == 1000 and b"16-byte aligned" in msg and word in msg, (rc, msg)

    for i in range(5):  # x, residual, weight, y, residual_out
        a = [P(odd if j == i else ok) for j in range(5)]
        refused(lib.pico_rmsnorm_fwd(a[0], a[1], a[2], a[3], a[4], P(ok), 4, 64, 1e-5, None), b"pico_rmsnorm_fwd")
    for i in range(5):  # dy, dresidual, x, weight, dx
        a = [P(odd if j == i else ok) for j in range(5)]
        refused(lib.pico_rmsnorm_bwd(a[0], a[1], a[2], a[3], P(ok), a[4], P(ok), P(ok), 4, 64, None), b"pico_rmsnorm_bwd")
        refused(lib.pico_rmsnorm_bwd_acc(a[0], a[1], a[2], a[3], P(ok), a[4], P(ok), 1, 1.0, P(ok), 4, 64, None),
                b"pico_rmsnorm_bwd")
        refused(lib.pico_rmsnorm_bwd_chain(a[0], a[1], a[2], a[3], P(ok), a[4], P(ok), 0, 1.0, P(ok), 4, 64, 1, None, 0,
                                           0, None, 0, 1.0, None), b"pico_rmsnorm_bwd")
    refused(lib.pico_cross_entropy_fwd(P(odd), 64, P(ok), P(ok), P(ok), 4, 64, -100, None), b"logits")
    refused(lib.pico_cross_entropy_fwd_grad(P(odd), 64, P(ok), P(ok), P(ok), P(ok), 4, 64, -100, None), b"logits")
    refused(lib.pico_cross_entropy_bwd(P(odd), 64, P(ok), P(ok), P(ok), P(ok), 64, 4, 64, -100, None), b"logits")
    refused(lib.pico_cross_entropy_bwd(P(ok), 64, P(ok), P(ok), P(ok), P(odd), 64, 4, 64, -100, None), b"dlogits")


def test_ce_bwd_shape_checks(lib):
    P = ctypes.c_void_p
    a = [P(4096)] * 5
    assert lib.pico_cross_entropy_bwd(a[0], 56, a[1], a[2], a[3], a[4], 64, 4, 64, -100, None) == 1000
    assert b"ld " in lib.pico_last_error() and b">= vocab" in lib.pico_last_error()
    assert lib.pico_cross_entropy_bwd(a[0], 64, a[1], a[2], a[3], a[4], 56, 4, 64, -100, None) == 1000
    assert b"ldd" in lib.pico_last_error()
    assert lib.pico_cross_entropy_bwd(a[0], 64, a[1], a[2], a[3], a[4], 64, 1 << 31, 64, -100, None) == 1000
    assert b"rows" in lib.pico_last_error()


def test_negative_grad_scale_is_refused(lib):
    assert lib.pico_ce_count(ctypes.c_void_p(4096), 4, -100, -0.5, ctypes.c_void_p(4096), None) == 1000
    assert b"grad_scale" in lib.pico_last_error()
    from picotron_amd import ops
    x = torch.zeros(2, 8, dtype=BF)
    with pytest.raises(ValueError, match="grad_scale"):
        ops.lm_head_cross_entropy(x, torch.zeros(8, 8, dtype=BF), torch.zeros(2, dtype=torch.long), grad_scale=-1.0)
    with pytest.raises(ValueError, match="grad_scale"):
        ops.lm_head_cross_entropy(x, torch.zeros(8, 8, dtype=BF), torch.zeros(2, dtype=torch.long),
                                  grad_scale=float("nan"))
