"""The whole-parameter-list kernels (adamw.hip, grad_clip.hip, muon.hip, dp_bucket.hip) against tests/optim_ref.py:
every element inside the fp64 bound (rowwise_ref.elem_check at K_ELEM), bit-equal to the CPU restatement under one
contraction variant per launch (vector and scalar tensors alike), NaN guard bands around every buffer and table, unread
columns pointed at guard-only NaN buffers, and the tensor list of optim_ref.ROWS that reaches every path. The device
tables are built by hand from include/picotron_hip.h; nothing here goes through picotron_amd.optim."""
import itertools

import pytest
import torch

import optim_ref as O
import rowwise_ref as R

pytestmark = pytest.mark.gpu
BF, F32, F64 = O.BF, O.F32, O.F64
SEED = 0xFEDCBA9876543210
WORST = {}
_LAST = {}


@pytest.fixture(scope="module")
def lists():
    return {kind: O.make_list(kind) for kind in O.KINDS}


def _ids():
    return [3 + 7 * i for i in range(len(O.ROWS))]


def _kernel(form):
    return "adamw_master" if form == "master" else "adamw_bf16"


def _check_paths(kernel, ptrs):
    """The launch's real addresses choose the paths the host test counted."""
    for r_, a in zip(O.ROWS, ptrs):
        assert O.is_vec(kernel, r_, a) == O.is_vec(kernel, r_), (kernel, r_)


def _adamw_case(form, data, h, coef, clip_entry=False):
    """One guarded launch, checked against fp64 and the restatement. Returns the launch's outputs."""
    nc = None if coef is None else torch.stack([torch.tensor(2.5), O.f32s(coef)])
    got = O.launch_adamw(form, O.ROWS, data, h, nc, SEED, _ids(), clip_entry)
    _check_paths(_kernel(form), got["ptrs"])
    keys = [k for k in ("p", "p32", "m", "v") if k in got]
    c = None if coef is None else O.f32s(coef)
    per = [{k: got[k][i] for k in keys} for i in range(len(O.ROWS))]
    for i, (r_, d) in enumerate(zip(O.ROWS, data)):
        ref = O.ref_adamw(d, h, O.grad_value(d["g"], c), master=form == "master")
        ref = O.sr_widen(ref, R.K_ELEM) if form == "sr" else ref
        R.check_all(f"adamw_{form} row{i}", per[i], ref, worst_k=WORST)
        if form == "master":
            assert bool(O.bits_equal(per[i]["p"], per[i]["p32"].to(BF)).all()), i

    def restate(i, var):
        out = O.restate_adamw(form, data[i], h, O.is_vec(_kernel(form), O.ROWS[i]), c, sr=(SEED, _ids()[i]), variant=var)
        assert int(out["undecided"].sum()) <= O.MAX_UNDECIDED * O.ROWS[i].n
        return {k: out[k] for k in keys + ["undecided"]}

    key = (form, coef is not None)

    def holds(var, only=None):
        """Every element of the launch (of output `only`) bit-equal to the restatement under var."""
        got_ = per if only is None else [{only: x[only]} for x in per]
        return bool(O.matching_variants(got_, lambda i, v: {k: x for k, x in restate(i, v).items()
                                                             if only is None or k in (only, "undecided")}, [var])[0])

    ok = [_LAST[key]] if key in _LAST and holds(_LAST[key]) else []
    if not ok:  # m and v each depend on their own site alone; the parameter on all three
        vm = [b for b in (0, 1, 2) if holds((0, b, 0), "m")]
        vv = [c_ for c_ in (0, 1, 2) if holds((0, 0, c_), "v")]
        ok = [(a, b, c_) for b in vm for c_ in vv for a in (0, 1) if holds((a, b, c_))][:1]
        print(f"VARIANT-SEARCH adamw_{form}: m sites {vm}, v sites {vv}")
    print(f"VARIANT adamw_{form}{'_clip' if coef is not None else ''} (decay, m, v) = {ok}")
    assert ok, f"adamw_{form}: no single variant restates every element of the launch"
    _LAST[key] = ok[0]
    return got


CASES = [("bf16", None, False), ("bf16", 0.37, True), ("master", None, False), ("master", 0.37, False),
         ("sr", None, False), ("sr", 0.37, False)]


@pytest.mark.parametrize("form,coef,clip_entry", CASES)
@pytest.mark.parametrize("kind", ("randn", "wide"))
def test_adamw(form, coef, clip_entry, kind, lists):
    for step in (1, 1000):
        _adamw_case(form, lists[kind], O.hyper(3e-4, 0.1, step), coef, clip_entry)


@pytest.mark.parametrize("form,clip_entry", [("bf16", True), ("master", False), ("sr", False)])
def test_adamw_clip_edges(form, clip_entry, lists):
    """A non-finite norm leaves every buffer bit-identical; coef = 1 gives the bits of the unclipped entry point."""
    data, h = lists["randn"], O.hyper(3e-4, 0.1, 7)
    keys = ("p", "m", "v") + (("p32",) if form == "master" else ())
    src = {"p": "p", "m": "m32" if form == "master" else "m", "v": "v32" if form == "master" else "v", "p32": "p32"}
    for norm in (float("inf"), float("-inf"), float("nan")):
        got = O.launch_adamw(form, O.ROWS, data, h, torch.tensor([norm, 0.5]), SEED, _ids(), clip_entry)
        for k in keys:
            for i, d in enumerate(data):
                assert bool(O.bits_equal(got[k][i], d[src[k]]).all()), (k, i)
    plain = O.launch_adamw(form, O.ROWS, data, h, None, SEED, _ids(), False)
    one = O.launch_adamw(form, O.ROWS, data, h, torch.tensor([0.5, 1.0]), SEED, _ids(), clip_entry)
    for k in keys:
        for a, b in zip(plain[k], one[k]):
            assert bool(O.bits_equal(a, b).all()), k


def _grad_vecs():
    return [O.is_vec("grad", r_) for r_ in O.ROWS]


@pytest.mark.parametrize("kind", O.KINDS)
def test_grad_norm_and_scale(kind, lists):
    grads = [d["g"] for d in lists[kind]]
    want = O.restate_grad_sqnorm(grads, _grad_vecs(), max_norm=1.0)
    got = O.launch_grad_norm(O.ROWS, grads, 1.0, scale_with="own")
    for r_, a in zip(O.ROWS, got["ptrs"]):
        assert O.is_vec("grad", r_, a) == O.is_vec("grad", r_)
    ref = O.ref_sumsq([O.grad_value(g) for g in grads])
    err = (got["partials"].double() - ref).abs() / ref.clamp_min(1e-300)
    print(f"SQNORM {kind}: worst relative error of a chunk partial {float(err.max()):.3g} (bound {O.SQNORM_BOUND:.3g})")
    assert bool((err <= O.SQNORM_BOUND).all())
    assert bool(O.bits_equal(got["partials"], want["partials"]).all())
    assert bool(O.bits_equal(got["sumsq"].reshape(1), want["sumsq"].reshape(1)).all())
    assert bool(O.bits_equal(got["norm_coef"], want["norm_coef"]).all())
    coef = want["norm_coef"][1]
    assert float(coef) < 1.0
    for i, g in enumerate(grads):
        assert bool(O.bits_equal(got["g"][i], O.restate_grad_scale(g, coef)).all()), i
        chk = got["g"][i].to(BF)
        rf = O.ref_grad_scale(g, coef)["g"]
        R.report(f"grad_scale row{i}", [R.elem_check("g", chk, rf[0], rf[1], BF)], WORST)


def test_grad_scale_writes_nothing_at_one_or_nonfinite(lists):
    grads = [d["g"] for d in lists["randn"]]
    for nc in ([0.5, 1.0], [float("inf"), 0.5], [float("-inf"), 0.5]):
        got = O.launch_grad_norm(O.ROWS, grads, 1.0, scale_with=torch.tensor(nc))
        for a, b in zip(got["g"], grads):
            assert bool(O.bits_equal(a, b).all()), nc


def test_sqnorm_final_second_trip():
    """300 chunks from 300 tensors of 8 .. 64 elements: the final kernel's lanes 0 .. 43 add two partials."""
    g_ = torch.Generator().manual_seed(11)
    rows = [O.Row(8 + (i * 5) % 57, False, 0, 0, 0, "") for i in range(300)]
    grads = [(torch.randn(r_.n, generator=g_) * 3).to(BF) for r_ in rows]
    vecs = [O.is_vec("grad", r_) for r_ in rows]
    assert any(vecs) and not all(vecs)
    want = O.restate_grad_sqnorm(grads, vecs, max_norm=0.25)
    got = O.launch_grad_norm(rows, grads, 0.25)
    assert got["partials"].numel() == 300
    assert bool(O.bits_equal(got["partials"], want["partials"]).all())
    assert bool(O.bits_equal(got["sumsq"].reshape(1), want["sumsq"].reshape(1)).all())
    assert bool(O.bits_equal(got["norm_coef"], want["norm_coef"]).all())


@pytest.mark.parametrize("momentum", (0.0, 0.3, 0.5, 0.95))
@pytest.mark.parametrize("nesterov", (False, True))
def test_muon_momentum(momentum, nesterov):
    kind = "wide" if momentum in (0.3, 0.5) else "randn"
    data = O.make_muon_list(kind, momentum, nesterov)
    got = O.launch_muon_momentum(O.ROWS, data, momentum, nesterov)
    _check_paths("muon_momentum", got["ptrs"])
    vecs = [O.is_vec("muon_momentum", r_) for r_ in O.ROWS]
    per = [{"m": got["m"][i], "u": got["u"][i]} for i in range(len(O.ROWS))]
    for i, d in enumerate(data):
        R.check_all(f"muon_momentum row{i}", per[i], O.ref_muon_momentum(d["g"], d["m"], momentum, nesterov, per[i]["m"]),
                    worst_k=WORST)
    ok, member = O.matching_variants(
        per, lambda i, var: O.restate_muon_momentum(data[i]["g"], data[i]["m"], momentum, nesterov, vecs[i], var),
        O.VARIANTS_MOMENTUM)
    print(f"VARIANT muon_momentum momentum {momentum} nesterov {nesterov}: (a + w d, b - d (1 - w)) contracted = {ok}; "
          f"every element in the candidate set: {member}")
    assert ok, "no single variant restates every element: the vector and scalar loops were compiled differently"
    # the partials: the sum of squares of the bf16 u the kernel stored, in pico_grad_sqnorm's order
    want = O.list_partials([u.float() for u in got["u"]], vecs)
    assert bool(O.bits_equal(got["partials"], want).all())
    ref = O.ref_sumsq([u.float() for u in got["u"]])
    assert bool(((got["partials"].double() - ref).abs() <= O.SQNORM_BOUND * ref).all())


def test_muon_normalize(lists):
    data = lists["randn"]
    work = [d["m"] for d in data]
    work[3] = torch.zeros_like(work[3])  # an all-zero u: norm = eps, finite zeros out
    vecs = [O.is_vec("muon_normalize", r_) for r_ in O.ROWS]
    part = O.list_partials([w.float() for w in work], vecs)
    got = O.launch_muon_normalize(O.ROWS, work, part, 1e-7)
    ch = O.chunks_of([r_.n for r_ in O.ROWS])
    for i, w in enumerate(work):
        nrm = O.restate_muon_norm(part[torch.tensor([ti == i for ti, _ in ch])], 1e-7)
        assert bool(O.bits_equal(got["norms"][i].reshape(1), nrm.reshape(1)).all()), i
        assert bool(O.bits_equal(got["work"][i], O.restate_muon_normalize(w, nrm)).all()), i
        rf = O.ref_muon_normalize(w, nrm)["work"]
        R.report(f"muon_normalize row{i}", [R.elem_check("work", got["work"][i], rf[0], rf[1], BF)], WORST)
    assert float(got["norms"][3]) == float(O.f32s(1e-7)) and not bool(got["work"][3].float().abs().sum())


def test_muon_norm_second_trip():
    """chunk_start feeds only the norm kernel: 300 hand-made partials for a one-chunk tensor reach its second
    256-partial trip."""
    part = (torch.rand(300, generator=torch.Generator().manual_seed(4)) * 7).float()
    rows = [O.Row(2056, False, 0, 0, 0, "")]
    w = O.make_row("randn", rows[0])["m"]
    got = O.launch_muon_normalize(rows, [w], part, 1e-7, chunk_start=[0, 300])
    nrm = O.restate_muon_norm(part, 1e-7)
    assert bool(O.bits_equal(got["norms"], nrm.reshape(1)).all())
    assert bool(O.bits_equal(got["work"][0], O.restate_muon_normalize(w, nrm)).all())


@pytest.mark.parametrize("lr,wd", [(0.02, 0.1), (1.0, 0.0), (3e-4, 0.01)])
def test_muon_update(lr, wd, lists):
    data = lists["randn" if lr != 1.0 else "wide"]
    ratios = [(1.0, 0.2 * 1.7)[i % 2] for i in range(len(O.ROWS))]
    got = O.launch_muon_update(O.ROWS, data, lr, wd, ratios)
    for r_, a in zip(O.ROWS, got["ptrs"]):
        assert O.is_vec("muon_update", r_, dict(a, s=0)) == O.is_vec("muon_update", r_)
    vecs = [O.is_vec("muon_update", r_) for r_ in O.ROWS]
    per = [{"p": p} for p in got["p"]]
    for i, d in enumerate(data):
        mul = O.restate_muon_update(d["p"], d["o"], lr, wd, ratios[i])["mul"]
        R.check_all(f"muon_update row{i}", per[i], O.ref_muon_update(mul, d["o"], lr, ratios[i]), worst_k=WORST)
    ok, member = O.matching_variants(
        per, lambda i, var: {"p": O.restate_muon_update(data[i]["p"], data[i]["o"], lr, wd, ratios[i], var, vec=vecs[i])["p"]},
        O.VARIANTS_UPDATE)
    print(f"VARIANT muon_update lr {lr} wd {wd}: pf + alpha o contracted = {ok}; every element in the candidate set: {member}")
    assert ok, "no single variant restates every element: the vector and scalar loops were compiled differently"


NS = (1, 3, 4, 5, 7, 8, 2056, 2999, 3000)


@pytest.mark.parametrize("divide_by", (1.0, 3.0, 8.0))
def test_grad_accum(divide_by):
    g_ = torch.Generator().manual_seed(21)
    for n, shift in itertools.product(NS, (0, 1)):
        x, g = torch.randn(n, generator=g_) * 4, torch.randn(n, generator=g_).to(BF)
        got = O.launch_bucket("accum", x, g, divide_by, shift=shift)
        assert bool(O.bits_equal(got, O.restate_grad_accum(x, g, divide_by)).all()), (n, shift)
        rf = O.ref_grad_accum(x, g, divide_by)["main"]
        assert R.elem_check("main", got, rf[0], rf[1], F32)["ok"]


def test_scale_and_cast():
    g_ = torch.Generator().manual_seed(22)
    for n in (1, 3, 4, 5, 2056):
        x = torch.randn(n, generator=g_) * 4
        for w in (3.0, 8.0, 1.0):
            assert bool(O.bits_equal(O.launch_bucket("scale", x, divide_by=w), O.restate_scale_f32(x, w)).all()), (n, w)
    for n, shift in itertools.product(NS, (0, 1)):
        x = O._wide(n, g_)
        assert bool(O.bits_equal(O.launch_bucket("cast", x, shift=shift), O.restate_cast(x)).all()), (n, shift)


def test_sr_round():
    """Aligned with n % 8 in {0, 5} (vector body and scalar tail in one launch), n = 3, and unaligned."""
    g_ = torch.Generator().manual_seed(23)
    for (n, shift), q in zip(((2056, 0), (2061, 0), (3, 0), (2056, 1), (2061, 1)), (0, 1, 2, 1, 0)):
        x = O._wide(n, g_)
        got = O.launch_bucket("sr_round", x, shift=shift, sr=(SEED, 9, 5, q))
        assert bool(O.bits_equal(got, O.restate_sr_round(x, SEED, 9, 5, q)).all()), (n, shift)


def _edges(t, n):
    """The first, the last and the seam-adjacent 4096 elements (the seam: where the grid-stride loop wraps)."""
    seam = n - (n % 2048 or 8) if n % 8 == 0 else n - 1
    idx = torch.cat([torch.arange(0, 4096), torch.arange(seam - 2048, min(n, seam + 2048)), torch.arange(n - 4096, n)])
    return t[idx.to(t.device)].cpu()


@pytest.mark.parametrize("n", (4096 * 256 * 8 + 8, 4096 * 256 + 1))
def test_bucket_grid_stride_second_trip(n):
    """The smallest n at which a lane of the vector (4096 * 256 * 8 + 8) and of the scalar (4096 * 256 + 1) kernels
    takes a second grid-stride trip; compared on the device, the edges also on the CPU."""
    g_ = torch.Generator(device="cuda").manual_seed(31)
    x = torch.randn(n, device="cuda", generator=g_) * 4
    g = torch.randn(n, device="cuda", generator=g_).to(BF)
    inv = (torch.ones((), dtype=F32) / O.f32s(3.0)).cuda()
    got = O.launch_bucket("accum", x, g, 3.0, keep_device=True)
    want = (x + g.float()) * inv
    assert bool(O.bits_equal(got, want).all())
    assert bool(O.bits_equal(_edges(got, n), O.restate_grad_accum(_edges(x, n), _edges(g, n), 3.0)).all())
    got = O.launch_bucket("cast", x, keep_device=True)
    assert bool(O.bits_equal(got, x.to(BF)).all())
    assert bool(O.bits_equal(_edges(got, n), O.restate_cast(_edges(x, n))).all())


def test_zz_report_worst_k():
    """Last in the file: the smallest K that passed, per kernel and output (DESIGN.md records them)."""
    for k, v in sorted(WORST.items()):
        print(f"GPU-K {k}: {v:.2f}")
        assert v <= R.K_ELEM
