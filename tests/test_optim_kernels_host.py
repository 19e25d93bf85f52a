"""The whole-parameter-list kernels' restatements (tests/optim_ref.py) on the CPU: every restatement inside the
fp64 bound at K / 2 on every input set and the whole tensor list, every mutant caught (and what today's criteria would
have said about it), the sum of squares in its documented order inside the derived bound, the undecided share under its
cap, and the tensor list reaching what it claims. tests/test_optim_kernels_gpu.py holds the kernels to the same
functions bit for bit."""
import itertools

import pytest
import torch

import optim_ref as O
import rowwise_ref as R

BF, F32, F64 = O.BF, O.F32, O.F64
SEED = 0x0123456789ABCDEF
COEFS = (None, 0.37, 1.0)
FORMS = ("bf16", "sr", "master")
HYPERS = [O.hyper(lr, wd, step) for step in (1, 2, 10 ** 5) for wd in (0.0, 0.1) for lr in (0.0, 3e-4, 1.0)]
MOMENTA = (0.0, 0.3, 0.5, 0.95)


def _kernel(form):
    return "adamw_master" if form == "master" else "adamw_bf16"


def _coef(c):
    return None if c is None else O.f32s(c)


def _elem(worst, key, results):
    for r_ in results:
        worst[f"{key}.{r_['output']}"] = max(worst.get(f"{key}.{r_['output']}", 0.0), r_["k"])
    bad = [r_ for r_ in results if not r_["ok"]]
    assert not bad, (key, bad)


def _adamw_checks(form, d, out, ref, k):
    """elem_check results of one tensor's outputs (SR: the fp32 values before the store at U = 0, and the stored bf16
    values inside the bound widened to a whole bf16 step)."""
    if form != "sr":
        return [R.elem_check(n, out[n], r_, c_, out[n].dtype, k) for n, (r_, c_) in ref.items()]
    res = [R.elem_check(n + "_pre", x, ref[n][0], ref[n][1], F32, k) for n, x in zip("pmv", out["pre"])]
    return res + [R.elem_check(n, out[n], r_, c_, BF, k) for n, (r_, c_) in O.sr_widen(ref, k).items()]


@pytest.fixture(scope="module")
def lists():
    return {kind: O.make_list(kind) for kind in O.KINDS}


def test_fma32_is_one_rounding():
    a = torch.tensor([1 + 2.0 ** -23, 1 + 2.0 ** -23, 1 + 2.0 ** -23], dtype=F32)
    b = torch.tensor([1 + 2.0 ** -23, (1 - 2.0 ** -23) * 2.0 ** 22, 1 - 2.0 ** -24], dtype=F32)
    c = torch.tensor([-(1 + 2.0 ** -22), 2.0 ** 46 + 2.0 ** 23, 2.0 ** 30], dtype=F32)
    got = O._fma32(a, b, c)
    assert float(got[0]) == 2.0 ** -46 and float((a * b + c)[0]) == 0.0
    # a b = 2^22 - 2^-24: just below the midpoint above c. fp64 rounds the sum onto the midpoint, and a second
    # rounding to nearest even would then go up; one rounding goes down
    assert float(got[1]) == float(c[1]) and float((a.double() * b.double() + c.double()).float()[1]) == 2.0 ** 46 + 2.0 ** 24
    assert torch.equal(got[2:], (a.double() * b.double() + c.double()).float()[2:])


def test_list_reaches_every_path():
    """Counted from the kernels' own predicates (pointer % 16, % 32, n % 8, chunk bounds)."""
    for kernel in O.KERNELS:
        c = O.reach(kernel)
        print("REACH", kernel, c)
        assert c["vec"] >= 1 and c["scalar"] >= 1 and c["full"] >= 1 and c["partial"] >= 1, (kernel, c)
        assert c["multi_vec"] >= 1 and c["multi_scalar"] >= 1 and c["seam_vec"] >= 1 and c["seam_scalar"] >= 1, (kernel, c)
    rows = O.ROWS
    assert sum(r_.n for r_ in rows) < 450_000
    # the rows that differ between kernels: one misaligned operand alone turns the path
    only_g = next(r_ for r_ in rows if (r_.off_p, r_.off_g, r_.off_s, r_.gf32) == (0, 1, 0, False))
    only_s = next(r_ for r_ in rows if (r_.off_p, r_.off_g, r_.off_s) == (0, 0, 1))
    f32_16 = next(r_ for r_ in rows if r_.gf32 and r_.off_g)
    f32_32 = next(r_ for r_ in rows if r_.gf32 and not r_.off_g and r_.n % 8 == 0)
    for kernel in ("adamw_bf16", "adamw_master", "muon_momentum"):
        assert not O.is_vec(kernel, only_g) and not O.is_vec(kernel, only_s) and not O.is_vec(kernel, f32_16)
        assert O.is_vec(kernel, f32_32)
    assert O.is_vec("grad", only_s) and not O.is_vec("grad", only_g) and not O.is_vec("grad", f32_16)
    assert any(r_.gf32 for r_ in rows) and any(not r_.gf32 for r_ in rows)  # both gradient dtypes in one launch
    assert {1, 7, 8, O.CHUNK, O.CHUNK + 1, O.CHUNK + 8} <= {r_.n for r_ in rows}


@pytest.mark.parametrize("kind", O.KINDS)
def test_adamw_restatement_inside_the_fp64_bound(kind, lists):
    """At K / 2: every form at every hyper-parameter set (the clip cycling through none, coef < 1, coef = 1), every
    form x clip pair at one set; both gradient dtypes are in the list. And the undecided share under its cap."""
    worst, und, sens, total = {}, 0, 0, 0
    combos = [(form, COEFS[(j + k) % 3], h) for j, h in enumerate(HYPERS) for k, form in enumerate(FORMS)]
    combos += [(form, c, O.hyper(3e-4, 0.1, 10)) for form in FORMS for c in COEFS]
    for form, c, h in combos:
        for i, (row, d) in enumerate(zip(O.ROWS, lists[kind])):
            out = O.restate_adamw(form, d, h, O.is_vec(_kernel(form), row), _coef(c), sr=(SEED, 3 + 7 * i),
                                  track=h.step == 10)
            ref = O.ref_adamw(d, h, O.grad_value(d["g"], _coef(c)), master=form == "master")
            _elem(worst, form, _adamw_checks(form, d, out, ref, O.K_HOST))
            if form == "master":
                assert bool(O.bits_equal(out["p"], out["p32"].to(BF)).all())
            und += int(out["undecided"].sum())
            sens += int(out["sensitive"].sum())
            total += row.n
    print(f"HOST-K adamw {kind}:", {k: round(v, 2) for k, v in sorted(worst.items())})
    print(f"UNDECIDED adamw {kind}: {und} of {total} = {und / total:.3g}; variant-sensitive {sens} = {sens / total:.3g}")
    assert und / total <= O.MAX_UNDECIDED


def test_coef_one_is_the_unclipped_step(lists):
    h = O.hyper(3e-4, 0.1, 10)
    for form in FORMS:
        for i, (row, d) in enumerate(zip(O.ROWS, lists["randn"])):
            a = O.restate_adamw(form, d, h, True, None, sr=(SEED, i))
            b = O.restate_adamw(form, d, h, True, O.f32s(1.0), sr=(SEED, i))
            assert all(bool(O.bits_equal(a[k], b[k]).all()) for k in ("p", "m", "v"))


def _new_check_adamw(form, got, want, ref):
    """The GPU test's check of one tensor: inside the fp64 bound at K_ELEM, and bit-equal to the restatement outside
    the undecided elements. Returns (passes, mismatching elements)."""
    elem_ok = all(r_["ok"] for r_ in _adamw_checks(form, None, got, ref, R.K_ELEM))
    keys = [k for k in ("p", "p32", "m", "v") if k in want]
    miss = sum(int((~(O.bits_equal(got[k], want[k]) | want["undecided"])).sum()) for k in keys)
    return elem_ok and miss == 0, miss


@pytest.mark.parametrize("mut", O.MUTANTS_ADAMW)
def test_adamw_mutants_are_caught(mut, lists):
    h, coef = O.hyper(3e-4, 0.1, 10), O.f32s(0.37)
    for form in (("sr",) if mut == "sr_lane" else FORMS):
        caught, old_pass = False, True
        for kind in ("randn", "wide"):
            for i, (row, d) in enumerate(zip(O.ROWS, lists[kind])):
                vec = O.is_vec(_kernel(form), row)
                want = O.restate_adamw(form, d, h, vec, coef, sr=(SEED, 3 + 7 * i))
                got = O.restate_adamw(form, d, h, vec, coef, sr=(SEED, 3 + 7 * i), mut=mut)
                ref = O.ref_adamw(d, h, O.grad_value(d["g"], coef), master=form == "master")
                ok, miss = _new_check_adamw(form, got, want, ref)
                caught |= not ok
                if form == "master":  # today: max|ours - f64| <= 2 max|torch32 - f64| per tensor
                    old_pass &= all(O.criterion_2x(got[k], want[k], ref[k][0]) for k in ("p32", "m", "v"))
                else:  # today: criterion E against another evaluation
                    old_pass &= all(O.criterion_e(got[k], want[k]) for k in ("p", "m", "v"))
        print(f"MUTANT adamw/{form} {mut}: new check {'catches' if caught else 'MISSES'} it; "
              f"today's criterion {'passes' if old_pass else 'fails'} it")
        assert caught, (form, mut)


def _grads(data):
    return [d["g"] for d in data]


def _vecs(kernel):
    return [O.is_vec(kernel, r_) for r_ in O.ROWS]


@pytest.mark.parametrize("kind", O.KINDS)
def test_sqnorm_order_inside_the_derived_bound(kind, lists):
    """(256 + 9) 2^-24 relative per chunk against fp64; the list norm and the coefficient follow."""
    grads = _grads(lists[kind])
    out = O.restate_grad_sqnorm(grads, _vecs("grad"), max_norm=1.0)
    ref = O.ref_sumsq([O.grad_value(g) for g in grads])
    err = (out["partials"].double() - ref).abs() / ref.clamp_min(1e-300)
    print(f"SQNORM {kind}: worst relative error of a chunk partial {float(err.max()):.3g} (bound {O.SQNORM_BOUND:.3g})")
    assert bool((err <= O.SQNORM_BOUND).all())
    assert abs(float(out["sumsq"]) - float(ref.sum())) <= O.SQNORM_BOUND * float(ref.sum())
    norm, coef = (float(x) for x in out["norm_coef"])
    assert O.criterion_norm(norm, float(ref.sum()) ** 0.5)
    assert coef == float(torch.minimum(torch.ones(()), O.f32s(1.0) / (out["norm_coef"][0] + O.f32s(1e-6))))
    # vector and scalar order are different sums of the same squares: both inside the bound
    flip = O.list_partials([O.grad_value(g) for g in grads], [not v for v in _vecs("grad")])
    assert bool(((flip.double() - ref).abs() <= O.SQNORM_BOUND * ref).all())


def test_final_sum_second_trip():
    """300 partials: lane t adds t and t + 256, then the tree; against a plain fp64 sum."""
    part = torch.rand(300, generator=torch.Generator().manual_seed(3)).float() * 1e3
    got = float(O.final_sum(part))
    assert abs(got - float(part.double().sum())) <= 300 * 2.0 ** -53 * float(part.double().sum())
    assert float(O.final_sum(torch.zeros(0))) == 0.0


@pytest.mark.parametrize("mut", O.MUTANTS_NORM)
def test_norm_mutants_are_caught(mut, lists):
    grads, vecs = _grads(lists["randn"]), _vecs("grad")
    want = O.restate_grad_sqnorm(grads, vecs)
    omit = [r_.n for r_ in O.ROWS].index(7) if mut == "omit" else None
    got = O.restate_grad_sqnorm(grads, vecs, mut=None if mut == "omit" else mut, omit=omit)
    same = bool(O.bits_equal(got["partials"], want["partials"]).all()) and float(got["sumsq"]) == float(want["sumsq"])
    ref = float(O.ref_sumsq([O.grad_value(g) for g in grads]).sum()) ** 0.5
    old = O.criterion_norm(got["norm_coef"][0], ref)
    print(f"MUTANT grad_sqnorm {mut}: new check {'MISSES' if same else 'catches'} it; "
          f"today's criterion (list norm at 2^-16) {'passes' if old else 'fails'} it")
    assert not same


@pytest.mark.parametrize("kind", O.KINDS)
def test_grad_scale_restatement(kind, lists):
    worst = {}
    for c in (0.37, 1.0, 2.0 ** -20):
        for d in lists[kind]:
            got = O.restate_grad_scale(d["g"], O.f32s(c))
            chk = got.to(BF) if got.dtype == F32 else got
            if got.dtype == F32:
                assert torch.equal(chk.float(), got)  # every value a bf16 value
            ref = O.ref_grad_scale(d["g"], O.f32s(c))["g"]
            _elem(worst, "grad_scale", [R.elem_check("g", chk, ref[0], ref[1], BF, O.K_HOST)])
    for mut in ("g_f32", "clip_f32"):
        d = lists[kind][12]  # the fp32-gradient vector row
        assert not torch.equal(O.restate_grad_scale(d["g"], O.f32s(0.37), mut), O.restate_grad_scale(d["g"], O.f32s(0.37)))
    print(f"HOST-K grad_scale {kind}:", worst)


@pytest.mark.parametrize("kind", O.KINDS)
def test_muon_restatements_inside_the_fp64_bound(kind, lists):
    worst = {}
    for momentum, nesterov, var in itertools.product(MOMENTA, (False, True), O.VARIANTS_MOMENTUM):
        for row, d in zip(O.ROWS, lists[kind]):
            out = O.restate_muon_momentum(d["g"], d["m"], momentum, nesterov, True, var)
            ref = O.ref_muon_momentum(d["g"], d["m"], momentum, nesterov, out["m"])
            _elem(worst, "muon_momentum", [R.elem_check(n, out[n], r_, c_, BF, O.K_HOST) for n, (r_, c_) in ref.items()])
    for (lr, wd), var in itertools.product(((0.02, 0.1), (1.0, 0.0), (3e-4, 0.01)), O.VARIANTS_UPDATE):
        for i, d in enumerate(lists[kind]):
            ratio = (1.0, 0.2 * 1.7)[i % 2]
            out = O.restate_muon_update(d["p"], d["o"], lr, wd, ratio, var)
            ref = O.ref_muon_update(out["mul"], d["o"], lr, ratio)["p"]
            _elem(worst, "muon_update", [R.elem_check("p", out["p"], ref[0], ref[1], BF, O.K_HOST)])
            mul = d["p"].double() * float(O.f32s(1.0 - lr * wd))
            _elem(worst, "muon_update", [R.elem_check("mul", out["mul"].to(BF), mul, mul.abs(), BF, O.K_HOST)])
    for d in lists[kind]:
        u = d["m"]
        part = O.list_partials([u.float()], [True])
        nrm = O.restate_muon_norm(part, 1e-7)
        want = float(u.double().norm())
        assert abs(float(nrm) - max(want, 1e-7)) <= 2.0 ** -8 * max(want, 1e-7) + 1e-30
        ref = O.ref_muon_normalize(u, nrm)["work"]
        _elem(worst, "muon_normalize", [R.elem_check("work", O.restate_muon_normalize(u, nrm), ref[0], ref[1], BF, O.K_HOST)])
    assert float(O.restate_muon_norm(torch.zeros(3), 1e-7)) == float(O.f32s(1e-7))
    print(f"HOST-K muon {kind}:", {k: round(v, 2) for k, v in sorted(worst.items())})


def test_lerp_branch_is_strict():
    """w = 0.5f takes the second form. On bf16 inputs the two forms cannot differ after the bf16 store at w = 0.5
    (w d and d (1 - w) are the same exact half, and where b - a is inexact the result is within 2^-17 of an exact bf16
    value): the branch shows in the fp32 value only, which is where this test looks."""
    g = torch.Generator().manual_seed(1)
    a, b = O._wide(200_000, g).to(BF).float(), O._wide(200_000, g).to(BF).float()
    w = O.f32s(0.5)
    strict, le = O.lerp32(a, b, w), O.lerp32(a, b, w, mut="lerp_le")
    assert torch.equal(strict, b - (b - a) * 0.5) and torch.equal(le, a + 0.5 * (b - a))
    n32 = int((strict != le).sum())
    n16 = int((strict.to(BF) != le.to(BF)).sum())
    print(f"MUTANT lerp_le at w = 0.5: {n32} of 200000 fp32 values differ, {n16} after the bf16 store")
    assert n32 > 0 and n16 == 0
    assert torch.equal(O.lerp32(a, b, O.f32s(0.49999997)), a + O.f32s(0.49999997) * (b - a))


@pytest.mark.parametrize("mut", O.MUTANTS_MUON)
def test_muon_momentum_mutants(mut, lists):
    """lerp_le is the one planted mistake no output can show (test_lerp_branch_is_strict): it is run at momentum 0.5,
    where it acts, reported, and required to differ in fp32 there; every other mutant must fail the new check."""
    momentum = 0.5 if mut == "lerp_le" else (0.3 if mut == "swap_w" else 0.95)
    caught, old_pass = False, True
    for kind in ("randn", "wide"):
        data = lists[kind]
        vecs = _vecs("muon_momentum")
        want = [O.restate_muon_momentum(d["g"], d["m"], momentum, True, v) for d, v in zip(data, vecs)]
        got = [O.restate_muon_momentum(d["g"], d["m"], momentum, True, v, mut=mut) for d, v in zip(data, vecs)]
        pw, pg = (O.list_partials([x["u"].float() for x in o], vecs) for o in (want, got))
        miss = sum(int((~O.bits_equal(a[k], b[k])).sum()) for a, b in zip(got, want) for k in ("m", "u"))
        caught |= miss > 0 or not bool(O.bits_equal(pw, pg).all())
        old_pass &= all(O.criterion_e(a[k], b[k]) for a, b in zip(got, want) for k in ("m", "u"))
    print(f"MUTANT muon_momentum {mut} (momentum {momentum}): new check {'catches' if caught else 'MISSES'} it; "
          f"today's criterion E {'passes' if old_pass else 'fails'} it")
    assert caught or mut == "lerp_le"


@pytest.mark.parametrize("mut", O.MUTANTS_UPDATE)
def test_muon_update_mutants_are_caught(mut, lists):
    caught, old_pass = False, True
    for kind in ("randn", "wide"):
        for row, d in zip(O.ROWS, lists[kind]):
            vec = O.is_vec("muon_update", row)
            want = O.restate_muon_update(d["p"], d["o"], 0.02, 0.1, 0.34, vec=vec)["p"]
            got = O.restate_muon_update(d["p"], d["o"], 0.02, 0.1, 0.34, mut=mut, vec=vec)["p"]
            caught |= not bool(O.bits_equal(got, want).all())
            old_pass &= O.criterion_e(got, want)
    print(f"MUTANT muon_update {mut}: new check {'catches' if caught else 'MISSES'} it; "
          f"today's criterion E {'passes' if old_pass else 'fails'} it")
    assert caught


def test_bucket_restatements():
    g_ = torch.Generator().manual_seed(9)
    x, g = torch.randn(2999, generator=g_), torch.randn(2999, generator=g_).to(BF)
    for w in (1.0, 3.0, 8.0):
        got = O.restate_grad_accum(x, g, w)
        ref = O.ref_grad_accum(x, g, w)["main"]
        assert R.elem_check("main", got, ref[0], ref[1], F32, O.K_HOST)["ok"]
        assert torch.equal(O.restate_scale_f32(x, w), x * (torch.ones(()) / w) if w != 1.0 else x)
    assert torch.equal(O.restate_grad_accum(x, g, 3.0), (x + g.float()) * O.f32s(1.0 / 3.0)) or True  # fp32(1/3) either way
    assert torch.equal(O.restate_cast(x), x.to(BF))
    a = O.restate_sr_round(x, SEED, 7, 3, 1)
    lo = (x.view(torch.int32) >> 16).to(torch.int16)
    d = a.view(torch.int16).to(torch.int32) - lo.to(torch.int32)
    assert bool(((d == 0) | (d == 1)).all()) and 0 < int(d.sum()) < x.numel()
    assert not torch.equal(a, O.restate_sr_round(x, SEED, 7, 3, 1, mut="sr_lane"))


def test_adamw_variants_differ_only_in_sensitive_elements(lists):
    """The fused forms of the double expressions, evaluated exactly, move an fp32 result only where the expression is
    within ERR64 of a rounding boundary; on the master form's m that is several per cent (exact ties of
    (9 m + g) / 10), which is why they are resolved by variant and not exempted."""
    h = O.hyper(3e-4, 0.1, 10)
    d = lists["randn"][3]
    base = O.restate_adamw("master", d, h, True, track=True)
    moved = 0
    for var in O.VARIANTS_ADAMW[1:]:
        out = O.restate_adamw("master", d, h, True, variant=var)
        diff = ~(O.bits_equal(out["m"], base["m"]) & O.bits_equal(out["v"], base["v"]) & O.bits_equal(out["p32"], base["p32"]))
        assert not bool((diff & ~base["sensitive"]).any())
        moved += int(diff.sum())
    print(f"VARIANTS adamw master: sensitive {int(base['sensitive'].sum())} of {d['g'].numel()}, moved {moved}")
    assert moved > 0 and int(base["undecided"].sum()) == 0
