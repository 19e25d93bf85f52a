"""Every dispatch path of the row-wise and elementwise kernels (rmsnorm.hip, rope.hip, swiglu.hip, cross_entropy.hip,
embedding.hip) on the GPU under the per-element bound and the guard bands of tests/rowwise_ref.py.

Each case launches through the C ABI on guarded buffers (NaN around every tensor, NaN-filled outputs, guarded
workspaces), checks that the guards are bit-identical afterwards, every output element was written and no input was,
and holds every element of every output to
    |got - ref| <= U |ref| + 8 2^-23 cond + 2^-120
against an fp64 reference computed in plain torch on the GPU (U = 2^-8 for bf16 outputs, 0 for fp32). One line per
output is printed (worst ratio, the K it would need, where), and the worst K per operation and output at the end of
the module. Which instantiation and loop trip a case reaches is asserted on the CPU by
tests/test_rowwise_host.py::test_case_tables_reach_every_path. At import this file only defines its tables."""
import pytest
import torch

import rowwise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
BF, F32 = R.BF, R.F32
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _print_worst_k():
    yield
    for key, k in sorted(WORST.items()):
        print(f"WORSTK {key} {k:.2f}")


def _mk(kind, rows, cols, seed=0):
    return R.make(kind, rows, cols, seed, DEV)


def _check(tag, got, ref, k=R.K_ELEM):
    R.check_all(tag, got, ref, k, WORST)


# ------------------------------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("cols", R.RMS_FWD_COLS)
def test_rmsnorm_fwd(cols):
    for rows in R.RMS_FWD_ROWS:
        for kind in R.KINDS:
            x, res, w = _mk(kind, rows, cols), _mk(kind, rows, cols, 1), _mk("randn", 1, cols, 2)[0]
            for rr, want in ((None, False), (res, True), (res, False)):
                got = R.launch_rmsnorm_fwd(x, w, EPS, rr, want_res_out=want)
                ref = R.ref_rmsnorm_fwd(x, w, EPS, rr)
                if not want:
                    ref.pop("residual_out", None)
                _check(f"rms_fwd {rows}x{cols} {kind} res{rr is not None} out{want}", got, ref)
                if want:  # the rounded residual stream is exact: one bf16 rounding of an exact fp32 sum
                    assert torch.equal(got["residual_out"], (x.float() + res.float()).to(BF))


@pytest.mark.parametrize("rows,cols", R.RMS_FWD_T)
def test_rmsnorm_fwd_t(rows, cols):
    for kind in R.KINDS:
        x, res, w = _mk(kind, rows, cols), _mk(kind, rows, cols, 1), _mk("randn", 1, cols, 2)[0]
        for rr in (None, res):
            got = R.launch_rmsnorm_fwd(x, w, EPS, rr, transposed=True)
            _check(f"rms_fwd_t {rows}x{cols} {kind} res{rr is not None}", got, R.ref_rmsnorm_fwd(x, w, EPS, rr))
            assert torch.equal(got["y_t"], got["y"].t()), "y_t != y^T"
            plain = R.launch_rmsnorm_fwd(x, w, EPS, rr)
            assert torch.equal(plain["y"], got["y"]) and torch.equal(plain["rstd"], got["rstd"])


def _bwd_inputs(kind, rows, cols):
    x, dy, dres = _mk(kind, rows, cols), _mk(kind, rows, cols, 1), _mk(kind, rows, cols, 3)
    w = _mk("randn", 1, cols, 2)[0]
    rstd = torch.rsqrt(x.double().pow(2).mean(-1) + EPS).float()  # an input of the backward
    return x, dy, dres, w, rstd, _mk("randn", 1, cols, 4)[0]


@pytest.mark.parametrize("cols", R.RMS_BWD_COLS)
def test_rmsnorm_bwd(cols):
    for rows in R.rms_bwd_rows(cols):
        for kind in R.KINDS:
            x, dy, dres, w, rstd, g0 = _bwd_inputs(kind, rows, cols)
            for dr in (None, dres):
                for mode, g in ((0, None), (1, g0), (2, g0.float())):
                    got = R.launch_rmsnorm_bwd(dy, x, w, rstd, dr, mode, g, 0.25)
                    _check(f"rms_bwd {rows}x{cols} {kind} dres{dr is not None} mode{mode}", got,
                           R.ref_rmsnorm_bwd(dy, x, w, rstd, dr, mode, g, 0.25))


@pytest.mark.parametrize("rows,cols,pc", R.RMS_CHAIN)
def test_rmsnorm_chained_dw(rows, cols, pc):
    """The previous call's partial rows (synthetic here) reduced inside this launch: under the bound against the fp64
    sum, bit for bit against pico_rmsnorm_dw_reduce where the summation order is the same (one partial row; the
    cpw > 16 fallback, which is that launch), and this launch's own outputs unchanged by the chaining."""
    nb_own = R.bwd_blocks(rows, cols)
    fused = (pc + nb_own - 1) // nb_own <= 16
    pg0 = _mk("randn", 1, pc, 4)[0]
    for kind in R.KINDS:  # the launch's own inputs and the previous call's partial rows from the same set
        x, dy, _, w, rstd, g0 = _bwd_inputs(kind, rows, cols)
        base = R.launch_rmsnorm_bwd(dy, x, w, rstd)
        _check(f"rms_chain own {rows}x{cols} {kind}", base, R.ref_rmsnorm_bwd(dy, x, w, rstd))
        for nb in R.CHAIN_NB:
            part = _mk(kind, nb, pc, 5).float() * 1.37
            for pm, pg in ((0, None), (1, pg0), (2, pg0.float())):
                prev = {"part": part, "mode": pm, "g0": pg, "scale": 0.25}
                sep = R.launch_dw_reduce(part, pm, pg, 0.25)
                for own in (1, 0):
                    got = R.launch_rmsnorm_bwd(dy, x, w, rstd, reduce_own=own, prev=prev)
                    tag = f"rms_chain {rows}x{cols} prev {nb}x{pc} {kind} mode{pm} own{own}"
                    _check(tag, {"dw": got["prev_dw"]}, R.ref_dw_reduce(part, pm, pg, 0.25))
                    if nb == 1 or not fused:
                        assert torch.equal(got["prev_dw"], sep), tag
                    assert torch.equal(got["dx"], base["dx"]) and torch.equal(got["part"], base["part"]), tag
                    if own:
                        assert torch.equal(got["dw"], base["dw"]), tag
                    else:  # the partial rows left for a later reduction give the same dw
                        assert torch.equal(R.launch_dw_reduce(got["part"]), base["dw"]), tag


# ------------------------------------------------------------------------------------------ RoPE
def _rope_inputs(kind, B, S, Hh, D):
    x = _mk(kind, B * S * Hh, D).view(B, S, Hh, D)
    cos, sin = R.A.rope_tables(S, D, DEV, base=10000.0)
    return x, cos, sin


@pytest.mark.parametrize("D", R.ROPE_D)
def test_rope(D):
    for Hh in R.ROPE_H:
        for S in R.ROPE_S:
            for B in R.ROPE_B:
                for kind in R.KINDS:
                    x, cos, sin = _rope_inputs(kind, B, S, Hh, D)
                    for conj in (False, True):
                        tag = f"rope D{D} H{Hh} S{S} B{B} {kind} conj{conj}"
                        got = R.launch_rope(x, cos, sin, conj)
                        assert torch.equal(got["out"], R.restate_rope(x, cos, sin, conj)["out"]), tag
                        _check(tag, got, R.ref_rope(x, cos, sin, conj), 0.0)
                        alias = R.launch_rope(x, cos, sin, conj, alias=True)  # out == x, both strided
                        assert torch.equal(alias["out"], got["out"]), tag + " aliased"


def test_rope_second_loop_trip():
    """More than 8192 x 256 vectors: bit for bit against the fp32 restatement on the device, and the last batch's last
    8 positions under U against fp64."""
    B, S, Hh, D = R.ROPE_BIG
    x, cos, sin = _rope_inputs("randn", B, S, Hh, D)
    got = R.launch_rope(x, cos, sin, False)
    assert torch.equal(got["out"], R.restate_rope(x, cos, sin)["out"])
    ref = R.ref_rope(x[B - 1:, S - 8:], cos[S - 8:], sin[S - 8:])
    _check("rope big slice", {"out": got["out"][B - 1:, S - 8:]}, ref, 0.0)


# ------------------------------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("rows,cols,fused,shift", R.SWIGLU_CASES + list(R.SWIGLU_BIG))
def test_swiglu(rows, cols, fused, shift):
    for kind in R.KINDS:
        g, u, dh = _mk(kind, rows, cols), _mk(kind, rows, cols, 1), _mk(kind, rows, cols, 2)
        tag = f"{rows}x{cols} fused{fused} shift{shift} {kind}"
        _check("swiglu_fwd " + tag, R.launch_swiglu(g, u, None, fused, shift), R.ref_swiglu_fwd(g, u))
        _check("swiglu_bwd " + tag, R.launch_swiglu(g, u, dh, fused, shift), R.ref_swiglu_bwd(dh, g, u))


@pytest.mark.parametrize("rows,cols", R.SWIGLU_T)
def test_swiglu_fwd_t(rows, cols):
    for kind in R.KINDS:
        g, u = _mk(kind, rows, cols), _mk(kind, rows, cols, 1)
        got = R.launch_swiglu_t(g, u)
        _check(f"swiglu_fwd_t {rows}x{cols} {kind}", {"h": got["h"]}, R.ref_swiglu_fwd(g, u))
        assert torch.equal(got["h_t"], got["h"].t()), "h_t != h^T"


# ------------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("V", sorted(set(R.CE_VOCABS_256 + R.CE_VOCABS_512)))
def test_cross_entropy(V):
    for kind in R.KINDS:
        x, t = R.make_ce(kind, V, device=DEV)
        valid = R._valid(t, V)
        if V in R.CE_VOCABS_512:  # the fused forward + gradient, in place, 512 threads per row
            got = R.launch_ce_fwd_grad(x, t, R.CE_GSCALE)
            _check(f"ce_fwd_grad V{V} {kind}", got, R.ref_ce(x, t, R.CE_GSCALE))
            d = got["dlogits"].float()
            hot = torch.zeros_like(d, dtype=torch.bool)
            hot[torch.arange(len(t), device=DEV)[valid], t[valid]] = True
            # the target column's fix-up touched nothing else: every other element is a softmax term (>= 0), an ignored
            # row is zero; the target's own element is the kernel's formula recomputed from the kernel's own lse, to
            # within one bf16 ulp of the result plus 4 fp32 ulps of g (the hardware exp2 / log2 are 1-ulp functions
            # and not torch's; their error comes before the subtraction of g and does not shrink with the result)
            assert bool((d[~hot] >= 0).all()) and bool((d[~valid] == 0).all())
            r, want = R.fwd_grad_target(x, t, got["lse"], R.CE_GSCALE)
            have = got["dlogits"][r, t[valid]]
            mag = torch.maximum(want.float().abs(), have.float().abs()).clamp_min(2.0 ** -126)
            tol = torch.exp2(torch.floor(torch.log2(mag)) - 7) + 4 * 2.0 ** -24 * R.CE_GSCALE
            off = (have.float() - want.float()).abs()
            print(f"FIXUP V{V} {kind}: worst {float((off / tol).max()):.2f} of the tolerance")
            assert bool((off <= tol).all()), (V, kind, have, want)
        if V in R.CE_VOCABS_256:
            fwd = R.launch_ce_fwd(x, t)
            ref = R.ref_ce(x, t, R.CE_GSCALE, lse_in=fwd["lse"])  # dlogits from the lse the backward is given
            _check(f"ce_fwd V{V} {kind}", fwd, {n: ref[n] for n in ("lse", "loss")})
            bwd = R.launch_ce_bwd(x, t, fwd["lse"], R.CE_GSCALE)
            _check(f"ce_bwd V{V} {kind}", bwd, {"dlogits": ref["dlogits"]})
            for splits in ((0, V), (0, max(8, V // 16 * 8), V)):
                if len(set(splits)) != len(splits):
                    continue
                outs = [R.launch_ce_vp(x, t, splits, R.CE_GSCALE, inplace) for inplace in (False, True)]
                ref = R.ref_ce(x, t, R.CE_GSCALE, lse_in=outs[0]["lse"])
                _check(f"ce_vp V{V} tp{len(splits) - 1} {kind}", outs[0], ref)
                for n in ("lse", "loss", "dlogits"):
                    assert torch.equal(outs[0][n], outs[1][n]), f"ce_vp V{V} {kind}: {n} in place != out of place"


@pytest.mark.parametrize("up_dtype", [F32, BF])
def test_ce_scale_grad(up_dtype):
    x = _mk("wide", 1, R.SCALE_N)[0]
    for s in (0.3, -1.7):
        got = R.launch_scale(x, torch.tensor(s, dtype=up_dtype, device=DEV))
        assert got.pop("nonunit") == 1
        _check(f"ce_scale {up_dtype} {s}", got, R.ref_scale(x, s))
    got = R.launch_scale(x, torch.tensor(1.0, dtype=up_dtype, device=DEV))
    assert got["nonunit"] == 0 and torch.equal(got["dx"], x)


# ------------------------------------------------------------------------------------------ embedding backward
@pytest.mark.parametrize("dim", R.EMB_DIMS)
def test_embedding_bwd(dim):
    for n in R.EMB_N:
        for dt in (BF, F32):
            for kind in R.ID_KINDS:
                ids = R.make_ids(kind, n, R.EMB_V, device=DEV)
                dy = _mk("randn" if kind == "random" else "bait", n, dim, 1)
                g0 = _mk("randn", R.EMB_V, dim, 2).to(dt)
                got = R.launch_embedding(g0, ids, dy, 0.5)
                _check(f"emb n{n} dim{dim} {dt} {kind}", got, R.ref_embedding(g0, ids, dy, 0.5))
                untouched = torch.ones(R.EMB_V, dtype=torch.bool, device=DEV)
                untouched[ids] = False
                assert torch.equal(got["grad"][untouched], g0[untouched]), "an untouched row changed"
                again = R.launch_embedding(g0, ids, dy, 0.5)
                assert torch.equal(again["grad"], got["grad"]), "two calls differ"


# ------------------------------------------------------------------------------------------ wrappers
def test_wrappers_copy_views_at_odd_offsets():
    """A view at element offset 4 (8 bytes: not 16-byte aligned) gives the same bits as an aligned clone: the
    wrappers copy it instead of handing the pointer to the 16-byte vector kernels."""
    from picotron_amd import ops
    rows, cols = 5, 520

    def view_of(t):
        flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
        v = flat[4:4 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 8
        return v

    x, res, dy = _mk("randn", rows, cols), _mk("randn", rows, cols, 1), _mk("randn", rows, cols, 3)
    w = _mk("randn", 1, cols, 2)[0]
    outs = []
    for f in (lambda t: t.clone(), view_of):
        xx, ww = f(x).requires_grad_(True), f(w).requires_grad_(True)
        y, ro = ops.rms_norm(xx, ww, EPS, residual=f(res), prenorm=True)
        y.backward(f(dy))
        outs.append((y.detach(), ro.detach(), xx.grad, ww.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    lg, t = R.make_ce("randn", 4104, device=DEV)
    outs = []
    for f in (lambda t_: t_.clone(), view_of):
        ll = f(lg).requires_grad_(True)
        loss = ops.cross_entropy(ll, t, ignore_index=R.IGNORE)
        loss.backward()
        outs.append((loss.detach(), ll.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
