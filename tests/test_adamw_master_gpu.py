"""pico_adamw_master (picotron_amd.optim.AdamW(master_weights=True)): fp32 master weights and fp32 moments under
bf16 parameters, against torch.optim.AdamW(fused=True) on fp32 clones and against the same step evaluated in fp64.

Criterion of the parity tests, per tensor and per quantity (master, exp_avg, exp_avg_sq):
max|ours - f64| <= 2 * max|torch32 - f64|. Both are one fp32 rounding of the same double-evaluated expression, so a
factor of two covers a differing contraction and nothing more. The bf16 parameter is bitwise master.to(bfloat16).
Everything the feature claims to be "the same as" (clip-then-step, cast-then-step, a reloaded checkpoint, the graph
step) is compared bit for bit.

The largest fp32-ulp distance to torch is printed, not gated. Measured on MI355X: 0 for exp_avg and exp_avg_sq in
every tensor and step; the master differs from torch's by one rounding of the update's operands (at most 4 ulps of
max(|p before|, |p after|)), which is up to 2**18 ulps of the result where the update cancels a weight to near zero,
while max|ours - f64| equals max|torch32 - f64| to three digits in every tensor.
"""
import gc
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
SHAPES = [(2048,), (6144, 2048), (1000, 3), (7,), (65536 + 8,), (3, 5, 40)]  # + an unaligned 6000-element view


def _base(seed):
    """bf16 values for the parameter list; the last is a [1:] view (storage offset 2 bytes: the scalar path)."""
    torch.manual_seed(seed)
    base = [torch.randn(s, device="cuda").to(BF) for s in SHAPES]
    base.append(torch.randn(1 + 6000, device="cuda").to(BF)[1:])
    return base


def _params(base):
    """Own copies of `base` as parameters, the last one again an unaligned view."""
    ps = [torch.nn.Parameter(t.clone()) for t in base[:-1]]
    big = torch.zeros(base[-1].numel() + 1, device="cuda", dtype=BF)
    big[1:] = base[-1]
    ps.append(torch.nn.Parameter(big[1:]))
    assert ps[-1].data_ptr() % 16 == 2 and ps[-1].is_contiguous()
    return ps


def _grads(shapes, mag, gen):
    return [(torch.randn(s, device="cuda", generator=gen) * mag).to(BF) for s in shapes]


def _unaligned(g):
    big = torch.zeros(g.numel() + 1, device="cuda", dtype=g.dtype)
    big[1:] = g.reshape(-1)
    return big[1:].view(g.shape)


def _set(ps, grads):
    """Own copies of `grads` as the .grad of `ps` (None: no gradient); the last one an unaligned view."""
    for i, (p, g) in enumerate(zip(ps, grads)):
        p._pico_grad_deferred = False
        p.grad = None if g is None else (_unaligned(g) if i == len(ps) - 1 else g.clone())


def _bits(t):
    return t.detach().view({F32: torch.int32, BF: torch.int16}[t.dtype])


def _ulps32(a, b):
    """Distance in fp32 ulps (bit patterns ordered like the values)."""
    def o(x):
        i = x.detach().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (o(a) - o(b)).abs()


def _f64_step(p, g, m, v, lr, wd, step, b1=0.9, b2=0.999, eps=1e-8):
    """The AdamW step (decoupled decay) in fp64 from fp32 / bf16 inputs; returns (p, m, v) as fp64."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    p = p - lr * wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1 - b2 ** step) + eps
    return p - (lr / (1 - b1 ** step)) * m / denom, m, v


def _assert_same(o1, ps1, o2, ps2, what):
    for a, b in zip(ps1, ps2):
        assert torch.equal(_bits(a), _bits(b)), (what, "param", tuple(a.shape))
        assert (a in o1.state) == (b in o2.state)
        if a in o1.state:
            for key in ("master_param", "exp_avg", "exp_avg_sq"):
                x, y = o1.state[a][key], o2.state[b][key]
                assert x.dtype == F32 and y.dtype == F32
                assert torch.equal(_bits(x), _bits(y)), (what, key, tuple(a.shape))
            assert float(o1.state[a]["step"]) == float(o2.state[b]["step"])


def _check_against_torch(ours, o1, ref, o2, before, hyper, what):
    """The criterion of the module docstring for every parameter that stepped; `before`: per parameter (p32, g, m,
    v, step number) going into the step, `hyper`: per parameter (lr, wd). Returns the largest fp32-ulp distance to
    torch. Then re-synchronises our state to torch's, so each step is compared from identical states."""
    worst = 0
    for a, b, pre, (lr, wd) in zip(ours, ref, before, hyper):
        if pre is None:
            continue
        want = _f64_step(*pre[:4], lr, wd, pre[4])
        st1, st2 = o1.state[a], o2.state[b]
        for name, x, y, w in (("master", st1["master_param"], b.detach(), want[0]),
                              ("exp_avg", st1["exp_avg"], st2["exp_avg"], want[1]),
                              ("exp_avg_sq", st1["exp_avg_sq"], st2["exp_avg_sq"], want[2])):
            assert x.dtype == F32 and x.shape == a.shape
            e_ours = float((x.double() - w).abs().max())
            e_torch = float((y.double() - w).abs().max())
            ulps = int(_ulps32(x, y).max())
            worst = max(worst, ulps)
            # the same distance in ulps of the larger of |value before| and |value after|: an update that cancels
            # to near zero carries the rounding of its operands, many ulps of the small result
            scale = torch.maximum(pre[0].abs(), x.abs()) if name == "master" else x.abs()
            at_scale = float(((x.double() - y.double()).abs() / torch.ldexp(torch.ones_like(scale), torch.frexp(
                scale.clamp_min(1e-30)).exponent - 24).double()).max())
            print(f"{what} {tuple(a.shape)} {name}: |ours-f64|={e_ours:.3g} |torch32-f64|={e_torch:.3g} "
                  f"max fp32 ulps to torch={ulps} (at the operands' scale: {at_scale:.3g})")
            assert e_ours <= 2 * e_torch, (what, tuple(a.shape), name, e_ours, e_torch)
        assert torch.equal(_bits(a), _bits(st1["master_param"].to(BF))), (what, tuple(a.shape))
        with torch.no_grad():
            st1["master_param"].copy_(b)
            st1["exp_avg"].copy_(st2["exp_avg"])
            st1["exp_avg_sq"].copy_(st2["exp_avg_sq"])
    return worst


def _snapshot(ref, o2, grads):
    out = []
    for b, g in zip(ref, grads):
        if g is None:
            out.append(None)
            continue
        st = o2.state.get(b, {})
        m = st["exp_avg"].clone() if st else torch.zeros_like(b)
        v = st["exp_avg_sq"].clone() if st else torch.zeros_like(b)
        out.append((b.detach().clone(), g.float(), m, v, (int(st["step"]) if st else 0) + 1))
    return out


@pytest.mark.parametrize("wd,lr", [(0.01, 3e-4), (0.0, 1e-2), (0.1, 1e-3)])
def test_master_matches_torch_fp32(wd, lr):
    from picotron_amd.optim import AdamW
    base = _base(0)
    ours = _params(base)
    ref = [torch.nn.Parameter(t.float()) for t in base]
    o1 = AdamW(ours, lr=lr, weight_decay=wd, master_weights=True)
    o2 = torch.optim.AdamW(ref, lr=lr, weight_decay=wd, fused=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    worst = 0
    for step in range(4):
        grads = _grads([t.shape for t in base], 10.0 ** (step - 2), gen)
        _set(ours, grads)
        for b, g in zip(ref, grads):
            b.grad = g.float()
        before = _snapshot(ref, o2, grads)
        o1.step()
        o2.step()
        worst = max(worst, _check_against_torch(ours, o1, ref, o2, before, [(lr, wd)] * len(ours), f"step {step}"))
    print(f"wd={wd} lr={lr}: largest fp32-ulp distance to torch over 4 steps = {worst}")
    assert set(o1.state[ours[0]]) == set(o2.state[ref[0]]) | {"master_param"}
    assert float(o1.state[ours[0]]["step"]) == 4.0


def test_master_param_groups_and_step_counts():
    """Two groups with their own lr / weight_decay, one parameter idle on one step: torch's fp32 optimizer under
    the same criterion, and torch's step counters."""
    from picotron_amd.optim import AdamW
    torch.manual_seed(2)
    base = [torch.randn(s, device="cuda").to(BF) for s in [(512,), (64, 33), (300,), (65536 + 8,)]]
    ours = [torch.nn.Parameter(t.clone()) for t in base]
    ref = [torch.nn.Parameter(t.float()) for t in base]
    hyper = [(1e-2, 0.01), (1e-2, 0.01), (3e-4, 0.1), (3e-4, 0.1)]

    def groups(ps):
        return [{"params": ps[:2], "lr": 1e-2, "weight_decay": 0.01}, {"params": ps[2:], "lr": 3e-4, "weight_decay": 0.1}]
    o1 = AdamW(groups(ours), master_weights=True)
    o2 = torch.optim.AdamW(groups(ref), fused=True)
    gen = torch.Generator(device="cuda").manual_seed(3)
    for step in range(4):
        grads = _grads([t.shape for t in base], 1.0, gen)
        if step == 1:
            grads[1] = None
        for a, b, g in zip(ours, ref, grads):
            a.grad = None if g is None else g.clone()
            b.grad = None if g is None else g.float()
        before = _snapshot(ref, o2, grads)
        o1.step()
        o2.step()
        _check_against_torch(ours, o1, ref, o2, before, hyper, f"step {step}")
    assert [float(o1.state[p]["step"]) for p in ours] == [4.0, 3.0, 4.0, 4.0]
    assert [float(o2.state[p]["step"]) for p in ref] == [4.0, 3.0, 4.0, 4.0]


def test_master_clip_equals_clip_then_step():
    from picotron_amd.optim import AdamW, clip_grad_norm_
    c = 1.0
    base = _base(4)
    fused, unfused = _params(base), _params(base)
    o1 = AdamW(fused, lr=1e-2, weight_decay=0.01, master_weights=True, max_grad_norm=c)
    o2 = AdamW(unfused, lr=1e-2, weight_decay=0.01, master_weights=True)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for step, mag in enumerate([1.0, 1e-6, 1.0]):  # norm ~ 3500, 0.0035, 3500: the coefficient below 1, 1, below 1
        grads = _grads([t.shape for t in base], mag, gen)
        _set(fused, grads)
        _set(unfused, grads)
        o1.step()
        ret = clip_grad_norm_(unfused, c, groups=())
        coef = float(ret._base[1])
        assert (coef < 1.0) == (mag == 1.0), (step, coef)
        o2.step()
        assert torch.equal(o1.grad_norm, ret)
        _assert_same(o1, fused, o2, unfused, step)
        for p in fused:
            assert torch.equal(_bits(p), _bits(o1.state[p]["master_param"].to(BF)))


def test_master_clip_with_huge_max_norm_is_the_unclipped_step():
    from picotron_amd.optim import AdamW
    base = _base(6)
    a, b = _params(base), _params(base)
    o1 = AdamW(a, lr=3e-3, weight_decay=0.1, master_weights=True, max_grad_norm=1e30)
    o2 = AdamW(b, lr=3e-3, weight_decay=0.1, master_weights=True)
    gen = torch.Generator(device="cuda").manual_seed(7)
    for step, mag in enumerate([1.0, 100.0]):
        grads = _grads([t.shape for t in base], mag, gen)
        _set(a, grads)
        _set(b, grads)
        o1.step()
        o2.step()
        _assert_same(o1, a, o2, b, step)


def test_master_non_finite_gradient_skips_the_update():
    from picotron_amd.optim import AdamW
    base = _base(8)
    ps = _params(base)
    opt = AdamW(ps, lr=1e-2, weight_decay=0.01, master_weights=True, max_grad_norm=1.0)
    gen = torch.Generator(device="cuda").manual_seed(9)
    _set(ps, _grads([t.shape for t in base], 1.0, gen))
    opt.step()
    assert bool(torch.isfinite(opt.grad_norm))
    snap = [(p.detach().clone(), {k: opt.state[p][k].clone() for k in ("master_param", "exp_avg", "exp_avg_sq")})
            for p in ps]
    _set(ps, _grads([t.shape for t in base], 1.0, gen))
    ps[2].grad.view(-1)[17] = float("inf")
    opt.step()
    assert not math.isfinite(float(opt.grad_norm))
    for p, (w, st) in zip(ps, snap):
        assert torch.equal(_bits(p), _bits(w))
        for k, t in st.items():
            assert torch.equal(_bits(opt.state[p][k]), _bits(t)), k


@pytest.mark.parametrize("clip", [None, 1.0])
def test_master_deferred_main_grad_equals_cast_then_step(clip):
    """A deferred fp32 main_grad (DataParallelBucket(defer_grad_cast=True): .grad is the stale, not-yet-cast bf16
    tensor) gives the bits of casting to bf16 first and then stepping; vector and scalar paths of the fp32 load."""
    from picotron_amd.optim import AdamW
    base = _base(10)
    a, b = _params(base), _params(base)
    o1 = AdamW(a, lr=1e-2, weight_decay=0.01, master_weights=True, max_grad_norm=clip)
    o2 = AdamW(b, lr=1e-2, weight_decay=0.01, master_weights=True, max_grad_norm=clip)
    gen = torch.Generator(device="cuda").manual_seed(11)
    for step in range(2):
        g32 = [torch.randn(t.shape, device="cuda", generator=gen) for t in base]
        assert not torch.equal(g32[0].to(BF).float(), g32[0])
        g32[-1] = _unaligned(g32[-1])  # 4 bytes off: the scalar path of the fp32 form
        for p, g in zip(a, g32):
            p.grad = torch.full(g.shape, 3.0, device="cuda", dtype=BF)  # stale: must not be read
            p._pico_grad_f32 = g
            p._pico_grad_deferred = True
        _set(b, [g.to(BF) for g in g32])
        o1.step()
        o2.step()
        _assert_same(o1, a, o2, b, step)


def test_small_updates_survive_in_master_mode():
    """p = 1, g = +1, lr = 1e-4, no decay, 200 steps: each update (~1e-4) is below half a bf16 ulp at 1.0 (2**-8),
    so the bf16 optimizer never moves; the fp32 master ends at 0.9799967 (torch.optim.AdamW on fp32, CPU)."""
    from picotron_amd.optim import AdamW
    res = {}
    for master in (True, False):
        p = torch.nn.Parameter(torch.ones(8, device="cuda", dtype=BF))
        p.grad = torch.ones(8, device="cuda", dtype=BF)
        opt = AdamW([p], lr=1e-4, weight_decay=0.0, master_weights=master)
        for _ in range(200):
            opt.step()
        res[master] = (p.detach().float().cpu(), opt.state[p].get("master_param"))
    p_master, master = res[True]
    print("master mode: param", p_master.tolist(), "master", master.tolist(), "| bf16 mode: param", res[False][0].tolist())
    assert torch.equal(p_master, torch.full((8,), 0.98046875))  # bf16(0.98)
    assert float((master.cpu() - 0.9799967).abs().max()) <= 1e-5
    assert torch.equal(res[False][0], torch.ones(8))  # why the feature exists


def test_second_moment_decays_in_master_mode():
    """50 steps with g = 1, then 2000 with g = 2**-6, beta2 = 0.999: fp64 gives exp_avg_sq = 0.0068081 (a bf16
    exp_avg_sq cannot decay: 0.999 v rounds back to v, and ends 7x too large)."""
    from picotron_amd.optim import AdamW
    p = torch.nn.Parameter(torch.ones(8, device="cuda", dtype=BF))
    opt = AdamW([p], lr=1e-4, weight_decay=0.0, master_weights=True)
    p.grad = torch.ones(8, device="cuda", dtype=BF)
    for _ in range(50):
        opt.step()
    p.grad.fill_(2.0 ** -6)
    for _ in range(2000):
        opt.step()
    v = opt.state[p]["exp_avg_sq"].double().cpu()
    v64 = 0.0
    for i in range(2050):
        v64 = 0.999 * v64 + 0.001 * (1.0 if i < 50 else 2.0 ** -12)
    assert abs(v64 - 0.0068081) < 1e-7
    rel = float(((v - 0.0068081) / 0.0068081).abs().max())
    print(f"exp_avg_sq={v.tolist()[0]:.9g} fp64={v64:.9g} rel err={rel:.3g}")
    assert rel <= 1e-3


def test_checkpoint_round_trip():
    from picotron_amd.optim import AdamW
    base = _base(12)
    shapes = [t.shape for t in base]
    gen = torch.Generator(device="cuda").manual_seed(13)
    a = _params(base)
    o1 = AdamW(a, lr=1e-2, weight_decay=0.01, master_weights=True, max_grad_norm=1.0)
    for _ in range(2):
        _set(a, _grads(shapes, 1.0, gen))
        o1.step()
    sd = o1.state_dict()
    assert all(st[k].dtype == F32 for st in sd["state"].values() for k in ("master_param", "exp_avg", "exp_avg_sq"))
    b = _params([p.detach() for p in a])
    o2 = AdamW(b, lr=1e-2, weight_decay=0.01, master_weights=True, max_grad_norm=1.0)
    o2.load_state_dict(sd)
    _assert_same(o1, a, o2, b, "loaded")
    grads = _grads(shapes, 1.0, gen)
    _set(a, grads)
    _set(b, grads)
    o1.step()
    o2.step()
    _assert_same(o1, a, o2, b, "step after load")
    assert float(o2.state[b[0]]["step"]) == 3.0


def test_bf16_checkpoint_loads_into_master_mode():
    """A checkpoint of the bf16 optimizer (bf16 moments, no master_param): the moments are upcast exactly and the
    masters are made from the parameters at the next step — the step equals that of a master-mode optimizer whose
    state was set to exactly those fp32 tensors."""
    from picotron_amd.optim import AdamW
    base = _base(14)
    shapes = [t.shape for t in base]
    gen = torch.Generator(device="cuda").manual_seed(15)
    old = _params(base)
    o_old = AdamW(old, lr=1e-2, weight_decay=0.01)
    _set(old, _grads(shapes, 1.0, gen))
    o_old.step()
    sd = o_old.state_dict()
    assert all(st["exp_avg"].dtype == BF and "master_param" not in st for st in sd["state"].values())
    a, b = _params([p.detach() for p in old]), _params([p.detach() for p in old])
    o1 = AdamW(a, lr=1e-2, weight_decay=0.01, master_weights=True)
    o1.load_state_dict(sd)
    for p, q in zip(a, old):
        st = o1.state[p]
        assert "master_param" not in st and st["exp_avg"].dtype == F32 and st["exp_avg_sq"].dtype == F32
        assert torch.equal(st["exp_avg"], o_old.state[q]["exp_avg"].float())
        assert torch.equal(st["exp_avg_sq"], o_old.state[q]["exp_avg_sq"].float())
    o2 = AdamW(b, lr=1e-2, weight_decay=0.01, master_weights=True)
    o2.load_state_dict({"param_groups": sd["param_groups"], "state": {
        i: {"step": st["step"].clone(), "exp_avg": st["exp_avg"].float(), "exp_avg_sq": st["exp_avg_sq"].float(),
            "master_param": q.detach().float()} for (i, st), q in zip(sd["state"].items(), old)}})
    grads = _grads(shapes, 1.0, gen)
    _set(a, grads)
    _set(b, grads)
    o1.step()  # creates the masters as float(param), then steps
    o2.step()
    _assert_same(o1, a, o2, b, "first master == float(param)")
    assert float(o1.state[a[0]]["step"]) == 2.0


def test_sync_master_params():
    """The kernel never reads the bf16 parameter: a parameter overwritten after the first step is overridden by its
    master at the next step, unless sync_master_params() re-reads the masters."""
    from picotron_amd.optim import AdamW
    res = {}
    for sync in (False, True):
        torch.manual_seed(16)
        p = torch.nn.Parameter(torch.randn(4096 + 8, device="cuda").to(BF))
        old = p.detach().clone()
        opt = AdamW([p], lr=1e-3, weight_decay=0.0, master_weights=True)
        p.grad = torch.randn(p.shape, device="cuda").to(BF)
        opt.step()
        master = opt.state[p]["master_param"]
        new = (old.float() + 10.0).to(BF)
        with torch.no_grad():
            p.copy_(new)
        if sync:
            opt.sync_master_params()
            assert opt.state[p]["master_param"] is master and torch.equal(master, new.float())
        opt.step()
        res[sync] = (float((p.detach().float() - new.float()).abs().max()),
                     float((p.detach().float() - old.float()).abs().max()))
        assert torch.equal(_bits(p), _bits(master.to(BF)))
    # one Adam step moves a weight by about lr (1e-3) plus one bf16 rounding (|p| < 16: 2**-5)
    assert res[True][0] < 0.05 and res[True][1] > 9.9, res
    assert res[False][1] < 0.05 and res[False][0] > 9.9, res  # the master silently won


def test_master_step_does_not_wait_on_the_host():
    from picotron_amd.optim import AdamW
    base = _base(17)
    ps = _params(base)
    opt = AdamW(ps, lr=1e-2, master_weights=True, max_grad_norm=1.0)
    gen = torch.Generator(device="cuda").manual_seed(18)
    _set(ps, _grads([t.shape for t in base], 1.0, gen))
    opt.step()  # first step: masters and tables are built and uploaded
    tables = dict(opt._tables)
    (ent,) = tables.values()
    uploaded = ent["ptrs"]
    probe = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    flagged = False
    try:
        try:  # where the build has it, a host read of a device value inside the steps raises
            torch.cuda.set_sync_debug_mode("error")
            probe.item()
        except RuntimeError:
            flagged = True
        except Exception as e:  # pragma: no cover
            print("torch.cuda.set_sync_debug_mode is not implemented on this build:", e)
        opt.step()
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode flags a host read on this build:", flagged)
    # the pointer tables, the masters table included, are stable after the first step: nothing is uploaded again
    assert dict(opt._tables) == tables and ent["ptrs"] is uploaded and len(uploaded[0]) == 6
    assert float(opt.state[ps[0]]["step"]) == 3.0


def test_master_under_graph_training_step(golden_loss):
    """TrainingStep(graphs=True) with AdamW(master_weights=True, max_grad_norm=1.0) on the 2-layer model of the
    graph-replay tests (test_model_gpu.test_graph_replay_matches_eager, which asserts bitwise equality of the
    updated parameters with the eager loop): the kernel writes the bf16 parameters in place, so the captured graph
    keeps its pointers. Three steps: finite losses, every parameter bitwise bf16(master) after every step, and the
    parameters after step 3 bitwise those of the same steps with graphs=False."""
    from picotron_amd.data import SyntheticDataLoader
    from picotron_amd.model import LlamaConfig, build_llama
    from picotron_amd.optim import AdamW
    from picotron_amd.train import TrainingStep
    cfg = LlamaConfig(**golden_loss["config"])
    assert cfg.num_hidden_layers == 2
    res = {}
    for graphs in (False, True):
        torch.manual_seed(7)
        m = build_llama(cfg, "cuda", BF)
        with torch.no_grad():
            m.final_proj.weight.normal_(0, 0.02, generator=torch.Generator("cuda").manual_seed(1))
        opt = AdamW(m.parameters(), lr=1e-3, master_weights=True, max_grad_norm=1.0)
        loader = SyntheticDataLoader(2, 128, 3, cfg.vocab_size, seed=5, kind="uniform", num_batches=3, device="cuda")
        step = TrainingStep(m, opt, loader, "cuda", graphs=graphs)
        losses, ptrs = [], None
        for _ in range(3):
            losses.append(step())
            if ptrs is None:  # after the first step: the model lays its weights out at its first forward
                ptrs = [p.data_ptr() for p in m.parameters()]
            for n, p in m.named_parameters():
                assert torch.equal(_bits(p), _bits(opt.state[p]["master_param"].to(BF))), n
        torch.cuda.synchronize()
        assert all(math.isfinite(x) for x in losses), losses
        assert [p.data_ptr() for p in m.parameters()] == ptrs  # the optimizer writes in place
        assert bool(torch.isfinite(opt.grad_norm))
        res[graphs] = (losses, {n: p.detach().clone() for n, p in m.named_parameters()})
        # TrainingStep and its graph object refer to each other (graphs.zero_grads is a bound method of the step):
        # collect them here, with the device idle, so the captured HIP graphs are not destroyed by a later garbage
        # collection in the middle of another test's stream capture
        del step, m, opt
        gc.collect()
        torch.cuda.synchronize()
    assert res[False][0] == res[True][0], (res[False][0], res[True][0])
    for n in res[False][1]:
        assert torch.equal(_bits(res[False][1][n]), _bits(res[True][1][n])), n
