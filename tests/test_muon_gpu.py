"""picotron_amd.optim.Muon and its kernels (csrc/muon.hip) against torch on the same data.

Criterion E, tests/test_optim_gpu.py's criterion against torch's elementwise kernels: no element differs by more than
1 bf16 ulp, except where both values are below 1e-12 in magnitude, and fewer than 1e-3 of the elements differ at all.

Sums of squares: 2**-16 relative against the fp64 sum, the bound derived at the top of tests/test_grad_clip_gpu.py
for this summation order.

End to end (test 4) the yardstick calibrates itself: with p = 0, lr = 1, weight_decay = 0 the stored parameter is
bf16(-ratio * O); per matrix e = ||p_torch - p_64|| / ||p_64|| is torch.optim.Muon's own bf16 error against an fp64
restatement of the algorithm, and ours must lie within e of torch's: ||p_ours - p_torch|| / ||p_64|| <= e.

Precondition on inputs (a condition, not a tolerance): the Newton-Schulz input is divided by a norm rounded to bf16,
and a norm that rounds to the other neighbour moves the output by ~2e-2 relative. Every (gradient, buffer) pair is
therefore drawn from a fixed seed such that the fp64 norm of the reference u lies at least 2**-12 relative from the
nearest midpoint between adjacent bf16 values, moving to the next seed otherwise (at most 8 times: the band excludes
at most 1/8 of the draws)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TOL = 2.0 ** -16
CO = (3.4445, -4.7750, 2.0315)
# (8, 8): smallest square; (40, 72) x2: two slices of one work buffer; (128, 64) x2: tall, transposed GEMM view;
# (1000, 3): numel % 8 != 0, scalar path, tall; (2, 32772): 65,544 elements, the second chunk has 8; (513, 128):
# crosses a chunk on the vector path; then (16, 24) as a view at element offset 1 (unaligned, scalar path)
SHAPES = [(8, 8), (40, 72), (40, 72), (128, 64), (128, 64), (1000, 3), (2, 32772), (513, 128), (16, 24)]


def _ulp_diff(a, b):
    return (a.view(torch.int16).to(torch.int32) - b.view(torch.int16).to(torch.int32)).abs()


def _assert_e(x, y, what):
    """Criterion E."""
    d = _ulp_diff(x, y)
    bad = (d > 1) & ~((x.float().abs() < 1e-12) & (y.float().abs() < 1e-12))
    assert not bool(bad.any()), (what, int(d.max()))
    assert float((d > 0).float().mean()) < 1e-3, what


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _alloc(shape, last):
    """An uninitialised bf16 tensor of `shape`; last: a view at element offset 1 of a larger buffer."""
    if not last:
        return torch.empty(shape, device="cuda", dtype=BF)
    t = torch.empty(1 + shape[0] * shape[1], device="cuda", dtype=BF)[1:].view(shape)
    assert t.data_ptr() % 16 == 2 and t.is_contiguous()
    return t


def _like(values):
    """Copies of `values` laid out as the test's tensors are (the last one unaligned)."""
    out = []
    for i, v in enumerate(values):
        t = _alloc(tuple(v.shape), i == len(values) - 1)
        t.copy_(v)
        out.append(t)
    return out


def _midpoint_distance(x):
    """Relative distance of x > 0 from the nearest midpoint between adjacent bf16 values (8 significand bits)."""
    ulp = 2.0 ** (math.floor(math.log2(x)) - 7)
    return abs((x / ulp) % 1.0 - 0.5) * ulp / x


def _ref_u(g, m, momentum, nesterov):
    m1 = torch.lerp(m, g, 1 - momentum)
    return m1, (torch.lerp(g, m1, momentum) if nesterov else m1)


def _draw(shape, m, momentum, nesterov, seed, scale=1.0):
    """A bf16 gradient for buffer m that meets the precondition (module docstring)."""
    for k in range(8):
        gen = torch.Generator(device="cuda").manual_seed(1000 * seed + k)
        g = (torch.randn(shape, device="cuda", generator=gen) * scale).to(BF)
        nrm = float(_ref_u(g, m, momentum, nesterov)[1].double().norm())
        if _midpoint_distance(nrm) >= 2.0 ** -12:
            return g
    raise AssertionError(f"no draw in 8 seeds met the precondition for {shape}")


def _inputs(momentum, nesterov, seed):
    """(gradients, buffers) for SHAPES, each pair meeting the precondition."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ms = [(torch.randn(s, device="cuda", generator=gen) * 0.5).to(BF) for s in SHAPES]
    gs = [_draw(s, m, momentum, nesterov, seed * 100 + i) for i, (s, m) in enumerate(zip(SHAPES, ms))]
    return gs, ms


class _Tables:
    """The device tables of the three entry points for the test's tensors, built as Muon.step() builds them."""

    def __init__(self, ps, gs, ms, adjust_lr_fn=None, f32=False):
        from picotron_amd import _lib
        from picotron_amd.optim import _muon_layout, _muon_work, _new_tables, _sync_ptrs
        self.L, self.lib, dev = _lib, _lib.load(), ps[0].device
        self.layout = _muon_layout([p.shape for p in ps], adjust_lr_fn)
        self.ent = _new_tables([p.numel() for p in ps], dev, "out")
        self.bufs, self.work = _muon_work(self.layout, dev)
        self.out = [torch.empty_like(w) for w in self.work]
        _sync_ptrs(self.ent, [(p.data_ptr(), g.data_ptr(), m.data_ptr(), w.data_ptr(), 1 if f32 else 0, o.data_ptr())
                              for p, g, m, w, o in zip(ps, gs, ms, self.work, self.out)], dev)
        self.chunk_start = torch.tensor(self.layout["chunk_start"], dtype=torch.int64, device=dev)
        self.ratios = torch.tensor(self.layout["ratios"], dtype=torch.float64, device=dev)
        self.partials = torch.zeros(self.ent["n_chunks"], dtype=torch.float32, device=dev)
        self.norms = torch.zeros(len(ps), dtype=torch.float32, device=dev)
        self.n = len(ps)
        self.stream = _lib.stream_of(ps[0])

    def _common(self):
        e, P = self.ent, self.L.ptr
        return P(e["tens"]), P(e["sizes"]), P(e["chunks"]), e["n_chunks"]

    def momentum(self, momentum, nesterov):
        t, s, c, n = self._common()
        self.L.check(self.lib.pico_muon_momentum(t, s, c, n, momentum, int(nesterov), self.L.ptr(self.partials),
                                                 self.stream), "pico_muon_momentum")

    def normalize(self, eps):
        t, s, c, n = self._common()
        self.L.check(self.lib.pico_muon_normalize(t, s, c, n, self.L.ptr(self.chunk_start), self.n,
                                                  self.L.ptr(self.partials), eps, self.L.ptr(self.norms), self.stream),
                     "pico_muon_normalize")

    def update(self, lr, wd):
        t, s, c, n = self._common()
        self.L.check(self.lib.pico_muon_update(t, self.L.ptr(self.ent["out"]), s, c, n, lr, wd,
                                               self.L.ptr(self.ratios), self.stream), "pico_muon_update")


# ---- 1. the momentum kernel through the ABI ----

@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("momentum", [0.95, 0.0])
def test_momentum_kernel(momentum, nesterov):
    gs, ms = _inputs(momentum, nesterov, 11)
    gs, ms0 = _like(gs), _like(ms)
    ms = _like(ms0)
    tb = _Tables(ms, gs, ms)  # the param column is not read
    assert tb.layout["chunk_start"][-1] == tb.ent["n_chunks"] == len(SHAPES) + 2
    tb.momentum(momentum, nesterov)
    partials = tb.partials.double().cpu()
    for i, (g, m0, m, u) in enumerate(zip(gs, ms0, ms, tb.work)):
        m_ref = torch.lerp(m0, g, 1 - momentum)
        _assert_e(m, m_ref, ("m'", i))
        # u from m' after its rounding (the stored value)
        _assert_e(u, torch.lerp(g, m, momentum) if nesterov else m, ("u", i))
        if momentum == 0.0:
            assert _bits_equal(m, g) or bool((m == g).all())
        flat = u.double().flatten()
        c0, c1 = tb.layout["chunk_start"][i], tb.layout["chunk_start"][i + 1]
        for c in range(c0, c1):
            want = float(flat[(c - c0) * 65536:(c - c0 + 1) * 65536].square().sum())
            got = float(partials[c])
            print(f"momentum={momentum} nesterov={nesterov} tensor {i} chunk {c}: rel {abs(got - want) / want:.3e}")
            assert abs(got - want) <= TOL * want, (i, c, got, want)
        # the tensor's norm before its bf16 rounding: the chunk partials added in index order in double
        nrm, want = math.sqrt(sum(float(x) for x in partials[c0:c1])), float(flat.norm())
        assert abs(nrm - want) <= TOL * want, (i, nrm, want)


# ---- 2. normalize through the ABI ----

def test_normalize_kernel():
    eps = 1e-7
    gs, ms = _inputs(0.95, True, 12)
    gs, ms = _like(gs), _like(ms)
    zero = len(SHAPES) - 2  # one all-zero u: the (513, 128) matrix
    gs[zero].zero_()
    ms[zero].zero_()
    tb = _Tables(ms, gs, ms)
    tb.momentum(0.95, True)
    us = [w.clone() for w in tb.work]
    partials = tb.partials.double().cpu()
    tb.normalize(eps)
    first = [w.clone() for w in tb.work]
    norms = tb.norms.cpu()
    for i, (u, x0) in enumerate(zip(us, first)):
        c0, c1 = tb.layout["chunk_start"][i], tb.layout["chunk_start"][i + 1]
        s = 0.0
        for x in partials[c0:c1]:
            s += float(x)
        want = max(float(torch.tensor(math.sqrt(s), dtype=torch.float32).to(BF)), float(torch.tensor(eps).float()))
        assert float(norms[i]) == want, (i, float(norms[i]), want)
        if i == zero:
            assert float(norms[i]) == float(torch.tensor(eps).float())
            assert bool((x0 == 0).all()) and bool(torch.isfinite(x0.float()).all())
            continue
        assert float(norms[i]) == float(u.norm()), i  # torch's bf16 norm(): the precondition holds
        _assert_e(x0, u / u.norm().clamp(min=eps), ("X0", i))
    # the same bits on a second run from the same inputs
    for w, u in zip(tb.work, us):
        w.copy_(u)
    tb.normalize(eps)
    for i, (w, x0) in enumerate(zip(tb.work, first)):
        assert _bits_equal(w, x0), i
    assert torch.equal(tb.norms.cpu(), norms)


# ---- 3. the update kernel through the ABI ----

@pytest.mark.parametrize("lr,wd", [(0.02, 0.1), (1.0, 0.0), (3e-4, 0.01)])
@pytest.mark.parametrize("adjust_lr_fn", ["original", "match_rms_adamw"])
def test_update_kernel(lr, wd, adjust_lr_fn):
    from torch.optim._muon import _adjust_lr
    gen = torch.Generator(device="cuda").manual_seed(13)
    base = [torch.randn(s, device="cuda", generator=gen).to(BF) for s in SHAPES]
    ps = _like(base)
    tb = _Tables(ps, ps, ps, adjust_lr_fn)  # only the param column and out_ptrs are read
    for o, s in zip(tb.out, SHAPES):
        o.copy_((torch.randn(s, device="cuda", generator=gen) * 0.3).to(BF))
    tb.update(lr, wd)
    for i, (p, b, o) in enumerate(zip(ps, base, tb.out)):
        ref = b.clone()
        ref.mul_(1 - lr * wd)
        ref.add_(o, alpha=-_adjust_lr(lr, adjust_lr_fn, b.shape))
        _assert_e(p, ref, ("p", i, lr, wd, adjust_lr_fn))


# ---- 4. end to end against torch.optim.Muon ----

def _p64(g, m, momentum, nesterov, eps, ns_steps, ratio):
    """Steps 1-7 in fp64 on the CPU from the same bf16 inputs, p = 0, lr = 1, weight_decay = 0: -ratio * O."""
    g, m = g.double().cpu(), m.double().cpu()
    m1 = m + (1 - momentum) * (g - m)
    u = g + momentum * (m1 - g) if nesterov else m1
    x = u / max(float(u.norm()), eps)
    tall = x.shape[0] > x.shape[1]
    if tall:
        x = x.T
    a, b, c = CO
    for _ in range(ns_steps):
        gm = x @ x.T
        x = a * x + (b * gm + c * (gm @ gm)) @ x
    return -ratio * (x.T if tall else x)


@pytest.mark.parametrize("nesterov,adjust_lr_fn", [(True, None), (False, "match_rms_adamw")])
def test_step_matches_torch_muon(nesterov, adjust_lr_fn):
    from picotron_amd.optim import Muon, _muon_ratio
    momentum, eps, ns_steps = 0.95, 1e-7, 5
    gen = torch.Generator(device="cuda").manual_seed(14)
    ms = [(torch.randn(s, device="cuda", generator=gen) * 0.5).to(BF) for s in SHAPES]
    zeros = [torch.zeros(s, device="cuda", dtype=BF) for s in SHAPES]
    ours = [torch.nn.Parameter(t) for t in _like(zeros)]
    ref = [torch.nn.Parameter(t) for t in _like(zeros)]
    kw = dict(lr=1.0, weight_decay=0.0, momentum=momentum, nesterov=nesterov, eps=eps, ns_steps=ns_steps,
              adjust_lr_fn=adjust_lr_fn)
    o1, o2 = Muon(ours, **kw), torch.optim.Muon(ref, **kw)
    for a, b, m in zip(ours, ref, _like(ms)):
        o1.state[a]["momentum_buffer"] = m
        o2.state[b]["momentum_buffer"] = m.clone()
    worst = 0.0
    for step in range(3):
        before = [o2.state[b]["momentum_buffer"].clone() for b in ref]
        gs = [_draw(s, m, momentum, nesterov, 7000 + 100 * step + i, 10.0 ** (step - 1))
              for i, (s, m) in enumerate(zip(SHAPES, before))]
        for a, b, g in zip(ours, ref, _like(gs)):
            a.grad, b.grad = g, g.clone()
        o1.step()
        o2.step()
        for i, (a, b, g, m0) in enumerate(zip(ours, ref, gs, before)):
            p64 = _p64(g, m0, momentum, nesterov, eps, ns_steps, _muon_ratio(adjust_lr_fn, SHAPES[i]))
            den = float(p64.norm())
            e = float((b.detach().double().cpu() - p64).norm()) / den
            d = float((a.detach().double() - b.detach().double()).norm()) / den
            print(f"nesterov={nesterov} step {step} {SHAPES[i]}: e {e:.3e} "
                  f"ours-torch {d:.3e} ratio {d / e:.3f}")
            worst = max(worst, d / e)
            assert bool(torch.isfinite(a.detach().float()).all()) and d <= e, (step, SHAPES[i], d, e)
            m_ours, m_ref = o1.state[a]["momentum_buffer"], o2.state[b]["momentum_buffer"]
            if nesterov:
                _assert_e(m_ours, m_ref, ("momentum_buffer", step, i))
                m_ours.copy_(m_ref)  # re-sync, so each step is compared from identical states
            else:  # torch 2.10 normalises its buffer in place here: ours keeps m', checked against the lerp
                want = torch.lerp(m0, g, 1 - momentum)
                _assert_e(m_ours, want, ("momentum_buffer", step, i))
                m_ours.copy_(want)
                m_ref.copy_(want)
            with torch.no_grad():
                a.zero_()
                b.zero_()
    print(f"nesterov={nesterov}: largest yardstick ratio {worst:.3f}")
    assert set(o1.state[ours[0]]) == set(o2.state[ref[0]]) == {"momentum_buffer"}


# ---- 5. a realistic step through the zero-norm clamp ----

def test_zero_gradient_step_is_weight_decay_alone():
    from picotron_amd.optim import Muon
    gen = torch.Generator(device="cuda").manual_seed(15)
    base = [torch.randn(s, device="cuda", generator=gen).to(BF) for s in SHAPES]
    ps = [torch.nn.Parameter(t) for t in _like(base)]
    for p in ps:
        p.grad = torch.zeros_like(p)
    opt = Muon(ps, lr=0.02, weight_decay=0.1)
    opt.step()
    decay = torch.tensor(1 - 0.02 * 0.1, dtype=torch.float32, device="cuda")
    for i, (p, b) in enumerate(zip(ps, base)):
        assert bool(torch.isfinite(p.detach().float()).all()), i
        assert _bits_equal(p.detach(), (b.float() * decay).to(BF)), i
        assert bool((opt.state[p]["momentum_buffer"] == 0).all())


# ---- 6. the deferred fp32 main_grad ----

def test_deferred_main_grad_is_bit_identical_to_cast_then_step():
    from picotron_amd.optim import Muon
    gen = torch.Generator(device="cuda").manual_seed(16)
    base = [torch.randn(s, device="cuda", generator=gen).to(BF) for s in SHAPES]
    a = [torch.nn.Parameter(t) for t in _like(base)]
    b = [torch.nn.Parameter(t) for t in _like(base)]
    o1, o2 = Muon(a, lr=0.02), Muon(b, lr=0.02)
    for step in range(2):
        for x, y in zip(a, b):
            g32 = torch.randn(x.shape, device="cuda", generator=gen) * 0.1
            x.grad = torch.full_like(x, 3.0)  # stale: must not be read
            x._pico_grad_f32 = g32
            x._pico_grad_deferred = True
            y.grad = g32.to(BF)
        o1.step()
        o2.step()
        for i, (x, y) in enumerate(zip(a, b)):
            assert _bits_equal(x.detach(), y.detach()), (step, i)
            assert _bits_equal(o1.state[x]["momentum_buffer"], o2.state[y]["momentum_buffer"]), (step, i)
    (ent,) = o1._tables.values()
    assert all(t[4] == 1 for t in ent["ptrs"])


# ---- 7. steady state ----

def test_steady_state_allocates_and_uploads_nothing():
    from picotron_amd.optim import Muon
    gen = torch.Generator(device="cuda").manual_seed(17)
    base = [torch.randn(s, device="cuda", generator=gen).to(BF) for s in SHAPES]
    grads = [[(torch.randn(s, device="cuda", generator=gen) * 0.1).to(BF) for s in SHAPES] for _ in range(3)]

    def run():
        ps = [torch.nn.Parameter(t) for t in _like(base)]
        for p in ps:
            p.grad = torch.zeros_like(p)  # persistent gradient buffers
        opt = Muon(ps, lr=0.02, adjust_lr_fn="match_rms_adamw")
        for k in range(2):
            for p, g in zip(ps, grads[k]):
                p.grad.copy_(g)
            opt.step()
        tables = dict(opt._tables)
        (ent,) = tables.values()
        uploaded = ent["ptrs"]
        for p, g in zip(ps, grads[2]):
            p.grad.copy_(g)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        opt.step()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        assert dict(opt._tables) == tables and ent["ptrs"] is uploaded and len(uploaded[0]) == 6
        assert ent["out"].data_ptr() == ent["buf"].data_ptr() + 8 * 5 * len(ps)  # one buffer, one upload
        return [p.detach().clone() for p in ps]

    first, second = run(), run()
    for i, (x, y) in enumerate(zip(first, second)):
        assert _bits_equal(x, y), i


# ---- 8. refusals on the device ----

def test_refusals_leave_the_state_empty():
    from picotron_amd.optim import Muon
    p = torch.nn.Parameter(torch.randn(8, 16, device="cuda"))  # fp32
    p.grad = torch.randn(8, 16, device="cuda")
    opt = Muon([p])
    with pytest.raises(TypeError, match="bf16 HIP tensors"):
        opt.step()
    assert len(opt.state) == 0
    q = torch.nn.Parameter(torch.randn(8, 16, device="cuda").to(BF))
    q.grad = torch.randn(16, 8, device="cuda").to(BF).T  # not contiguous
    opt = Muon([q])
    with pytest.raises(ValueError, match="contiguous"):
        opt.step()
    assert len(opt.state) == 0
    with pytest.raises(ValueError, match="2D"):
        Muon([torch.nn.Parameter(torch.randn(16, device="cuda").to(BF))])
