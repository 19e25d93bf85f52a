"""Global gradient norm and clip (csrc/grad_clip.hip, pico_adamw_bf16_clip; picotron_amd.optim.clip_grad_norm_ /
get_grad_norm / AdamW(max_grad_norm=...)) against fp64 torch arithmetic on the same data.

Tolerance on the norm: 2**-16 relative, a derived bound. Each chunk's sum of squares runs in fp32: a lane's chain
is at most 256 terms long (the scalar path: 256 elements into one accumulator; the vector path: 32 terms into
each of 8 accumulators, then 3 pairwise levels), then 6 wave levels and 2 levels across the four waves, each
square rounded once: <= (256 + 9) * 2**-24 relative on the sum of squares, i.e. <= 7.9e-6 on the norm. The sum
over chunks runs in double and the result is rounded to fp32 once (6e-8). 7.9e-6 + 6e-8 < 2**-16 = 1.53e-5.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TOL = 2.0 ** -16


def _param(grad, deferred=False):
    """A bf16 parameter whose gradient is `grad`: a bf16 tensor, or (deferred) an fp32 main_grad presented the
    way DataParallelBucket(defer_grad_cast=True) leaves it (.grad is the not-yet-cast bf16 view)."""
    p = torch.nn.Parameter(torch.randn(grad.shape, device="cuda").to(BF))
    if deferred:
        p.grad = torch.full(grad.shape, 3.0, device="cuda", dtype=BF)  # stale: must not be read
        p._pico_grad_f32 = grad
        p._pico_grad_deferred = True
    else:
        p.grad = grad
    return p


def _grad_of(p):
    return p._pico_grad_f32 if getattr(p, "_pico_grad_deferred", False) else p.grad


def _as_bf16(g):
    return g if g.dtype == BF else g.to(BF)


def _norm64(params):
    tot = torch.zeros((), dtype=torch.float64, device="cuda")
    for p in params:
        if p.grad is not None:
            tot += _as_bf16(_grad_of(p)).double().square().sum()
    return float(tot.sqrt())


def _grad_list(mag, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*shape):
        return torch.randn(shape, device="cuda", generator=g) * mag

    grads = [rn(*s).to(BF) for s in [(2048,), (640, 256), (1000, 3), (7,), (65536,)]]
    tail = rn(65536 + 8)
    tail[-8:] = mag * (65536 / 8) ** 0.5  # the last 8 elements carry about half of this tensor's sum of squares
    grads.append(tail.to(BF))
    grads.append(rn(3, 5, 40).to(BF))
    grads.append(rn(6001).to(BF)[1:])  # storage offset 2 bytes: the unaligned scalar path
    params = [_param(x) for x in grads]
    assert params[-1].grad.data_ptr() % 16 == 2
    f32 = rn(384, 40)  # deferred fp32 main_grad, vector path; values not bf16-representable
    assert not torch.equal(f32.to(BF).float(), f32)
    params.append(_param(f32, deferred=True))
    params.append(_param(rn(333), deferred=True))  # and the scalar path of the fp32 form
    return params


def _sumsq(params):
    """The device double pico_grad_sqnorm leaves for a parameter list (local: every parameter counts)."""
    from picotron_amd import _lib, optim
    ps, ent = optim._grad_tables(params)
    s = optim._sqnorm(_lib.load(), ent, [True] * len(ps), _lib.stream_of(ps[0].grad))
    return s.clone()


def _ordered(x):
    """bf16 bits as integers ordered like the values (sign-magnitude -> two's complement)."""
    i = x.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_norm_against_fp64(k):
    from picotron_amd.optim import get_grad_norm
    params = _grad_list(10.0 ** (k - 2), seed=k)
    ref = _norm64(params)
    norm = get_grad_norm(params, groups=())
    assert norm.dtype == torch.float32 and norm.dim() == 0 and norm.is_cuda
    err = abs(float(norm) - ref) / ref
    print(f"k={k} norm={float(norm):.9g} ref={ref:.9g} rel err={err:.3g}")
    assert err <= TOL, (float(norm), ref, err)
    # a parameter without a gradient is skipped
    extra = torch.nn.Parameter(torch.ones(64, device="cuda", dtype=BF))
    assert float(get_grad_norm(params + [extra], groups=())) == float(norm)


def test_many_chunks_and_determinism():
    from picotron_amd.optim import get_grad_norm
    g = torch.Generator(device="cuda").manual_seed(5)
    small = (torch.randn(1100, 8, device="cuda", generator=g) * 30).to(BF)
    params = [_param(small[i]) for i in range(1100)]
    params.append(_param(torch.randn(300 * 65536, device="cuda", generator=g).to(BF)))  # 1400 partials > 256 lanes
    ref = _norm64(params)
    norm = float(get_grad_norm(params, groups=()))
    err = abs(norm - ref) / ref
    print(f"norm={norm:.9g} ref={ref:.9g} rel err={err:.3g}")
    assert err <= TOL, (norm, ref, err)
    a, b = _sumsq(params), _sumsq(params)
    assert a.dtype == torch.float64
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert abs(float(a) ** 0.5 - ref) / ref <= TOL


@pytest.mark.parametrize("k", [0, 2])
def test_standalone_clip(k):
    from picotron_amd.optim import clip_grad_norm_
    max_norm = 1.0
    params = _grad_list(10.0 ** (k - 2), seed=10 + k)
    before = [_grad_of(p).clone() for p in params]
    stale = [p.grad.clone() for p in params]
    ref = _norm64(params)
    assert ref > 2 * max_norm
    ret = clip_grad_norm_(params, max_norm, groups=())
    assert abs(float(ret) - ref) / ref <= TOL  # the pre-clip norm
    coef = ret._base[1]  # the device (norm, coefficient) pair behind the returned norm
    coef64 = max_norm / (ref + 1e-6)
    assert abs(float(coef) - coef64) / coef64 <= TOL + 2.0 ** -23, (float(coef), coef64)
    worst = 0
    for p, g0, st in zip(params, before, stale):
        g0b = _as_bf16(g0)
        want = (g0b.float() * coef).to(BF)
        got = _grad_of(p)
        if got.dtype == torch.float32:  # deferred main_grad: scaled in place to the bf16 form's value, .grad untouched
            assert torch.equal(got, want.float()), tuple(p.shape)
            assert torch.equal(p.grad, st)
            got = got.to(BF)
        else:
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), tuple(p.shape)
        want64 = (g0b.double() * coef64).to(BF)
        d = int((_ordered(got) - _ordered(want64)).abs().max())
        worst = max(worst, d)
        assert d <= 1, (tuple(p.shape), d)
    print(f"k={k} coef={float(coef):.9g} coef64={coef64:.9g} worst ulp vs fp64 clip={worst}")
    # the norm is now max_norm (each element rounded to bf16 once: 2**-9 relative at the most)
    assert abs(_norm64(params) - max_norm) <= 2.0 ** -8 * max_norm


def test_standalone_clip_below_max_norm_changes_nothing():
    from picotron_amd.optim import clip_grad_norm_
    params = _grad_list(1.0, seed=20)
    before = [_grad_of(p).clone() for p in params]
    ref = _norm64(params)
    ret = clip_grad_norm_(params, 4.0 * ref, groups=())
    assert float(ret._base[1]) == 1.0
    assert abs(float(ret) - ref) / ref <= TOL
    for p, g0 in zip(params, before):
        if g0.dtype == BF:
            assert torch.equal(_grad_of(p).view(torch.int16), g0.view(torch.int16))
        else:  # what a later deferred-cast step reads is unchanged
            assert torch.equal(_grad_of(p).to(BF), g0.to(BF))


SHAPES = [(2048,), (640, 256), (1000, 3), (7,), (65536 + 8,)]


def _twin_params(seed):
    torch.manual_seed(seed)
    base = [torch.randn(s, device="cuda").to(BF) for s in SHAPES]
    return [[torch.nn.Parameter(t.clone()) for t in base] for _ in range(2)]


def _set_grads(lists, mag, deferred_idx=None, unaligned=True, idle=()):
    """The same fresh gradients on every twin list (own copies); the last parameter's gradient is an unaligned
    view; `deferred_idx`: that parameter carries a deferred fp32 main_grad instead."""
    n = len(lists[0])
    for i in range(n):
        shape = lists[0][i].shape
        if i in idle:
            for ps in lists:
                ps[i].grad = None
            continue
        g32 = torch.randn(shape, device="cuda") * mag
        for ps in lists:
            p = ps[i]
            p._pico_grad_deferred = False
            if i == deferred_idx:
                p.grad = torch.full(shape, 3.0, device="cuda", dtype=BF)
                p._pico_grad_f32 = g32.clone()
                p._pico_grad_deferred = True
            elif unaligned and i == 0:
                big = torch.zeros(p.numel() + 1, device="cuda", dtype=BF)
                big[1:] = g32.to(BF).reshape(-1)
                p.grad = big[1:].view(shape)
            else:
                p.grad = g32.to(BF)


def _assert_same_state(o1, ps1, o2, ps2, what):
    for a, b in zip(ps1, ps2):
        assert torch.equal(a.detach().view(torch.int16), b.detach().view(torch.int16)), (what, tuple(a.shape))
        assert (a in o1.state) == (b in o2.state)
        if a in o1.state:
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(o1.state[a][key].view(torch.int16), o2.state[b][key].view(torch.int16)), \
                    (what, key, tuple(a.shape))
            assert float(o1.state[a]["step"]) == float(o2.state[b]["step"])


@pytest.mark.parametrize("deferred", [False, True])
def test_fused_equals_unfused(deferred):
    from picotron_amd.optim import AdamW, clip_grad_norm_
    m = 1.0
    fused, unfused = _twin_params(3)
    o1 = AdamW(fused, lr=1e-2, weight_decay=0.01, max_grad_norm=m)
    o2 = AdamW(unfused, lr=1e-2, weight_decay=0.01)
    clipped = []
    for step, mag in enumerate([1.0, 1e-4, 1.0]):  # norm ~ 480, 0.05, 480: across max_norm in both directions
        _set_grads([fused, unfused], mag, deferred_idx=1 if deferred else None)
        ref = _norm64(fused)
        clipped.append(ref > m)
        o1.step()
        ret = clip_grad_norm_(unfused, m, groups=())
        o2.step()
        assert torch.equal(o1.grad_norm, ret), (step, float(o1.grad_norm), float(ret))
        assert abs(float(ret) - ref) / ref <= TOL
        _assert_same_state(o1, fused, o2, unfused, step)
    assert clipped == [True, False, True]


def test_fused_with_huge_max_norm_is_the_plain_step():
    from picotron_amd.optim import AdamW
    a, b = _twin_params(4)
    o1 = AdamW(a, lr=3e-3, weight_decay=0.1, max_grad_norm=1e30)
    o2 = AdamW(b, lr=3e-3, weight_decay=0.1)
    for step, mag in enumerate([1.0, 1e-2, 100.0]):
        _set_grads([a, b], mag, deferred_idx=2)
        o1.step()
        o2.step()
        _assert_same_state(o1, a, o2, b, step)


def test_per_parameter_step_counts():
    """A parameter idles on one step (no gradient): the norm covers only the parameters that have one, and on the
    next step the two launches (two step counts) use one coefficient — the result is the unfused one's."""
    from picotron_amd.optim import AdamW, clip_grad_norm_
    m = 0.5
    fused, unfused = _twin_params(6)
    o1 = AdamW(fused, lr=1e-2, weight_decay=0.01, max_grad_norm=m)
    o2 = AdamW(unfused, lr=1e-2, weight_decay=0.01)
    for step in range(3):
        _set_grads([fused, unfused], 1.0, idle=(1,) if step == 1 else ())
        ref = _norm64(fused)
        o1.step()
        ret = clip_grad_norm_(unfused, m, groups=())
        o2.step()
        assert abs(float(o1.grad_norm) - ref) / ref <= TOL, step
        assert float(o1.grad_norm) == float(ret)
        _assert_same_state(o1, fused, o2, unfused, step)
    assert [float(o1.state[p]["step"]) for p in fused] == [3.0, 2.0, 3.0, 3.0, 3.0]
    assert len(o1._tables) >= 3  # the last step ran one launch per step count


def test_non_finite_gradient_skips_the_update():
    from picotron_amd.optim import AdamW, clip_grad_norm_
    (ps,) = _twin_params(7)[:1]
    opt = AdamW(ps, lr=1e-2, weight_decay=0.01, max_grad_norm=1.0)
    _set_grads([ps], 1.0)
    opt.step()
    assert bool(torch.isfinite(opt.grad_norm))
    snap = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]
    _set_grads([ps], 1.0)
    ps[2].grad.view(-1)[17] = float("inf")
    opt.step()
    assert float(opt.grad_norm) == float("inf")
    for p, (w, m1, m2) in zip(ps, snap):
        assert torch.equal(p.detach().view(torch.int16), w.view(torch.int16))
        assert torch.equal(opt.state[p]["exp_avg"].view(torch.int16), m1.view(torch.int16))
        assert torch.equal(opt.state[p]["exp_avg_sq"].view(torch.int16), m2.view(torch.int16))
    assert float(opt.state[ps[0]]["step"]) == 2.0  # documented: the host counter advances, it never reads the norm
    grads = [p.grad.clone() for p in ps]
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(ps, 1.0, error_if_nonfinite=True, groups=())
    assert float(clip_grad_norm_(ps, 1.0, groups=())) == float("inf")
    for p, g in zip(ps, grads):  # a non-finite norm leaves the gradients as they are
        assert torch.equal(p.grad.view(torch.int16), g.view(torch.int16))


def test_clipped_step_does_not_wait_on_the_host():
    from picotron_amd.optim import AdamW
    (ps,) = _twin_params(8)[:1]
    opt = AdamW(ps, lr=1e-2, max_grad_norm=1.0)
    _set_grads([ps], 1.0, deferred_idx=1)
    opt.step()  # warm-up: tables built and uploaded
    probe = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:  # pragma: no cover
        pytest.skip(f"torch.cuda.set_sync_debug_mode is not implemented on this build: {e}")
    try:
        try:
            probe.item()
            caught = False
        except RuntimeError:
            caught = True
        if caught:
            opt.step()
            opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not caught:
        pytest.skip("this ROCm build's sync debug mode does not flag a host read of a device value")
    assert float(opt.state[ps[0]]["step"]) == 3.0
    assert float(opt.grad_norm) > 1.0
