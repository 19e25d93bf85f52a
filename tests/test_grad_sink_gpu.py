"""Every fused weight-gradient producer of picotron_amd.ops under every gradient sink (picotron_amd/grad_sink.py):
where the gradient landed, whether the DataParallelBucket readiness callback fired, and every element of the
accumulated gradient against a reference, over three micro-batches with different inputs.

Shapes: 2 x 64 tokens (T = 128), hidden 256, 4 heads of D = 64, 2 KV heads, intermediate 128, vocab 512 — the
smallest at which every fused path dispatches. The DataParallelBucket half of the contract is faked with its three
attributes (main_grad, _pico_wgrad_sync, _pico_wgrad_ready) and W = 4: two non-syncing micro-batches, then a
syncing one, so main_grad must end as (dW1 + dW2 + dW3) / 4.

The reference of a GEMM producer is its own bf16 operands (recorded where the producer hands them to the wgrad GEMM;
for the LM head: the CE kernel's dlogits of the same logits GEMM), up-cast and multiplied with torch.matmul in fp32,
summed over the micro-batches in fp64; RMSNorm dw and the embedding scatter use tests/rowwise_ref.py's fp64
references. The bound of an element is derived by following the arithmetic of the path (class _Acc), nothing is tuned:
  * a product of reduction length n carries n 2^-24 cond, cond = (|dy|^T |x|) elementwise (fp32 accumulation);
  * every rounding to bf16 the path performs adds 2^-8 of the value it rounds (the running sum and what it already
    carries): the in-place forms round once per GEMM (the accumulator holds C + dy^T x before the one rounding), the
    forms that hand a bf16 dW to `grad += dW` (autograd, the hook path, separately allocated row-stacked gradients)
    twice, the fp32 main_grad forms not at all unless a bf16 dW is formed first (row-stacked parameters);
  * every fp32 accumulation into main_grad adds 2^-24 of the running sum; the 1/W = 1/4 scaling is exact.
Every element is checked.
"""
import pytest
import torch

import rowwise_ref as R
from picotron_amd import ops
from picotron_amd import wgrad_pair as WP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
B, S, H, NH, NKV, D, I, V = 2, 64, 256, 4, 2, 64, 128, 512
T = B * S
EPS = 1e-5
WORLD = 4
U16, U32 = 2.0 ** -8, 2.0 ** -24
CASES = ("fresh_grad", "separate", "hooked", "dp_main", "fusion_off")


def _rand(seed, *shape, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(BF).to(DEV)


def _param(seed, *shape, std=0.05, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.Parameter((torch.randn(*shape, generator=g) * std + mean).to(BF).to(DEV))


# ------------------------------------------------------------------------------------------ the bound
class _Acc:
    """The exact running sum S (fp64) of a gradient and the bound B on what the path's arithmetic may be off by."""

    def __init__(self, shape):
        self.S = torch.zeros(shape, dtype=torch.float64, device=DEV)
        self.B = torch.zeros(shape, dtype=torch.float64, device=DEV)

    def add(self, term):
        self.S = self.S + term[0]
        self.B = self.B + term[1]
        return self

    def round(self, u=U16):
        self.B = self.B + u * (self.S.abs() + self.B)
        return self

    def scale(self, s):  # a power of two: exact
        self.S, self.B = self.S * s, self.B * s

    def term(self):
        return self.S, self.B


def _gemm_term(dy2, x2):
    """(dy2^T x2 in fp32 from the bf16 operands, its fp32 accumulation bound K 2^-24 |dy2|^T |x2|)."""
    d = torch.matmul(dy2.float().t(), x2.float())
    c = torch.matmul(dy2.float().abs().t(), x2.float().abs())
    return d.double(), dy2.shape[0] * U32 * c.double()


def _rows(term, r0, n):
    return term[0][r0:r0 + n], term[1][r0:r0 + n]


# ------------------------------------------------------------------------------------------ the producers
class _Op:
    stacked = False  # several row-stacked parameters behind one GEMM: a bf16 dW exists before any `+=` into another buffer

    def __init__(self, rec):
        self.rec = rec  # the (params, dy2, x2) the producers handed to the wgrad GEMM, newest last

    def _stacked_terms(self):
        params, dy2, x2 = self.rec.pop()
        assert not self.rec
        term, out, r0 = _gemm_term(dy2, x2), {}, 0
        for name, p in self.P.items():
            assert any(p is q for q in params)
            out[name] = [_rows(term, r0, p.shape[0])]
            r0 += p.shape[0]
        return out


class _Linear(_Op):
    def __init__(self, rec):
        super().__init__(rec)
        self.P = {"w": _param(1, H, H)}

    def step(self, i):
        x = _rand(100 + i, B, S, H).requires_grad_()
        ops.linear(x, self.P["w"]).backward(_rand(200 + i, B, S, H))
        return self._stacked_terms()


class _GateUp(_Op):
    stacked = True

    def __init__(self, rec):
        super().__init__(rec)
        self.P = {"gate": _param(2, I, H), "up": _param(3, I, H)}

    def step(self, i):
        x = _rand(110 + i, B, S, H).requires_grad_()
        ops.gate_up_swiglu(x, self.P["gate"], self.P["up"]).backward(_rand(210 + i, B, S, I))
        return self._stacked_terms()


class _QKV(_Op):
    stacked = True

    def __init__(self, rec):
        super().__init__(rec)
        self.P = {"q": _param(4, NH * D, H), "k": _param(5, NKV * D, H), "v": _param(6, NKV * D, H)}
        ang = torch.arange(S, dtype=torch.float32)[:, None] * (10000.0 ** (-torch.arange(D // 2) / (D // 2)))[None]
        self.cos, self.sin = ang.cos().to(BF).to(DEV), ang.sin().to(BF).to(DEV)

    def step(self, i):
        x = _rand(120 + i, B, S, H).requires_grad_()
        o = ops.qkv_rope_attention(x, self.P["q"], self.P["k"], self.P["v"], self.cos, self.sin, NH, NKV, True)
        o.backward(_rand(220 + i, B, S, NH * D))
        return self._stacked_terms()


class _Norm(_Op):
    def __init__(self, rec):
        super().__init__(rec)
        self.P = {"w": _param(7, H, std=0.1, mean=1.0)}

    def step(self, i):
        x, dy = _rand(130 + i, B, S, H), _rand(230 + i, B, S, H)
        ops.rms_norm(x.clone().requires_grad_(), self.P["w"], EPS).backward(dy)
        x2, dy2, w = x.view(T, H), dy.view(T, H), self.P["w"].detach()
        rstd = R.ref_rmsnorm_fwd(x2, w, EPS)["rstd"][0]
        dw, cond = R.ref_rmsnorm_bwd(dy2, x2, w, rstd)["dw"]
        # T row terms summed in fp32, each the product dy (x rstd) of fp32 factors: 2 roundings, and an fp32 rstd
        # (a sum of H squares, rsqrt) within 4 ulps of the fp64 one used here
        return {"w": [(dw, (T + 8) * U32 * cond)]}


class _Embedding(_Op):
    def __init__(self, rec):
        super().__init__(rec)
        self.P = {"w": _param(8, V, H)}

    def step(self, i):
        ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(140 + i)).to(DEV)
        dy = _rand(240 + i, B, S, H)
        ops.embedding(ids, self.P["w"]).backward(dy)
        flat, dy2 = ids.reshape(-1), dy.view(T, H).double()
        acc = torch.zeros(V, H, dtype=torch.float64, device=DEV).index_add_(0, flat, dy2)
        cond = torch.zeros(V, H, dtype=torch.float64, device=DEV).index_add_(0, flat, dy2.abs())
        n = int(torch.bincount(flat, minlength=V).max())  # the longest run of one token: that many fp32 additions
        # PICO_WGRAD_FUSION=0 is F.embedding, whose backward is ATen's: it adds a token's rows into the bf16 dense
        # gradient in up to n steps, each rounding a partial sum of at most sum|dy| (pico_embedding_bwd rounds once)
        self.unfused = {"w": [(acc, n * U32 * cond + n * U16 * cond)]}
        return {"w": [(acc, n * U32 * cond)]}


class _LMHead(_Op):
    chunk = T

    def __init__(self, rec):
        super().__init__(rec)
        self.P = {"w": _param(9, V, H)}

    def step(self, i):
        x = _rand(150 + i, B, S, H)
        t = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(250 + i))
        t[0, 3 + i] = t[1, 40] = R.IGNORE
        t = t.to(DEV)
        w = self.P["w"]
        ops.lm_head_cross_entropy(x.clone().requires_grad_(), w, t, grad_scale=1 / 3, chunk=self.chunk).backward()
        x2, tt = x.view(T, H), t.reshape(-1)
        gscale = float(ops.ce_count(tt, R.IGNORE, 1 / 3)[1])
        terms = []
        for c0 in range(0, T, self.chunk):  # the producer's own sequence: logits GEMM, CE kernel in place, dW GEMM
            c1 = min(T, c0 + self.chunk)
            logits = torch.mm(x2[c0:c1], w.detach().t())
            dlogits = R.launch_ce_fwd_grad(logits, tt[c0:c1], gscale)["dlogits"]
            terms.append(_gemm_term(dlogits, x2[c0:c1]))
        return {"w": terms}


class _LMHeadRagged(_LMHead):
    chunk = 48  # 48 + 48 + 32 rows


OPS = {"linear": _Linear, "gate_up_swiglu": _GateUp, "qkv_rope_attention": _QKV, "rms_norm": _Norm,
       "embedding": _Embedding, "lm_head_ce": _LMHead, "lm_head_ce_chunk48": _LMHeadRagged}


@pytest.fixture
def recorded(monkeypatch):
    """The operands every projection hands to its wgrad GEMM (ops._wgrad_paired), cloned."""
    rec, orig = [], ops._wgrad_paired

    def spy(params, dy2, x2):
        rec.append((params, dy2.clone(), x2.clone()))
        return orig(params, dy2, x2)
    monkeypatch.setattr(ops, "_wgrad_paired", spy)
    return rec


def _fake_dp(P, state, calls):
    for name, p in P.items():
        p.main_grad = torch.zeros(p.shape, dtype=torch.float32, device=DEV)
        p._pico_wgrad_sync = lambda: (state["sync"], WORLD)
        p._pico_wgrad_ready = lambda name=name: calls.append(name)


def _adjacent(grads):
    r0 = 0
    for g in grads:
        if g.untyped_storage().data_ptr() != grads[0].untyped_storage().data_ptr() or \
                g.data_ptr() != grads[0].data_ptr() + r0 * g.element_size():
            return False
        r0 += g.numel()
    return True


def _handed_to_autograd(terms):
    """The bf16 tensor a producer hands back: one rounded product, or (chunked LM head) a bf16 buffer the chunks'
    GEMMs accumulated into, rounded once per chunk."""
    a = _Acc(terms[0][0].shape)
    for t in terms:
        a.add(t).round()
    return a.term()


def _check(tag, got, acc):
    assert bool(torch.isfinite(got).all()), tag
    err = (got.double() - acc.S).abs()
    ratio = err / (acc.B + R.TINY)
    i = int(ratio.argmax())
    print(f"SINK {tag} ratio {float(ratio.flatten()[i]):.3f} err {float(err.flatten()[i]):.3e} "
          f"ref {float(acc.S.flatten()[i]):.3e} at {i}")
    assert float(ratio.max()) <= 1.0, tag


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("op", list(OPS))
def test_producer_under_sink(monkeypatch, recorded, op, case):
    monkeypatch.setenv("PICO_WGRAD_FUSION", "0" if case == "fusion_off" else "1")
    o = OPS[op](recorded)
    P = o.P
    state, calls, handed = {"sync": False}, [], {n: [] for n in P}
    own = {}
    if case == "separate":
        for n, p in P.items():
            own[n] = p.grad = torch.zeros_like(p)
    if case in ("hooked", "fusion_off"):
        for n, p in P.items():
            p.register_hook(lambda g, n=n: handed[n].append(tuple(g.shape)))
    if case in ("dp_main", "fusion_off"):
        _fake_dp(P, state, calls)
    accs = {n: _Acc(p.shape) for n, p in P.items()}
    for i in range(3):
        state["sync"] = i == 2
        before = {n: p.main_grad.clone() for n, p in P.items()} if case == "dp_main" else None
        del calls[:]
        terms = o.step(i)
        if case == "fusion_off":
            terms = getattr(o, "unfused", terms)
        torch.cuda.synchronize()
        for n, p in P.items():
            a, ts = accs[n], terms[n]
            if case == "dp_main":
                # landed in main_grad, autograd got None, the bucket was told once
                assert p.grad is None and calls.count(n) == 1 and not torch.equal(p.main_grad, before[n]), (n, i)
                for t in ts:
                    a.add(_handed_to_autograd([t]) if o.stacked else t).round(U32)
                if state["sync"]:
                    a.scale(1.0 / WORLD)
                continue
            assert not calls, (n, i, calls)
            if case in ("hooked", "fusion_off"):  # autograd got one tensor and did `grad += dW` itself
                assert handed[n] == [tuple(p.shape)] * (i + 1), (n, i, handed[n])
                a.add(_handed_to_autograd(ts))
                if i:
                    a.round()
                continue
            assert handed[n] == []
            if i == 0 and case == "fresh_grad":
                own[n] = p.grad
            assert p.grad is own[n] and p.grad.data_ptr() == own[n].data_ptr(), (n, i)
            for t in ts:  # in place: the GEMM (or the dw / scatter kernel) rounds the updated sum once
                if case == "separate" and o.stacked:
                    a.add(_handed_to_autograd([t])).round()  # a bf16 dW, then grad.add_(dW)
                else:
                    a.add(t).round()
        if case == "fresh_grad" and o.stacked:  # the row blocks of one buffer
            assert _adjacent([p.grad for p in P.values()]), i
        if case == "separate" and o.stacked:
            assert not _adjacent([p.grad for p in P.values()])
        if case == "fusion_off":
            assert all(not bool(p.main_grad.any()) for p in P.values())
    for n, p in P.items():
        _check(f"{op} {case} {n}", p.main_grad if case == "dp_main" else p.grad, accs[n])


def test_deferred_micro_batch_still_marks_the_parameter(monkeypatch, recorded):
    """wgrad_pair groups of 2 over 3 micro-batches, a fake-DP linear whose x^T and dy sit in the group buffers:
    micro-batch 0 defers its GEMM (main_grad untouched) and still tells the bucket once, micro-batch 1 adds both
    with one GEMM over K = 2 T, micro-batch 2 (alone in its group, syncing) its own and the 1/W."""
    monkeypatch.setenv("PICO_WGRAD_FUSION", "1")
    monkeypatch.setenv("PICO_WGRAD_PAIR", "1")
    monkeypatch.setenv("PICO_WGRAD_GROUP", "2")
    w = _param(11, H, H)
    state, calls = {"sync": False}, []
    _fake_dp({"w": w}, state, calls)
    acc, stats0 = _Acc(w.shape), dict(WP.STATS)
    held = []
    try:
        for i in range(3):
            state["sync"] = i == 2
            del calls[:]
            before = w.main_grad.clone()
            with WP.micro_batch(i, 3):
                x = _rand(160 + i, B, S, H)
                xt = WP.xt_out(w, H, H, T, BF, torch.device(DEV))
                xt.copy_(x.view(T, H).t())
                x._pico_t = xt
                dy = WP.dy_out(w, H, H, T, BF, torch.device(DEV))
                dy.copy_(_rand(260 + i, T, H))
                ops.linear(x.requires_grad_(), w).backward(dy.view(B, S, H))
            torch.cuda.synchronize()
            assert calls == ["w"] and w.grad is None, (i, calls)
            held.append(recorded.pop()[1:])
            if i == 0:
                assert torch.equal(w.main_grad, before)
                continue
            assert not torch.equal(w.main_grad, before)
            dy2, x2 = (torch.cat([h[k] for h in held]) for k in (0, 1))  # one GEMM over the group's rows
            acc.add(_gemm_term(dy2, x2)).round(U32)
            held = []
        acc.scale(1.0 / WORLD)
        assert {k: WP.STATS[k] - stats0[k] for k in stats0} == {"deferred": 1, "paired": 1}
        _check("linear paired dp_main w", w.main_grad, acc)
    finally:
        WP.begin_step()
        WP.release()
