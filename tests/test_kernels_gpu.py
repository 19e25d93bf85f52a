"""Parity of the gfx950 kernels (through the C ABI) with the CPU oracle and the reference goldens.

Tolerances (bf16 outputs vs an fp64/fp32 oracle on the SAME bf16 inputs):
  * elementwise/norm kernels (one bf16 rounding): rel-L2 <= 4e-3 and max-abs within 2 bf16 ulps of
    the output magnitude, and never worse than the reference's own bf16 eager path (+1 ulp);
  * attention fwd: rel-L2 <= 4e-3; bwd (dq/dk/dv): rel-L2 <= 1e-2 (P and dS are bf16 MFMA operands,
    as in flash-attn) — the reference's bf16 eager SDPA error at these shapes is 3.4e-3 fwd;
  * LSE (fp32): max-abs <= 2e-3;
  * DP bucket kernels: bit-exact.
"""
import ctypes
import math

import pytest
import torch

from conftest import max_abs, rel_l2
from oracle import hotpath as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _ops():
    from picotron_amd import ops
    return ops


def _ulp_bound(ref, k=2.0):
    # k bf16 ulps of the largest magnitude (2^-8 relative spacing)
    return k * float(ref.abs().max()) * 2.0 ** -8


# ------------------------------------------------------------------------------------------ RMSNorm
def test_rmsnorm_golden(golden_kernels):
    ops = _ops()
    g = golden_kernels
    x = g["rms.x"].to(DEV).requires_grad_(True)
    w = g["rms.w"].to(DEV).requires_grad_(True)
    y = ops.rms_norm(x, w, 1e-5)
    yref = g["rms.y_f64"]
    assert rel_l2(y.cpu(), yref) < 4e-3
    eager_err = max_abs(g["rms.y_eager_bf16"], yref)
    assert max_abs(y.detach().cpu(), yref) <= eager_err + _ulp_bound(yref, 1)
    y.backward(g["rms.dy"].to(DEV).to(BF))
    dx, dw = H.rmsnorm_grads(g["rms.x"], g["rms.w"], 1e-5, g["rms.dy"].to(BF).double())
    assert rel_l2(x.grad.cpu(), dx) < 4e-3
    assert rel_l2(w.grad.cpu(), dw) < 4e-3


@pytest.mark.parametrize("rows,cols", [(1, 64), (7, 128), (4096, 2048), (333, 4096), (5, 8192), (64, 1000 * 8)])
def test_rmsnorm_shapes(rows, cols):
    ops = _ops()
    torch.manual_seed(rows + cols)
    x = torch.randn(rows, cols, dtype=BF, device=DEV) * 3
    w = (1 + 0.1 * torch.randn(cols, device=DEV)).to(BF)
    y = ops.rms_norm(x, w, 1e-5)
    yref, _ = H.rmsnorm_fused(x.cpu().double(), w.cpu().double(), 1e-5)
    assert rel_l2(y.cpu(), yref) < 4e-3
    assert max_abs(y.cpu(), yref) <= _ulp_bound(yref, 2)
    if cols <= 4096:
        xr = x.clone().requires_grad_(True)
        wr = w.clone().requires_grad_(True)
        dy = torch.randn(rows, cols, dtype=BF, device=DEV)
        ops.rms_norm(xr, wr, 1e-5).backward(dy)
        dx, dw = H.rmsnorm_grads(x.cpu(), w.cpu(), 1e-5, dy.cpu().double())
        assert rel_l2(xr.grad.cpu(), dx) < 4e-3
        assert rel_l2(wr.grad.cpu(), dw) < 4e-3


@pytest.mark.parametrize("rows,cols", [(512, 2048), (512, 4096), (5000, 2048)])
def test_rmsnorm_chained_dw(monkeypatch, rows, cols):
    """Three stacked norms accumulating into persistent bf16 .grad (dw_mode 1): the first two weight gradients
    are reduced inside the NEXT norm's backward launch, the last by the end-of-backward callback
    (pico_rmsnorm_bwd_chain / pico_rmsnorm_dw_reduce). Same values as the one-launch-per-reduction path (same
    partial rows, fixed-order sums: within one bf16 rounding) and as the fp64 restatement, over two backward
    passes (the second accumulates into the first's .grad). 5000 rows: the full 256-workgroup grid, two
    passes of the row loop with a ragged second pass (some waves own one row, some none)."""
    ops = _ops()
    torch.manual_seed(cols)
    x0 = torch.randn(rows, cols, dtype=BF, device=DEV) * 2
    ws = [(1 + 0.1 * torch.randn(cols, device=DEV)).to(BF) for _ in range(3)]
    dys = [torch.randn(rows, cols, dtype=BF, device=DEV) for _ in range(2)]

    def run(chain):
        monkeypatch.setenv("PICO_NORM_DW_CHAIN", "1" if chain else "0")
        params = [w.clone().requires_grad_(True) for w in ws]
        for p in params:
            p.grad = torch.zeros_like(p)  # persistent bf16 grads: the in-place accumulation modes
        xs = []
        for dy in dys:
            x = x0.clone().requires_grad_(True)
            h = x
            for p in params:
                h = ops.rms_norm(h, p, 1e-5)
            h.backward(dy)
            xs.append(x.grad)
        torch.cuda.synchronize()
        assert not ops._NORM_PENDING, "a chained dw reduction was left pending after backward"
        return [p.grad.float().cpu() for p in params], [g.float().cpu() for g in xs]

    g_chain, dx_chain = run(True)
    g_plain, dx_plain = run(False)
    for a, b in zip(dx_chain, dx_plain):
        assert torch.equal(a, b)  # the data path is untouched
    for a, b in zip(g_chain, g_plain):
        assert max_abs(a, b) <= _ulp_bound(b.double(), 1), max_abs(a, b)
    # fp64 restatement of the stack's weight gradients, summed over the two passes
    ref = [torch.zeros(cols, dtype=torch.float64) for _ in range(3)]
    for dy in dys:
        hs = [x0.cpu().double()]
        for w in ws[:-1]:
            hs.append(H.rmsnorm_fused(hs[-1].to(BF).double(), w.cpu().double(), 1e-5)[0].to(BF).double())
        g = dy.cpu().double()
        for i in (2, 1, 0):
            dxi, dwi = H.rmsnorm_grads(hs[i].to(BF), ws[i].cpu(), 1e-5, g)
            ref[i] += dwi.double()
            g = dxi.to(BF).double()
    for a, r in zip(g_chain, ref):
        assert rel_l2(a, r) < 1e-2


@pytest.mark.parametrize("reentrant", [False, True])
def test_rmsnorm_chained_dw_under_checkpoint(reentrant):
    """a norm forward that runs INSIDE a backward pass (activation recompute by
    torch.utils.checkpoint) must not drop the chained weight gradient another norm of that pass left pending.
    Three stacked norms with persistent .grad (chained dw), the middle one checkpointed: weight gradients equal
    the run without checkpointing."""
    from torch.utils.checkpoint import checkpoint
    ops = _ops()
    torch.manual_seed(11)
    rows, cols = 512, 2048
    x0 = torch.randn(rows, cols, dtype=BF, device=DEV) * 2
    ws = [(1 + 0.1 * torch.randn(cols, device=DEV)).to(BF) for _ in range(3)]
    dy = torch.randn(rows, cols, dtype=BF, device=DEV)

    def run(ckpt):
        params = [w.clone().requires_grad_(True) for w in ws]
        for p in params:
            p.grad = torch.zeros_like(p)
        x = x0.clone().requires_grad_(True)
        h = ops.rms_norm(x, params[0], 1e-5)
        if ckpt:
            h = checkpoint(lambda t: ops.rms_norm(t, params[1], 1e-5), h, use_reentrant=reentrant)
        else:
            h = ops.rms_norm(h, params[1], 1e-5)
        h = ops.rms_norm(h, params[2], 1e-5)
        h.backward(dy)
        torch.cuda.synchronize()
        assert not ops._NORM_PENDING
        return [p.grad.float().cpu() for p in params], x.grad.float().cpu()

    g_ref, dx_ref = run(False)
    g_ck, dx_ck = run(True)
    assert torch.equal(dx_ck, dx_ref)
    for a, b in zip(g_ck, g_ref):
        assert max_abs(a, b) <= _ulp_bound(b.double(), 1), max_abs(a, b)


def test_rmsnorm_residual_prenorm():
    ops = _ops()
    torch.manual_seed(1)
    x = torch.randn(64, 2048, dtype=BF, device=DEV, requires_grad=True)
    r = torch.randn(64, 2048, dtype=BF, device=DEV, requires_grad=True)
    w = (1 + 0.1 * torch.randn(2048, device=DEV)).to(BF).requires_grad_(True)
    y, res = ops.layer_norm_fn(x, w, None, residual=r, eps=1e-5, prenorm=True, is_rms_norm=True)
    yref, xe = H.rmsnorm_fused(x.detach().cpu(), w.detach().cpu(), 1e-5, residual=r.detach().cpu())
    assert torch.equal(res.cpu(), xe)  # residual_out = bf16(x + r), bit-exact
    assert max_abs(y.detach().cpu(), yref.double()) <= _ulp_bound(yref.double(), 1)
    dy = torch.randn_like(y)
    dres = torch.randn_like(res)
    torch.autograd.backward([y, res], [dy, dres])
    dxe, dw = H.rmsnorm_grads(xe, w.detach().cpu(), 1e-5, dy.cpu().double())
    assert rel_l2(x.grad.cpu(), dxe + dres.cpu().double()) < 4e-3
    assert torch.equal(x.grad, r.grad)


def test_rmsnorm_dw_accumulate_modes():
    """pico_rmsnorm_bwd_acc: mode 2 (fp32 (g + dw) * scale) with g = 0, scale = 1 gives the fp32 dw sum;
    mode 1 == bf16(g_bf16 + that sum) and mode 2 == (g + sum) * scale bit for bit; dx identical in every
    mode; mode 0 == pico_rmsnorm_bwd."""
    import ctypes  # noqa: F401
    from picotron_amd import _lib as L
    torch.manual_seed(3)
    rows, cols = 300, 2048
    x = torch.randn(rows, cols, dtype=BF, device=DEV)
    w = (1 + 0.1 * torch.randn(cols, device=DEV)).to(BF)
    dy = torch.randn(rows, cols, dtype=BF, device=DEV)
    rstd = torch.rsqrt(x.float().pow(2).mean(1) + 1e-5)
    lib = L.load()
    ws = torch.empty(lib.pico_rmsnorm_bwd_workspace_bytes(rows, cols), dtype=torch.uint8, device=DEV)

    def run(mode, target, scale=1.0):
        dx = torch.empty_like(x)
        L.check(lib.pico_rmsnorm_bwd_acc(L.ptr(dy), None, L.ptr(x), L.ptr(w), L.ptr(rstd), L.ptr(dx), L.ptr(target),
                                         mode, scale, L.ptr(ws), rows, cols, L.stream_of(x)), "bwd_acc")
        torch.cuda.synchronize()
        return dx
    s32 = torch.zeros(cols, device=DEV)
    dx2 = run(2, s32)
    g1 = torch.randn(cols, device=DEV).to(BF)
    exp1 = (g1.float() + s32).to(BF)
    dx1 = run(1, g1)
    assert torch.equal(g1, exp1)
    g2 = torch.randn(cols, device=DEV)
    exp2 = (g2 + s32) * 0.25
    run(2, g2, 0.25)
    assert torch.equal(g2, exp2)
    d0 = torch.empty(cols, dtype=BF, device=DEV)
    dx0 = run(0, d0)
    assert torch.equal(d0, s32.to(BF))
    assert torch.equal(dx0, dx1) and torch.equal(dx0, dx2)
    d_ref = torch.empty(cols, dtype=BF, device=DEV)
    dxr = torch.empty_like(x)
    L.check(lib.pico_rmsnorm_bwd(L.ptr(dy), None, L.ptr(x), L.ptr(w), L.ptr(rstd), L.ptr(dxr), L.ptr(d_ref),
                                 L.ptr(ws), rows, cols, L.stream_of(x)), "bwd")
    torch.cuda.synchronize()
    assert torch.equal(d_ref, d0) and torch.equal(dxr, dx0)


def test_rmsnorm_rejects_cpu_tensors():
    ops = _ops()
    with pytest.raises(RuntimeError):
        ops.rms_norm(torch.randn(4, 64, dtype=BF), torch.ones(64, dtype=BF))


# ------------------------------------------------------------------------------------------ RoPE
def test_rope_golden(golden_kernels):
    ops = _ops()
    g = golden_kernels
    cos, sin = g["rope.cos"].to(DEV), g["rope.sin"].to(DEV)
    q = g["rope.q"].transpose(1, 2).contiguous().to(DEV).requires_grad_(True)  # [B,S,H,D]
    out = ops.apply_rotary_emb(q, cos[:, :32], sin[:, :32])
    ref = g["rope.out_f64"].transpose(1, 2)
    assert rel_l2(out.detach().cpu(), ref) < 4e-3
    assert max_abs(out.detach().cpu(), ref) <= max_abs(g["rope.out_eager_bf16"], g["rope.out_f64"]) + _ulp_bound(ref, 1)
    out.backward(g["rope.dy"].transpose(1, 2).to(DEV).to(BF))
    assert rel_l2(q.grad.cpu(), g["rope.dx_f64"].transpose(1, 2)) < 4e-3


@pytest.mark.parametrize("B,S,NH,D", [(4, 1024, 32, 64), (1, 100, 3, 128), (2, 37, 8, 64)])
def test_rope_shapes_and_strides(B, S, NH, D):
    ops = _ops()
    torch.manual_seed(S)
    cos, sin = H.get_cos_sin(S, D, base=10000.0)
    big = torch.randn(B, S, NH + 2, D, dtype=BF, device=DEV)
    x = big[:, :, 1:NH + 1]  # non-contiguous head slice (row stride (NH+2)*D)
    out = ops.apply_rotary_emb(x, cos.to(DEV)[:, : D // 2], sin.to(DEV)[:, : D // 2])
    ref = H.rope_fused(x.cpu().double(), cos.double(), sin.double())
    assert rel_l2(out.cpu(), ref) < 4e-3
    assert max_abs(out.cpu(), ref) <= _ulp_bound(ref, 2)
    # inplace=True rotates out of place and copies the result back: the kernel never sees out == x here
    y = x.clone()
    ops.apply_rotary_emb(y, cos.to(DEV)[:, : D // 2], sin.to(DEV)[:, : D // 2], inplace=True)
    assert torch.equal(y, out)
    # the truly aliased launch (out == x, both the strided head slice), as the fused qkv path issues it
    big2 = big.clone()
    z = big2[:, :, 1:NH + 1]
    ops._rope_launch(z, z, cos.to(DEV)[:, : D // 2], sin.to(DEV)[:, : D // 2], False)
    assert torch.equal(z, out)
    assert torch.equal(big2[:, :, 0], big[:, :, 0]) and torch.equal(big2[:, :, NH + 1], big[:, :, NH + 1])


# ------------------------------------------------------------------------------------------ SwiGLU
def test_swiglu_golden(golden_kernels):
    ops = _ops()
    g = golden_kernels
    gg = g["swiglu.g"].to(DEV).requires_grad_(True)
    uu = g["swiglu.u"].to(DEV).requires_grad_(True)
    h = ops.swiglu(gg, uu)
    ref = g["swiglu.h_f64"]
    assert rel_l2(h.detach().cpu(), ref) < 4e-3
    assert max_abs(h.detach().cpu(), ref) <= max_abs(g["swiglu.h_eager_bf16"], ref) + _ulp_bound(ref, 1)
    h.backward(g["swiglu.dh"].to(DEV).to(BF))
    dg, du = H.swiglu_grads(g["swiglu.g"], g["swiglu.u"], g["swiglu.dh"].to(BF))
    assert rel_l2(gg.grad.cpu(), dg) < 4e-3 and rel_l2(uu.grad.cpu(), du) < 4e-3


@pytest.mark.parametrize("n", [1, 7, 8, 4096 * 8192 // 16, 12345])
def test_swiglu_sizes(n):
    ops = _ops()
    torch.manual_seed(n)
    g = torch.randn(n, dtype=BF, device=DEV) * 2
    u = torch.randn(n, dtype=BF, device=DEV)
    h = ops.swiglu(g, u)
    ref = H.swiglu(g.cpu().double(), u.cpu().double())
    assert rel_l2(h.cpu(), ref) < 4e-3


# ------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("tag", ["causal", "full"])
def test_attention_golden(golden_kernels, tag):
    ops = _ops()
    g = golden_kernels
    p = lambda n: g[f"attn.{tag}.{n}"]
    to = lambda t: t.to(BF).transpose(1, 2).contiguous().to(DEV)  # [B,H,S,D] fp32 -> [B,S,H,D] bf16
    q, k, v = to(p("q")), to(p("k")), to(p("v"))
    sc = 1.0 / math.sqrt(64)
    o, lse = ops.attention_block_fwd(q, k, v, sc, tag == "causal")
    # oracle on the same bf16-rounded inputs
    qb, kb, vb = [p(n).to(BF).double() for n in ("q", "k", "v")]
    O, L = H.attention_fwd(qb, kb, vb, sc, tag == "causal")
    assert rel_l2(o.transpose(1, 2).cpu(), O) < 4e-3
    assert max_abs(lse.cpu(), L) < 2e-3
    assert rel_l2(o.transpose(1, 2).cpu(), p("o")) < 1e-2  # vs the reference's fp32 output
    do = to(p("do"))
    dq, dk, dv = ops.attention_block_bwd(do, q, k, v, o, lse, sc, tag == "causal")
    dQ, dK, dV = H.attention_bwd(p("do").to(BF).double(), qb, kb, vb, o.transpose(1, 2).cpu().double(),
                                 lse.cpu().double(), sc, tag == "causal")
    for a, b in ((dq, dQ), (dk, dK), (dv, dV)):
        assert rel_l2(a.transpose(1, 2).cpu(), b) < 1e-2


CASES = [
    # B, Sq, Sk, Hq, Hkv, D, causal
    (1, 128, 128, 2, 2, 64, True),
    (2, 1024, 1024, 4, 4, 64, True),   # C2 geometry slice
    (1, 257, 257, 4, 2, 64, True),     # ragged + GQA 2
    (1, 1000, 1000, 8, 2, 128, True),  # D=128, GQA 4, ragged
    (2, 96, 200, 4, 4, 64, False),     # cross lengths, non-causal
    (1, 300, 77, 2, 1, 128, False),
    (1, 1, 1, 1, 1, 64, True),
]


@pytest.mark.parametrize("B,Sq,Sk,Hq,Hkv,D,causal", CASES)
def test_attention_vs_oracle(B, Sq, Sk, Hq, Hkv, D, causal):
    ops = _ops()
    torch.manual_seed(Sq * 7 + Sk + D)
    q = torch.randn(B, Sq, Hq, D, dtype=BF, device=DEV)
    k = torch.randn(B, Sk, Hkv, D, dtype=BF, device=DEV)
    v = torch.randn(B, Sk, Hkv, D, dtype=BF, device=DEV)
    do = torch.randn(B, Sq, Hq, D, dtype=BF, device=DEV)
    sc = 1.0 / math.sqrt(D)
    o, lse = ops.attention_block_fwd(q, k, v, sc, causal)
    qd, kd, vd = [t.transpose(1, 2).cpu().double() for t in (q, k, v)]
    O, L = H.attention_fwd(qd, kd, vd, sc, causal)
    assert rel_l2(o.transpose(1, 2).cpu(), O) < 4e-3
    assert max_abs(lse.cpu(), L) < 2e-3
    dq, dk, dv = ops.attention_block_bwd(do, q, k, v, o, lse, sc, causal)
    dQ, dK, dV = H.attention_bwd(do.transpose(1, 2).cpu().double(), qd, kd, vd, o.transpose(1, 2).cpu().double(),
                                 lse.cpu().double(), sc, causal)
    assert rel_l2(dq.transpose(1, 2).cpu(), dQ) < 1e-2
    assert rel_l2(dk.transpose(1, 2).cpu(), dK) < 1e-2
    assert rel_l2(dv.transpose(1, 2).cpu(), dV) < 1e-2


@pytest.mark.parametrize("B,Hq,Hkv", [(8, 64, 8), (4, 32, 8)])
def test_attention_gqa_head_split(B, Hq, Hkv):
    """Small grids whose key blocks split their (query head, query tile) list over 2 or 4 workgroups (GQA 64/8 at B 8, 32/8 at B 4:
    fp32 dK/dV partials + attn_bwd_dkv_kernel) vs an fp32 torch reference on the GPU, causal S = 1024."""
    ops = _ops()
    torch.manual_seed(B * Hq + Hkv)
    S, D = 1024, 64
    q = torch.randn(B, S, Hq, D, dtype=BF, device=DEV)
    k = torch.randn(B, S, Hkv, D, dtype=BF, device=DEV)
    v = torch.randn(B, S, Hkv, D, dtype=BF, device=DEV)
    do = torch.randn(B, S, Hq, D, dtype=BF, device=DEV)
    sc = 1.0 / math.sqrt(D)
    o, lse = ops.attention_block_fwd(q, k, v, sc, True)
    dq, dk, dv = ops.attention_block_bwd(do, q, k, v, o, lse, sc, True)
    G = Hq // Hkv
    qf, kf, vf, dof = [t.float().transpose(1, 2).requires_grad_(True) for t in (q, k, v, do)]
    kr, vr = kf.repeat_interleave(G, 1), vf.repeat_interleave(G, 1)
    s = (qf @ kr.transpose(-1, -2)) * sc
    s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool, device=DEV), 1), float("-inf"))
    out = torch.softmax(s, -1) @ vr
    gq, gk, gv = torch.autograd.grad(out, (qf, kf, vf), dof.detach())
    assert rel_l2(o.transpose(1, 2).float(), out.detach()) < 4e-3
    assert rel_l2(dq.transpose(1, 2).float(), gq) < 1e-2
    assert rel_l2(dk.transpose(1, 2).float(), gk) < 1e-2
    assert rel_l2(dv.transpose(1, 2).float(), gv) < 1e-2


@pytest.mark.parametrize("S,Hq,Hkv,causal,mode", [(2300, 2, 2, True, "bf16"), (2304, 4, 2, False, "bf16"),
                                                   (2300, 2, 1, True, "f32acc"), (2304, 2, 2, True, "rope"),
                                                   (2304, 64, 64, True, "rope")])  # one workgroup per key block: dK RoPE^-1 in its epilogue
def test_attention_bwd_d128_key_block_groups(S, Hq, Hkv, causal, mode):
    """head_dim 128 at 18 key blocks of 128 keys (the name is from a fused backward that ran such lengths in key-block
    groups; pico_attn_bwd always takes the split path now). By attn_bwd_plan.h at 256 CUs the four B 1 cases have
    36 or 18 key blocks for 256 slots, so each key block's tile list is split 8 ways (hsplit 8: fp32 partials summed
    and, in the rope case, rotated by attn_bwd_dkv_kernel); the 64-head case runs the plain grid of 1152 workgroups
    with hsplit 1 (18 blocks are more than its 4 groups hold), dK rotated in the kernel's epilogue, and a dQ front
    of 10 blocks. vs an fp32 torch reference: bf16 dQ, the caller's fp32 accumulator (ring mode), the fused
    RoPE^-1."""
    from picotron_amd.model import get_cos_sin
    ops = _ops()
    torch.manual_seed(S + Hq + Hkv)
    B, D = 1, 128
    q, do = [torch.randn(B, S, Hq, D, dtype=BF, device=DEV) for _ in range(2)]
    k, v = [torch.randn(B, S, Hkv, D, dtype=BF, device=DEV) for _ in range(2)]
    sc = 1.0 / math.sqrt(D)
    o, lse = ops.attention_block_fwd(q, k, v, sc, causal)
    assert -(-S // 256) > 8  # grouped (the bound itself: tests/test_abi.py::test_workspace_sizes)
    G = Hq // Hkv
    qf, kf, vf = [t.float().transpose(1, 2).requires_grad_(True) for t in (q, k, v)]
    kr, vr = kf.repeat_interleave(G, 1), vf.repeat_interleave(G, 1)
    sm = (qf @ kr.transpose(-1, -2)) * sc
    if causal:
        sm = sm.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool, device=DEV), 1), float("-inf"))
    out = torch.softmax(sm, -1) @ vr
    gq, gk, gv = torch.autograd.grad(out, (qf, kf, vf), do.float().transpose(1, 2))
    gq, gk, gv = (t.transpose(1, 2) for t in (gq, gk, gv))
    if mode == "bf16":
        dq, dk, dv = ops.attention_block_bwd(do, q, k, v, o, lse, sc, causal)
        dq = dq.float()
    elif mode == "f32acc":
        dq = torch.full(q.shape, 0.25, dtype=torch.float32, device=DEV)
        _, dk, dv = ops.attention_block_bwd(do, q, k, v, o, lse, sc, causal, dq_accum=dq)
        dq = dq - 0.25
    else:
        cos, sin = get_cos_sin(S, D, base=10000.0)
        cos, sin = cos.to(DEV, BF)[:, : D // 2], sin.to(DEV, BF)[:, : D // 2]
        dq, dk, dv = [torch.empty_like(t) for t in (q, k, v)]
        ops._attention_bwd_into(do, q, k, v, o, lse, sc, causal, dq, dk, dv, rope=(cos, sin))
        rq, rk = torch.empty_like(q), torch.empty_like(k)
        ops._rope_launch(gq.to(BF).contiguous(), rq, cos, sin, True)
        ops._rope_launch(gk.to(BF).contiguous(), rk, cos, sin, True)
        gq, gk = rq.float(), rk.float()
        dq = dq.float()
    assert rel_l2(dq, gq) < 1e-2
    assert rel_l2(dk.float(), gk) < 1e-2
    assert rel_l2(dv.float(), gv) < 1e-2


@pytest.mark.parametrize("B,Sq,Sk,Hq,Hkv,causal,mode", [
    (2, 1024, 1024, 8, 8, True, "bf16"),     # C2 slice: 128 key blocks for 512 slots, plain grid with hsplit 4
    (1, 1000, 1000, 8, 2, True, "bf16"),     # ragged, GQA 4 (hsplit 8)
    (4, 1024, 1024, 32, 8, True, "bf16"),    # GQA 4 at a small grid: key blocks split over workgroups (hsplit 2)
    (1, 1536, 1536, 4, 4, True, "rope"),     # the causal default's last length, fused RoPE^-1
    (1, 2049, 2049, 2, 2, True, "f32acc"),   # past it (default: the 32-row kernel), caller's fp32 dQ
    (1, 2048, 2048, 4, 4, False, "bf16"),    # non-causal 2048: the 8-wave default
    (2, 96, 200, 4, 4, False, "bf16"),       # cross lengths, non-causal
    (1, 640, 640, 4, 4, False, "rope"),
])
def test_attention_bwd_d64_kv_kernels(monkeypatch, B, Sq, Sk, Hq, Hkv, causal, mode):
    """D = 64 dK/dV: attn_bwd_kvp_kernel (64-row query tiles, 4 or 8 waves x 32 keys per workgroup: the default up
    to 4096 keys) and the 32-row attn_bwd_kv_kernel (pico_select PICO_SEL_ATTN_KVP / PICO_SEL_KVP_WAVES force each), each
    with its matching dQ-kernel LSE form, vs an fp32 torch reference, and within bf16 rounding of each other."""
    _check_kv_kernels(64, ("0", "1", "1w8"), B, Sq, Sk, Hq, Hkv, causal, mode)


@pytest.mark.parametrize("B,Sq,Sk,Hq,Hkv,causal,mode", [
    (4, 1024, 1024, 16, 16, True, "bf16"),   # C4 per tp-2 rank (Llama-2-7B), micro-batch 4: 4 block groups
    (1, 1000, 1000, 8, 2, True, "bf16"),     # ragged, GQA 4, key blocks split over workgroups (hsplit 8)
    (2, 1024, 1024, 32, 8, True, "rope"),    # GQA 4, fused RoPE^-1
    (1, 520, 520, 4, 4, True, "f32acc"),     # caller's fp32 dQ
    (2, 96, 200, 4, 4, False, "bf16"),       # cross lengths, non-causal
    (1, 640, 640, 4, 4, False, "rope"),
])
def test_attention_bwd_d128_kv_kernels(B, Sq, Sk, Hq, Hkv, causal, mode):
    """D = 128 dK/dV: attn_bwd_kvp128_kernel (64-row query tiles in halves, one wave per SIMD: the default) and the
    32-row attn_bwd_kv_kernel<128> (pico_select PICO_SEL_ATTN_KVP 0), each with its dQ-kernel LSE form, vs an fp32
    torch reference and within bf16 rounding of each other."""
    _check_kv_kernels(128, ("0", "1"), B, Sq, Sk, Hq, Hkv, causal, mode)


def _check_kv_kernels(D, variants, B, Sq, Sk, Hq, Hkv, causal, mode):
    from picotron_amd.model import get_cos_sin
    ops = _ops()
    torch.manual_seed(Sq * 3 + Sk + Hq + Hkv + D)
    q, do = [torch.randn(B, Sq, Hq, D, dtype=BF, device=DEV) for _ in range(2)]
    k, v = [torch.randn(B, Sk, Hkv, D, dtype=BF, device=DEV) for _ in range(2)]
    sc = 1.0 / math.sqrt(D)
    o, lse = ops.attention_block_fwd(q, k, v, sc, causal)
    G = Hq // Hkv
    qf, kf, vf = [t.float().transpose(1, 2).requires_grad_(True) for t in (q, k, v)]
    kr, vr = kf.repeat_interleave(G, 1), vf.repeat_interleave(G, 1)
    sm = (qf @ kr.transpose(-1, -2)) * sc
    if causal:
        sm = sm.masked_fill(torch.triu(torch.ones(Sq, Sk, dtype=torch.bool, device=DEV), 1 + Sk - Sq), float("-inf"))
    out = torch.softmax(sm, -1) @ vr
    gq, gk, gv = torch.autograd.grad(out, (qf, kf, vf), do.float().transpose(1, 2))
    gq, gk, gv = (t.transpose(1, 2) for t in (gq, gk, gv))
    cos = sin = None
    if mode == "rope":
        cos, sin = get_cos_sin(max(Sq, Sk), D, base=10000.0)
        cos, sin = cos.to(DEV, BF)[:, : D // 2], sin.to(DEV, BF)[:, : D // 2]
        rq, rk = torch.empty_like(q), torch.empty_like(k)
        ops._rope_launch(gq.to(BF).contiguous(), rq, cos, sin, True)
        ops._rope_launch(gk.to(BF).contiguous(), rk, cos, sin, True)
        gq, gk = rq.float(), rk.float()
    res = {}
    from picotron_amd import _lib as L
    for kvp in variants:
        L.select(L.SEL_ATTN_KVP, int(kvp[0]))
        L.select(L.SEL_KVP_WAVES, 8 if kvp.endswith("w8") else 4)
        if mode == "bf16":
            dq, dk, dv = ops.attention_block_bwd(do, q, k, v, o, lse, sc, causal)
        elif mode == "f32acc":
            dq = torch.full(q.shape, 0.25, dtype=torch.float32, device=DEV)
            _, dk, dv = ops.attention_block_bwd(do, q, k, v, o, lse, sc, causal, dq_accum=dq)
            dq = dq - 0.25
        else:
            dq, dk, dv = [torch.empty_like(t) for t in (q, k, v)]
            ops._attention_bwd_into(do, q, k, v, o, lse, sc, causal, dq, dk, dv, rope=(cos, sin))
        torch.cuda.synchronize()
        L.select(L.SEL_ATTN_KVP, L.SEL_AUTO)
        L.select(L.SEL_KVP_WAVES, L.SEL_AUTO)
        res[kvp] = [t.float() for t in (dq, dk, dv)]
        for a, b in zip(res[kvp], (gq, gk, gv)):
            assert rel_l2(a, b) < 1e-2, (kvp, rel_l2(a, b))
    for other in variants[1:]:
        for a, b in zip(res["0"], res[other]):
            assert rel_l2(a, b) < 8e-3


def test_attention_dq_f32_accumulate():
    ops = _ops()
    torch.manual_seed(3)
    q, k, v, do = [torch.randn(1, 256, 2, 64, dtype=BF, device=DEV) for _ in range(4)]
    o, lse = ops.attention_block_fwd(q, k, v, 0.125, True)
    dq_bf, _, _ = ops.attention_block_bwd(do, q, k, v, o, lse, 0.125, True)
    acc = torch.full(q.shape, 0.5, dtype=torch.float32, device=DEV)
    ops.attention_block_bwd(do, q, k, v, o, lse, 0.125, True, dq_accum=acc)
    assert rel_l2((acc - 0.5).cpu(), dq_bf.float().cpu()) < 4e-3


def test_attention_strided_bhsd_views():
    """The reference hands flash-attn k/v as [B,S,H,D] views of BHSD tensors (ref model.py:33-35)."""
    ops = _ops()
    torch.manual_seed(5)
    q = torch.randn(2, 4, 128, 64, dtype=BF, device=DEV)
    k = torch.randn(2, 4, 128, 64, dtype=BF, device=DEV)
    v = torch.randn(2, 4, 128, 64, dtype=BF, device=DEV)
    o1 = ops.flash_attn_func(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), causal=True)
    o2 = ops.flash_attn_func(q.transpose(1, 2).contiguous(), k.transpose(1, 2).contiguous(),
                             v.transpose(1, 2).contiguous(), causal=True)
    assert torch.equal(o1, o2)


def test_attention_softmax_rescale_branch():
    """A spiked key forces the running max to jump mid-sweep (rule 26)."""
    ops = _ops()
    torch.manual_seed(9)
    q = torch.randn(1, 512, 2, 64, dtype=BF, device=DEV)
    k = torch.randn(1, 512, 2, 64, dtype=BF, device=DEV)
    v = torch.randn(1, 512, 2, 64, dtype=BF, device=DEV)
    k[:, 300] = q[:, 400] * 4  # row 400 sees a huge score at key 300 (tile 4 of 8)
    o, lse = ops.attention_block_fwd(q, k, v, 0.125, True)
    O, L = H.attention_fwd(*[t.transpose(1, 2).cpu().double() for t in (q, k, v)], 0.125, True)
    assert rel_l2(o.transpose(1, 2).cpu(), O) < 4e-3
    assert max_abs(o.transpose(1, 2).cpu(), O) < 2e-2


# ------------------------------------------------------------------------------------------ ring merge
def test_merge_golden(golden_kernels):
    """update_out_and_lse with the reference's signature and layout (ref
    picotron/context_parallel/context_parallel.py:157-187): block_out [B, H, S, D], block_lse [B, H, S]; the
    running out fp32 [B, H, S, D] and lse [B, H, S, 1], against the reference-generated 3-block merge."""
    from picotron_amd.context_parallel.context_parallel import update_out_and_lse
    g = golden_kernels
    out = lse = None
    for i in range(3):
        out, lse = update_out_and_lse(out, lse, g[f"merge.block_out{i}"].to(BF).to(DEV), g[f"merge.block_lse{i}"].to(DEV))
    ref_out, ref_lse = None, None
    for i in range(3):
        ref_out, ref_lse = H.update_out_and_lse(ref_out, ref_lse, g[f"merge.block_out{i}"].to(BF).double(),
                                                g[f"merge.block_lse{i}"].double())
    assert out.dtype == torch.float32 and out.shape == ref_out.shape and lse.shape == ref_lse.shape
    assert max_abs(out.cpu(), ref_out) < 1e-5
    assert max_abs(lse.cpu(), ref_lse) < 1e-5


def test_merge_reference_slice_and_fp32_block():
    """slice_ (ref :183-184: merge into out[slice_] / lse[slice_] only) on a query-row slice and a head slice,
    fp32 block_out, and the first-call slice_ error, against the oracle's restatement of the same function."""
    from picotron_amd.context_parallel.context_parallel import update_out_and_lse
    torch.manual_seed(5)
    B, Hh, S, D = 2, 4, 96, 64
    blocks = [(torch.randn(B, Hh, S, D, device=DEV).to(BF), torch.randn(B, Hh, S, device=DEV) * 3) for _ in range(2)]
    rows = (slice(None), slice(None), slice(32, None))
    heads = (slice(None), slice(1, 3))
    b2 = (torch.randn(B, Hh, S - 32, D, device=DEV), torch.randn(B, Hh, S - 32, device=DEV) * 3)  # fp32 block
    b3 = (torch.randn(B, 2, S, D, device=DEV).to(BF), torch.randn(B, 2, S, device=DEV) * 3)
    with pytest.raises(RuntimeError):
        update_out_and_lse(None, None, *blocks[0], slice_=rows)
    out = lse = None
    ro = rl = None
    for bo, bl in blocks:
        out, lse = update_out_and_lse(out, lse, bo, bl)
        ro, rl = H.update_out_and_lse(ro, rl, bo.cpu().double(), bl.cpu().double())
    out, lse = update_out_and_lse(out, lse, *b2, slice_=rows)
    ro, rl = H.update_out_and_lse(ro, rl, b2[0].cpu().double(), b2[1].cpu().double(), slice_=rows)
    out, lse = update_out_and_lse(out, lse, *b3, slice_=heads)
    ro, rl = H.update_out_and_lse(ro, rl, b3[0].cpu().double(), b3[1].cpu().double(), slice_=heads)
    assert max_abs(out.cpu(), ro) < 1e-5
    assert max_abs(lse.cpu(), rl) < 1e-5


def test_merge_rebinds_and_casts_like_reference():
    """a non-slice update_out_and_lse returns new tensors and leaves the caller's running out / lse
    untouched (the reference's `_update` rebinds, ref :185); a bf16 block_lse and an fp16 block_out are cast to
    fp32 as the reference's arithmetic would (ref :174), not rejected."""
    from picotron_amd.context_parallel.context_parallel import update_out_and_lse
    torch.manual_seed(6)
    B, Hh, S, D = 1, 2, 64, 64
    bo0, bl0 = torch.randn(B, Hh, S, D, device=DEV).to(BF), torch.randn(B, Hh, S, device=DEV) * 3
    bo1 = torch.randn(B, Hh, S, D, device=DEV).to(torch.float16)
    bl1 = (torch.randn(B, Hh, S, device=DEV) * 3).to(BF)
    out0, lse0 = update_out_and_lse(None, None, bo0, bl0)
    keep_o, keep_l = out0.clone(), lse0.clone()
    out1, lse1 = update_out_and_lse(out0, lse0, bo1, bl1)
    assert out1.data_ptr() != out0.data_ptr() and lse1.data_ptr() != lse0.data_ptr()
    assert torch.equal(out0, keep_o) and torch.equal(lse0, keep_l)  # the caller's tensors are untouched
    ro, rl = H.update_out_and_lse(None, None, bo0.cpu().double(), bl0.cpu().double())
    ro, rl = H.update_out_and_lse(ro, rl, bo1.float().cpu().double(), bl1.float().cpu().double())
    assert max_abs(out1.cpu(), ro) < 1e-5
    assert max_abs(lse1.cpu(), rl) < 1e-5


def test_ring_attention_single_process_blocks():
    """Causal attention over a sequence split in 4 blocks, merged with the kernels the way the ring
    does (step s computes q_r against kv_{r-s}), equals whole-sequence attention."""
    ops = _ops()
    from picotron_amd.context_parallel.context_parallel import _merge_bshd
    torch.manual_seed(11)
    B, S, Hh, D, W = 1, 512, 2, 64, 4
    q, k, v = [torch.randn(B, S, Hh, D, dtype=BF, device=DEV) for _ in range(3)]
    full, _ = ops.attention_block_fwd(q, k, v, 0.125, True)
    n = S // W
    for r in range(W):
        out = lse = None
        for step in range(r + 1):
            src = r - step
            bo, bl = ops.attention_block_fwd(q[:, r * n:(r + 1) * n], k[:, src * n:(src + 1) * n],
                                             v[:, src * n:(src + 1) * n], 0.125, step == 0)
            out, lse = _merge_bshd(out, lse, bo, bl)
        assert rel_l2(out.cpu(), full[:, r * n:(r + 1) * n].float().cpu()) < 4e-3


# ------------------------------------------------------------------------------------------ DP kernels
def test_grad_accum_and_cast_bit_exact():
    from picotron_amd.data_parallel.bucket import HipBucketKernels as K
    torch.manual_seed(0)
    for n in (1, 7, 8, 1000003, 4096 * 2048):
        m = torch.randn(n, device=DEV)
        g = torch.randn(n, device=DEV).to(BF)
        ref = m.clone().add_(g)
        K.accumulate(m, g, 1)
        assert torch.equal(m, ref)
        for W in (8, 3, 6):  # reference: add_ then /= W (ATen: * fp32(1/W) on the GPU)
            ref = m.clone().add_(g)
            ref /= W
            K.accumulate(m, g, W)
            assert torch.equal(m, ref), W
        ref = m.clone()
        ref /= 3
        K.scale(m, 3)
        assert torch.equal(m, ref)
        out = torch.empty(n, dtype=BF, device=DEV)
        K.cast(m, out)
        assert torch.equal(out, m.to(BF))
    # unaligned views (param offsets inside a bucket)
    big = torch.randn(1000, device=DEV)
    gg = torch.randn(1000, device=DEV).to(BF)
    v = big[3:803]
    ref = v.clone().add_(gg[3:803])
    K.accumulate(v, gg[3:803], 1)
    assert torch.equal(v, ref)


@pytest.mark.parametrize("n,vocab", [(1, 10), (7, 3), (1000, 49152), (4096, 49152), (4096, 17), (8192, 1 << 19),
                                     (3000, 32000)])
def test_sort_ids_matches_torch_stable_sort(n, vocab):
    """pico_sort_ids == torch.sort(ids, stable=True): ids and positions bit for bit (heavy duplicates,
    non-power-of-two counts, the largest id / count the packed key allows)."""
    ops = _ops()
    g = torch.Generator(device="cpu").manual_seed(n + vocab)
    ids = torch.randint(0, vocab, (n,), generator=g).to(DEV)
    if n > 2:
        ids[-1] = vocab - 1
        ids[0] = vocab - 1
    s1, p1 = ops.sort_ids(ids, vocab)
    s2, p2 = torch.sort(ids, stable=True)
    assert torch.equal(s1, s2) and torch.equal(p1, p2)


# ------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32])
def test_embedding_bwd_matches_dense(grad_dtype):
    """pico_embedding_bwd (stable sort + one workgroup per id run) == the dense backward of
    F.embedding accumulated into an existing gradient, incl. repeated ids and the 1/W scale; and it
    is deterministic (bitwise equal across calls)."""
    from picotron_amd.ops import _embedding_bwd_into
    torch.manual_seed(1)
    V, H, B, S = 512, 256, 3, 100
    ids = torch.randint(0, V // 4, (B, S), device=DEV)  # many repeats
    dy = torch.randn(B, S, H, dtype=BF, device=DEV)
    g0 = torch.randn(V, H, dtype=grad_dtype, device=DEV)
    dense = torch.zeros(V, H, dtype=torch.float64, device=DEV)
    dense.index_add_(0, ids.reshape(-1), dy.reshape(-1, H).double())
    scale = 0.25 if grad_dtype == torch.float32 else 1.0
    touched = torch.zeros(V, dtype=torch.bool, device=DEV)
    touched[ids.reshape(-1)] = True
    want = g0.double() + dense
    want[touched] *= scale  # only the rows of ids present are rewritten (and scaled)
    got = g0.clone()
    _embedding_bwd_into(got, ids, dy, scale)
    tol = 1e-6 if grad_dtype == torch.float32 else 8e-3
    assert rel_l2(got.cpu(), want.cpu()) < tol
    assert torch.equal(got[~touched], g0[~touched])
    again = g0.clone()
    _embedding_bwd_into(again, ids, dy, scale)
    assert torch.equal(again, got)


# ------------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("V,ignore", [(49152, False), (512, True), (32000, False)])
def test_cross_entropy_matches_torch(V, ignore):
    """pico_cross_entropy_fwd/_bwd == F.cross_entropy(mean) on the same bf16 logits: loss within bf16
    rounding of an fp64 reference, dlogits (incl. a non-unit upstream gradient) vs fp64 softmax - onehot,
    ignored targets (-100) excluded from the mean and given zero gradient."""
    from picotron_amd import ops
    torch.manual_seed(V)
    N = 300
    logits = (torch.randn(N, V, device=DEV) * 3).to(BF).requires_grad_(True)
    tgt = torch.randint(0, V, (N,), device=DEV)
    if ignore:
        tgt[::7] = -100
    loss = ops.cross_entropy(logits, tgt)
    (loss * 0.25).backward()
    x = logits.detach().double()
    keep = tgt != -100
    lse = torch.logsumexp(x, dim=1)
    ref_rows = lse - x.gather(1, tgt.clamp_min(0)[:, None]).squeeze(1)
    ref = ref_rows[keep].mean()
    assert loss.dtype == BF
    assert abs(float(loss) - float(ref)) <= 8e-3 * abs(float(ref)) + 1e-3
    p = torch.softmax(x, dim=1)
    p[torch.arange(N, device=DEV), tgt.clamp_min(0)] -= 1
    p[~keep] = 0
    p *= 0.25 / keep.sum()
    assert rel_l2(logits.grad.cpu(), p.cpu()) < 8e-3
    assert float(logits.grad[~keep].abs().sum()) == 0.0
    t_loss = torch.nn.functional.cross_entropy(logits.detach(), tgt)
    assert abs(float(t_loss) - float(loss)) <= 1.6e-2 * abs(float(ref)) + 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize("V,ignore,g", [(4000, False, 1.0), (4000, True, 0.25), (49152, True, 1.0 / 3)])
def test_lm_head_cross_entropy_fused(V, ignore, g):
    """ops.lm_head_cross_entropy (LM head GEMM + CE with dlogits written in the forward pass) ==
    mean F.cross_entropy(x W^T) in fp64: loss, dx and dW (accumulated onto an existing .grad) for a
    non-unit upstream gradient g, ignore_index rows excluded; and it agrees with the unfused
    ops.linear + ops.cross_entropy path."""
    from picotron_amd import ops
    torch.manual_seed(V + int(ignore))
    T, H = 512, 256
    x = (torch.randn(T, H, device=DEV) * 0.5).to(BF).requires_grad_(True)
    w = (torch.randn(V, H, device=DEV) * 0.05).to(BF).requires_grad_(True)
    w0 = (torch.randn(V, H, device=DEV) * 1e-5).to(BF)  # same scale as dW: accumulation visible in bf16
    w.grad = w0.clone()
    tgt = torch.randint(0, V, (T,), device=DEV)
    if ignore:
        tgt[::5] = -100
    loss = ops.lm_head_cross_entropy(x, w, tgt)
    (loss * g).backward()
    xd, wd = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(xd @ wd.t(), tgt)
    (ref * g).backward()
    assert loss.dtype == BF
    assert abs(float(loss) - float(ref)) <= 8e-3 * abs(float(ref)) + 1e-3
    assert rel_l2(x.grad.cpu(), xd.grad.cpu()) < 1.5e-2
    assert rel_l2((w.grad.double() - w0.double()).cpu(), wd.grad.cpu()) < 3e-2
    # the unfused path on the same inputs
    x2 = x.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    l2 = ops.cross_entropy(ops.linear(x2, w2), tgt)
    (l2 * g).backward()
    assert abs(float(l2) - float(loss)) <= 1e-2 * abs(float(ref)) + 2e-3
    assert rel_l2(x.grad.cpu(), x2.grad.cpu()) < 1.5e-2


@pytest.mark.gpu
@pytest.mark.parametrize("n,gdt,g", [(4096 * 2048, torch.bfloat16, 1.0), (1000, torch.float32, 0.37),
                                     (8 * 257 + 5, torch.bfloat16, 1.0 / 3), (3, torch.float32, -2.5)])
def test_ce_scale_grad_matches_torch_mul(n, gdt, g):
    """pico_ce_scale_grad (the LM-head CE backward's dx *= upstream gradient, read on the device) == ATen's
    dx.mul_(upstream) bit for bit (ATen casts the 0-dim operand to bf16 first), vector body and scalar tail."""
    from picotron_amd import ops
    torch.manual_seed(n)
    dx = torch.randn(n, dtype=BF, device=DEV)
    up = torch.tensor(g, dtype=gdt, device=DEV)
    ref = dx.clone().mul_(up)
    out = ops._scale_by_upstream(dx, up)
    torch.cuda.synchronize()
    assert out.data_ptr() == dx.data_ptr()
    assert torch.equal(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("T,chunk,V,ignore,mode", [(512, 128, 4000, False, "grad"), (500, 192, 4000, True, "fresh"),
                                                   (1024, 1024, 49152, True, "grad"), (700, 256, 4000, True, "autograd"),
                                                   (384, 100, 4000, False, "nograd")])
def test_lm_head_cross_entropy_chunked(T, chunk, V, ignore, mode):
    """ops.lm_head_cross_entropy(grad_scale=s, chunk=c) — logits never whole, dx / dW taken chunk by chunk in
    the forward — == s * mean F.cross_entropy(x W^T) in fp64 with unit upstream gradient: loss, dx, dW
    accumulated onto an existing bf16 .grad ("grad"), created when .grad is None ("fresh"), handed to
    autograd when the weight has a hook ("autograd"), or not at all ("nograd": weight frozen); ragged last
    chunks and ignore_index rows included. It matches the unchunked fused form on the same inputs."""
    from picotron_amd import ops
    torch.manual_seed(T + chunk + V)
    H, s = 256, 0.25
    x = (torch.randn(T, H, device=DEV) * 0.5).to(BF).requires_grad_(True)
    w = (torch.randn(V, H, device=DEV) * 0.05).to(BF).requires_grad_(mode != "nograd")
    w0 = (torch.randn(V, H, device=DEV) * 1e-5).to(BF)
    if mode == "grad":
        w.grad = w0.clone()
    if mode == "autograd":
        w.register_hook(lambda g: g)
    tgt = torch.randint(0, V, (T,), device=DEV)
    if ignore:
        tgt[::7] = -100
    loss = ops.lm_head_cross_entropy(x, w, tgt, grad_scale=s, chunk=chunk)
    loss.backward()
    xd, wd = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(xd @ wd.t(), tgt) * s
    ref.backward()
    assert loss.dtype == BF
    assert abs(float(loss) - float(ref)) <= 8e-3 * abs(float(ref)) + 1e-3
    assert rel_l2(x.grad.cpu(), xd.grad.cpu()) < 1.5e-2
    if mode != "nograd":
        got = w.grad.double() - (w0.double() if mode == "grad" else 0)
        assert rel_l2(got.cpu(), wd.grad.cpu()) < 3e-2
    else:
        assert w.grad is None
    # the unchunked fused form on the same inputs
    x2 = x.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    l2 = ops.lm_head_cross_entropy(x2, w2, tgt)
    (l2 * s).backward()
    assert abs(float(l2) * s - float(loss)) <= 1e-2 * abs(float(ref)) + 2e-3
    assert rel_l2(x.grad.cpu(), x2.grad.cpu()) < 1e-2
    if mode != "nograd":
        assert rel_l2(got.cpu(), w2.grad.double().cpu()) < 1e-2


@pytest.mark.gpu
def test_lm_head_ce_chunked_contract_and_loss_acc():
    """the chunked form takes dW in the forward for a unit upstream gradient. A backward
    with any other upstream gradient (here loss * 3) still gets an exact dx, and the violation is recorded on
    the device by the backward's own launch and raised by check_lm_head_grad_scale(); a unit upstream does not
    raise. VERDICT r02 item 9: loss_acc += loss inside the pico_ce_mean launch (value as stored in the bf16 loss)."""
    from picotron_amd import ops
    torch.manual_seed(9)
    T, H, V = 256, 128, 1024
    x = (torch.randn(T, H, device=DEV) * 0.5).to(BF).requires_grad_(True)
    w = (torch.randn(V, H, device=DEV) * 0.05).to(BF).requires_grad_(True)
    tgt = torch.randint(0, V, (T,), device=DEV)
    acc = torch.full((), 0.5, dtype=torch.float32, device=DEV)
    ops.check_lm_head_grad_scale()  # clean slate
    loss = ops.lm_head_cross_entropy(x, w, tgt, grad_scale=0.5, chunk=64, loss_acc=acc)
    loss.backward()
    torch.cuda.synchronize()
    assert float(acc) == 0.5 + float(loss.float())
    ops.check_lm_head_grad_scale()  # unit upstream: no violation
    dx1 = x.grad.clone()
    x.grad = None
    w.grad = None
    loss = ops.lm_head_cross_entropy(x, w, tgt, grad_scale=0.5, chunk=64)
    (loss * 3).backward()
    assert rel_l2(x.grad.float().cpu(), (dx1.float() * 3).cpu()) < 1e-2  # dx exact for any upstream
    with pytest.raises(RuntimeError, match="upstream gradient"):
        ops.check_lm_head_grad_scale()
    ops.check_lm_head_grad_scale()  # the flag was reset by the raise


# ------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("R,C,ld_pad", [(4096, 2048, 0), (6144, 2048, 0), (2048, 49152, 0), (72, 8, 0),
                                        (8, 136, 0), (200, 264, 16), (64, 64, 8)])
def test_transpose_bit_exact(R, C, ld_pad):
    """pico_transpose_bf16 == x.t() bit for bit, incl. partial tiles and padded row strides on both sides
    (the padding of the output is left untouched)."""
    from picotron_amd import ops
    torch.manual_seed(R + C)
    base = torch.randn(R, C + ld_pad, device=DEV).to(BF)
    x = base[:, :C]
    out_base = torch.full((C, R + ld_pad), 7.0, device=DEV, dtype=BF)
    out = out_base[:, :R]
    ops.transpose_2d(x, out=out)
    assert torch.equal(out, x.t())
    if ld_pad:
        assert bool((out_base[:, R:] == 7.0).all())
    assert torch.equal(ops.transpose_2d(x), x.t().contiguous())


# ------------------------------------------------------------------------------------------ fused RoPE backward
@pytest.mark.parametrize("B,S,Hq,Hkv,D", [(4, 1024, 32, 32, 64), (2, 256, 4, 2, 64), (1, 384, 4, 4, 128)])
def test_attention_rope_bwd_fused(B, S, Hq, Hkv, D):
    """PICO_ATTN_ROPE_BWD (RoPE^-1 fused into the dQ slab sum and the dK epilogue / dK-dV reduce, both
    the one-workgroup-per-key-block grid and the split small grid) == attention backward followed by the
    separate pico_rope(conjugate=1) on dq and dk, within one bf16 rounding; dv untouched."""
    from picotron_amd import ops
    from picotron_amd.model import get_cos_sin
    torch.manual_seed(S + D)
    q, do = [torch.randn(B, S, Hq, D, dtype=BF, device=DEV) for _ in range(2)]
    k, v = [torch.randn(B, S, Hkv, D, dtype=BF, device=DEV) for _ in range(2)]
    cos, sin = get_cos_sin(S, D, base=10000.0)
    cos, sin = cos.to(DEV, BF)[:, : D // 2], sin.to(DEV, BF)[:, : D // 2]
    sc = 1.0 / math.sqrt(D)
    o, lse = ops.attention_block_fwd(q, k, v, sc, True)
    dq0, dk0, dv0 = ops.attention_block_bwd(do, q, k, v, o, lse, sc, True)
    ref_dq, ref_dk = torch.empty_like(dq0), torch.empty_like(dk0)
    ops._rope_launch(dq0, ref_dq, cos, sin, True)
    ops._rope_launch(dk0, ref_dk, cos, sin, True)
    dq, dk, dv = [torch.empty_like(t) for t in (q, k, v)]
    ops._attention_bwd_into(do, q, k, v, o, lse, sc, True, dq, dk, dv, rope=(cos, sin))
    torch.cuda.synchronize()
    assert torch.equal(dv, dv0)
    assert rel_l2(dq.float().cpu(), ref_dq.float().cpu()) < 4e-3
    assert rel_l2(dk.float().cpu(), ref_dk.float().cpu()) < 4e-3


@pytest.mark.parametrize("B,S,Hq,Hkv,D,causal", [(4, 1024, 32, 32, 64, True), (2, 200, 4, 2, 64, True),
                                                  (1, 384, 4, 4, 128, True), (1, 330, 4, 2, 128, False)])
def test_attention_rope_q_fwd_fused(B, S, Hq, Hkv, D, causal):
    """PICO_ATTN_ROPE_Q_FWD (RoPE on q inside the attention forward, rotated q stored back into the qkv
    buffer) == pico_rope on q followed by the plain forward, bit for bit (both rotations round the two
    products before the sum, as the fp32 oracle does: ADVICE r02), and so O and LSE bit-equal too; k/v
    columns untouched. The rope kernel itself is pinned to the oracle by test_rope_golden."""
    from picotron_amd import ops
    from picotron_amd.model import get_cos_sin
    torch.manual_seed(S + D + Hkv)
    qkv = torch.randn(B, S, Hq + 2 * Hkv, D, dtype=BF, device=DEV)
    cos, sin = get_cos_sin(S, D, base=10000.0)
    cos, sin = cos.to(DEV, BF)[:, : D // 2], sin.to(DEV, BF)[:, : D // 2]
    sc = 1.0 / math.sqrt(D)
    q0 = qkv[:, :, :Hq]
    q_ref = torch.empty(q0.shape, dtype=BF, device=DEV)
    ops._rope_launch(q0, q_ref, cos, sin, False)
    kv0 = qkv[:, :, Hq:].clone()
    q_unrot = q0.clone()
    o_ref, lse_ref = ops.attention_block_fwd(q_ref, qkv[:, :, Hq:Hq + Hkv], qkv[:, :, Hq + Hkv:], sc, causal)
    o, lse = ops.attention_block_fwd(qkv[:, :, :Hq], qkv[:, :, Hq:Hq + Hkv], qkv[:, :, Hq + Hkv:], sc, causal,
                                     rope_q=(cos, sin))
    torch.cuda.synchronize()
    q = qkv[:, :, :Hq]
    assert torch.equal(qkv[:, :, Hq:], kv0)
    assert torch.equal(q, q_ref)
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
    # and the same rotation as the fp32 oracle (products rounded before the sum), bit for bit
    assert torch.equal(q.cpu(), H.rope_fused(q_unrot.cpu(), cos.cpu(), sin.cpu()))


@pytest.mark.parametrize("B,S,H,D,causal", [(2, 256, 4, 64, True), (1, 200, 2, 128, False), (4, 1024, 32, 64, True),
                                             (1, 100, 2, 64, True), (3, 140, 2, 128, True)])
def test_attention_fwd_transposed_output(B, S, H, D, causal):
    """pico_attn_fwd's optional o_t output == O transposed to [H*D, tokens], bit for bit (same rounding),
    and O itself unchanged by requesting it."""
    from picotron_amd import ops
    torch.manual_seed(S)
    q, k, v = [torch.randn(B, S, H, D, dtype=BF, device=DEV) for _ in range(3)]
    o_ref, lse_ref = ops.attention_block_fwd(q, k, v, 0.1, causal)
    o_t = torch.full((H * D, B * S + 8), 3.0, dtype=BF, device=DEV)[:, : B * S]
    o, lse = ops.attention_block_fwd(q, k, v, 0.1, causal, o_t=o_t)
    torch.cuda.synchronize()
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
    assert torch.equal(o_t, o.reshape(B * S, H * D).t())


@pytest.mark.parametrize("T,I", [(256, 512), (192, 576)])  # 128-column tiles; 64-column tiles (I % 128 != 0)
def test_swiglu_fwd_transposed_output(T, I):
    """pico_swiglu_fwd_t == pico_swiglu_fwd bit for bit on h, and writes h^T exactly (fused gate|up layout)."""
    from picotron_amd import _lib as L
    from picotron_amd import ops
    torch.manual_seed(5)
    gu = torch.randn(T, 2 * I, dtype=BF, device=DEV)
    h_ref = torch.empty(T, I, dtype=BF, device=DEV)
    ops._swiglu_fwd(gu, gu[:, I:], h_ref, T, I, 2 * I, I)
    h = torch.empty(T, I, dtype=BF, device=DEV)
    ht = torch.full((I, T + 16), 2.0, dtype=BF, device=DEV)
    L.check(L.load().pico_swiglu_fwd_t(L.ptr(gu), L.ptr(gu[:, I:]), L.ptr(h), L.ptr(ht), T, I, 2 * I, I, T + 16,
                                       L.stream_of(gu)), "swiglu_fwd_t")
    torch.cuda.synchronize()
    assert torch.equal(h, h_ref)
    assert torch.equal(ht[:, :T], h.t())
    assert bool((ht[:, T:] == 2.0).all())


@pytest.mark.parametrize("rows,cols,res", [(64, 2048, True), (96, 1024, False), (256, 2048, True), (4096, 2048, True)])
def test_rmsnorm_fwd_transposed_output(rows, cols, res):
    """pico_rmsnorm_fwd_t == pico_rmsnorm_fwd bit for bit (y, residual_out, rstd) and writes y^T exactly."""
    from picotron_amd import ops
    torch.manual_seed(rows + cols)
    x = torch.randn(rows, cols, dtype=BF, device=DEV)
    r = torch.randn(rows, cols, dtype=BF, device=DEV) if res else None
    w = (1 + 0.1 * torch.randn(cols, device=DEV)).to(BF)
    out_ref = ops._RMSNormFn.apply(x, r, w, 1e-5, res, False)
    out = ops._RMSNormFn.apply(x, r, w, 1e-5, res, True)
    y_ref, y = (out_ref[0], out[0]) if res else (out_ref, out)
    assert torch.equal(y, y_ref)
    if res:
        assert torch.equal(out[1], out_ref[1])
    assert torch.equal(y._pico_t, y.t())

