"""fp64 reference, bounds and the guarded launch for pico_decode_linear / ops.decode_linear
(tests/test_decode_linear_host.py, tests/test_decode_linear_gpu.py). A plain helper module.

Bounds (rowwise_ref.elem_check, |got - ref| <= U |ref| + k 2^-23 cond + 2^-120):
  projection   cond[m, n] = sum_k |h[m, k] W[n, k]|, k = K. bf16 x bf16 products are exact in fp32 and any-order fp32
               summation of K terms errs by at most (K - 1) 2^-24 sum|terms|: the bound is twice the worst case.
  SWIGLU       g and u are the projection's own bf16 outputs (same rows of W, same wave and slice order, so the same
               bits as the BF16 epilogue gives under the same split_k): the tests take them from a BF16 run, which
               the projection bound covers, and require bf16(silu(g) u) of exactly those values (swiglu_of). With
               random signs the worst-case fp32 term of g and u reaches the bf16 spacing, so marking undecided g / u
               against fp64 would mark most of them; this check needs no marking and holds at any K.
Undecided roundings: an h of the norm prologue whose fp64 value lies within its fp32 error term of a bf16 rounding
boundary may round either way. The term: |h| (K / 64 + 16) 2^-24 (the lane-then-wave sum of K non-negative squares
errs by (K / 64 + 6) 2^-24 relative at most, halved by the rsqrt, plus one ulp for the rsqrt and one for each of the
two products, rounded up). Exactly those elements are marked, and the bound of the outputs they reach is widened by
|W[n, k]| ulp_bf16(h[m, k]); MAX_UNDECIDED caps their share."""
import torch

import attn_ref as A
import rowwise_ref as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
MAX_UNDECIDED = 0.01


def _other_rounding(v64):
    """(nearest bf16 of v64, the bf16 neighbour on v64's side of it, distance of v64 to the boundary between them)."""
    near = v64.to(BF)
    step = torch.where(v64.abs() > near.double().abs(), 1, -1).to(torch.int16)
    other = (near.view(torch.int16) + step).view(BF)
    mid = (near.double() + other.double()) / 2
    return near, other, (v64 - mid).abs()


def inputs(M, N, K):
    """(x [M, K], w [N, K] at scale K^-1/2, norm_weight [K] around 1, residual [M, K]), randn in bf16 on the CPU."""
    g = torch.Generator().manual_seed(1000 * M + N + K + 1)
    x, w, nw, res = (torch.randn(*s, generator=g) for s in ((M, K), (N, K), (K,), (M, K)))
    return x.to(BF), (w / K ** 0.5).to(BF), (1 + 0.1 * nw).to(BF), res.to(BF)


def reference(x, w, norm_weight=None, eps=1e-5, residual=None):
    """x [M, K], w [N, K] (, norm_weight [K], residual [M, K]) bf16 on the CPU. Returns {"y": (ref, cond, k),
    "residual_out": exact bf16 or None, "undecided": {name: share}}; cond already holds the widening of the elements
    an undecided rounding reaches (as extra / (k 2^-23))."""
    K = x.shape[1]
    wd = w.double()
    h, res_out, widen, share = x.double(), None, 0.0, {}
    if norm_weight is not None:
        xe = x if residual is None else (x.float() + residual.float()).to(BF)
        res_out = xe if residual is not None else None
        xe = xe.double()
        h64 = xe * torch.rsqrt(xe.pow(2).mean(-1, keepdim=True) + eps) * norm_weight.double()
        near, other, dist = _other_rounding(h64)
        und = dist <= h64.abs() * (K / 64 + 16) * 2.0 ** -24
        share["h"] = float(und.double().mean())
        h = near.double()
        widen = torch.where(und, (other.double() - h).abs(), 0.0) @ wd.abs().t()  # (a zero's neighbour is NaN)
    acc = h @ wd.t()
    cond = h.abs() @ wd.abs().t()
    return {"y": (acc, cond + widen / (K * R.ULP32), float(K)), "residual_out": res_out, "undecided": share}


def check(tag, got, ref):
    """got {"y", "residual_out"} against reference(): every element of y inside its bound, residual_out bit-equal,
    the undecided share under the cap."""
    for name, s in ref["undecided"].items():
        assert s <= MAX_UNDECIDED, (tag, name, s)
    y = got["y"].cpu()
    if y.dtype == F32:  # the F32 epilogue: float(bf16(acc)), so every value is a bf16 value
        assert torch.equal(y, y.to(BF).float()), tag
        y = y.to(BF)
    r_, c_, k = ref["y"]
    R.report(tag, [R.elem_check("y", y, r_, c_, BF, k)])
    if ref["residual_out"] is not None:
        assert torch.equal(got["residual_out"].cpu().view(torch.int16), ref["residual_out"].view(torch.int16)), tag


def swiglu_of(y, exact=False):
    """The SWIGLU epilogue on a BF16 run's output y [M, 2 I] (gate | up): on the device pico_swiglu_fwd itself
    (exact: the comparison is bit for bit); on the CPU the fp64 value and ref_swiglu_fwd's cond for elem_check."""
    inter = y.shape[1] // 2
    if exact:
        return R.launch_swiglu(y[:, :inter].contiguous(), y[:, inter:].contiguous())["h"]
    return R.ref_swiglu_fwd(y[:, :inter], y[:, inter:])["h"]


def planted(M, N, K):
    """W zero except W[n, (5 n + 3) mod K] = 1; x[m, k] a distinct bf16-exact value: output (m, n) is x[m, (5 n + 3)
    mod K] exactly, so every output names the (n, k) it read."""
    w = torch.zeros(N, K)
    n = torch.arange(N)
    w[n, (5 * n + 3) % K] = 1.0
    x = ((torch.arange(M)[:, None] * 7 + torch.arange(K)[None, :]) % 251 - 125).float() / 4
    return x.to(BF), w.to(BF)


def launch(x, w, norm_weight=None, eps=1e-5, residual=None, want_res_out=True, swiglu=False, f32=False, split_k=0,
           ldx=None, ldw=None):
    """pico_decode_linear on NaN-guarded buffers (attn_ref.Guards), the guards checked untouched after the launch.
    Inputs are CPU or device bf16 tensors. Returns {"y", "residual_out"}."""
    import ctypes
    from picotron_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda")
    M, K = x.shape
    N = w.shape[0]
    epi = L.DL_SWIGLU if swiglu else (L.DL_F32 if f32 else L.DL_BF16)
    G = A.Guards(dev)
    xg = G.mat("x", M, K, data=x.to(dev), ld=ldx)
    wg = G.mat("w", N, K, data=w.to(dev), ld=ldw)
    outs = N // 2 if swiglu else N
    y = G.mat("y", M, outs, dtype=F32 if f32 else BF, ld=outs + 8)
    a = L.DecodeLinearArgs()
    a.x, a.weight, a.y = xg.data_ptr(), wg.data_ptr(), y.data_ptr()
    a.ldx, a.ldw, a.ldy = xg.stride(0), wg.stride(0), y.stride(0)
    ro = None
    if norm_weight is not None:
        a.norm_weight = G.mat("norm_weight", 1, K, data=norm_weight.to(dev)).data_ptr()
        if residual is not None:
            rg = G.mat("residual", M, K, data=residual.to(dev), ld=K + 8)
            a.residual, a.ldr = rg.data_ptr(), rg.stride(0)
        if want_res_out:
            ro = G.mat("residual_out", M, K, ld=K + 16)
            a.residual_out, a.ldro = ro.data_ptr(), ro.stride(0)
    nbytes = lib.pico_decode_linear_workspace_bytes(M, N, K, epi, split_k)
    assert nbytes >= 0, lib.pico_last_error()
    if nbytes:
        a.workspace = G.flat("workspace", nbytes, torch.uint8).data_ptr()
    a.m, a.n, a.k, a.split_k, a.eps, a.epilogue = M, N, K, split_k, eps, epi
    G.arm()
    L.check(lib.pico_decode_linear(ctypes.byref(a), L.stream_of(xg)), "pico_decode_linear")
    torch.cuda.synchronize()
    G.check()
    return {"y": y, "residual_out": ro}
