"""References, restatements, the per-element check, input sets and guarded launches for the row-wise and elementwise
kernel tests (tests/test_rowwise_host.py, tests/test_rowwise_gpu.py): rmsnorm.hip, rope.hip, swiglu.hip,
cross_entropy.hip, embedding.hip. A plain helper module: no fixture, no conftest; plain torch on any device except the
launch helpers at the bottom, which need the library and a HIP device.

ref_*       fp64, the operation itself. Each returns {output name: (reference, cond)}; cond is the fp64 condition
            term of elem_check, its formula in the function's docstring.
restate_*   the same operation at the kernel's own precision, in plain torch: fp32 math on the bf16 inputs with
            roundings where the kernel rounds, the order-sensitive reductions (RMSNorm dw, embedding runs) in the
            kernel's order. Written from the formulas in the kernels' header comments; this is what "a correct
            kernel" means to the host tests. The kernels' outputs calibrate nothing.
elem_check  every element of an output, none exempt:
                |got - ref| <= U |ref| + K 2^-23 cond + 2^-120
            U = 2^-8 for a bf16 output (the unit roundoff of bf16's 8-bit significand: one round-to-nearest of the
            result), 0 for an fp32 output; K = 8 fp32 ulps of the condition term
            (the restatements need at most 1.5 against fp64; the rest is room for the hardware's 1-ulp exp2 / log2 /
            rcp / rsq); 2^-120 absorbs fp32 / bf16 underflow (silu(-90), softmax tails at sigma = 30).
"""
import math

import torch

import attn_ref as A
from oracle import hotpath as H

BF = torch.bfloat16
F32, F64 = torch.float32, torch.float64
U_BF16 = 2.0 ** -8
K_ELEM = 8.0
ULP32 = 2.0 ** -23
TINY = 2.0 ** -120
OLD_TOL, OLD_TOL_CE = 4e-3, 8e-3  # the whole-tensor rel_l2 thresholds of tests/test_kernels_gpu.py
LOG2E = 1.4426950408889634
IGNORE = -100
rel_l2 = A.rel_l2


# ------------------------------------------------------------------------------------------ the check
def elem_check(name, got, ref, cond, out_dtype, k=K_ELEM):
    """|got - ref| <= U |ref| + k 2^-23 cond + 2^-120 for every element (U = 2^-8 for a bf16 output, 0 for fp32).
    Returns {"ok", "ratio" (worst |err| / bound), "index" (of that element), "k" (the smallest K that would pass
    every element, 0 when the U term alone does), "output", "err", "ref"}; a NaN or inf in got fails."""
    assert got.shape == ref.shape == cond.shape, (name, got.shape, ref.shape, cond.shape)
    assert got.dtype == out_dtype, (name, got.dtype)
    u = U_BF16 if out_dtype == BF else 0.0
    ref, cond = ref.double(), cond.double()
    err = (got.double() - ref).abs()
    base = u * ref.abs() + TINY
    ratio = torch.nan_to_num(err / (base + k * ULP32 * cond), nan=math.inf, posinf=math.inf)
    kneed = torch.nan_to_num((err - base).clamp_min(0) / (ULP32 * cond).clamp_min(1e-300), nan=math.inf, posinf=math.inf)
    if ratio.numel() == 0:
        return {"ok": True, "ratio": 0.0, "index": (), "k": 0.0, "output": name, "err": 0.0, "ref": 0.0}
    i = int(ratio.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape)) if ratio.dim() else ()
    worst = float(ratio.flatten()[i])
    return {"ok": worst <= 1.0, "ratio": worst, "index": idx, "k": float(kneed.max()), "output": name,
            "err": float(err.flatten()[i]), "ref": float(ref.flatten()[i])}


def report(tag, results, worst_k=None):
    """One line per output; asserts every one. worst_k: optional dict collecting the largest K per operation and output."""
    for r_ in results:
        print(f"ELEM {tag} {r_['output']} ratio {r_['ratio']:.3f} K {r_['k']:.2f} at {r_['index']}: "
              f"err {r_['err']:.3e}, ref {r_['ref']:.3e}")
        if worst_k is not None:
            key = f"{tag.split()[0]}.{r_['output']}"  # the tag's first word names the operation
            worst_k[key] = max(worst_k.get(key, 0.0), r_["k"])
    bad = [r_ for r_ in results if not r_["ok"]]
    assert not bad, (tag, bad)


def check_all(tag, got, ref, k=K_ELEM, worst_k=None):
    """got {name: tensor} against ref {name: (reference, cond)}: every output of ref must be present in got."""
    report(tag, [elem_check(n, got[n], r_, c_, got[n].dtype, k) for n, (r_, c_) in ref.items()], worst_k)


# ------------------------------------------------------------------------------------------ input sets
def _gen(seed, *dims):
    return torch.Generator().manual_seed(seed * 7919 + sum((i + 3) * int(d) for i, d in enumerate(dims)))


def make(kind, rows, cols, seed=0, device="cpu"):
    """bf16 [rows, cols]. randn; wide: random sign, magnitude log-uniform in 2^-12 .. 2^6; big: sigma = 30 (saturates
    sigmoid / exp); bait: row r scaled by 2^(r mod 7), and a planted element of 24 x that scale (alternating sign) in
    column 0 and in the row's last 8-vector (column cols - 1 - r mod 8), so a lost or misplaced vector, a neighbour's
    row statistic or a skipped tail is far outside the bound."""
    g = _gen(seed, rows, cols, len(kind))
    x = torch.randn(rows, cols, generator=g)
    if kind == "wide":
        sign = torch.where(torch.rand(rows, cols, generator=g) < 0.5, -1.0, 1.0)
        x = sign * torch.exp2(torch.rand(rows, cols, generator=g) * 18.0 - 12.0)
    elif kind == "big":
        x = x * 30.0
    elif kind == "bait":
        r = torch.arange(rows)
        sc = torch.exp2((r % 7).float())
        x = x * sc[:, None]
        sg = torch.where(r % 2 == 0, 1.0, -1.0)
        x[r, 0] = 24.0 * sc * sg
        x[r, cols - 1 - (r % min(8, cols))] = -24.0 * sc * sg
    elif kind != "randn":
        raise ValueError(kind)
    return x.to(BF).to(device)


KINDS = ("randn", "wide", "big", "bait")


def ce_columns(V):
    """The planted columns of the CE bait set: 0, 7, 8, V - 8, V - 1 and either side of every thread / pass boundary
    the vocabulary has (chunk 255 | 256: elements 2047 | 2048; chunk 511 | 512: 4095 | 4096)."""
    return sorted({c for c in (0, 7, 8, V - 8, V - 1, 2047, 2048, 4095, 4096) if 0 <= c < V})


def make_ce(kind, V, seed=0, device="cpu"):
    """(logits bf16 [rows, V], target int64 [rows]). randn / wide / big: 4 rows — a plain one (random target), an
    ignored one, target 0, target V - 1. bait: for every column c of ce_columns(V) one row whose maximum is planted
    at c (4 nats above the rest of the row, so the target's softmax stays clear of 1: the fp32 lse of a row of
    magnitude 2^7 has an absolute error of 2^-17, which a one-hot row would turn into the whole of p - 1) with the
    target on c (even rows) or on the next planted column (odd rows), rows scaled by 2^(r mod 7) / 2, and an ignored
    row after every second row. The last row is a tower: randn with 120 in the last column and the target in column
    0, so a row maximum taken over part of the row overflows the sum."""
    g = _gen(seed, V, len(kind), 11)
    if kind != "bait":
        x = make(kind, 4, V, seed + 1)
        t = torch.tensor([int(torch.randint(0, V, (1,), generator=g)), IGNORE, 0, V - 1])
        return x.to(device), t.to(device)
    cols = ce_columns(V)
    rows, tg = [], []
    for i, c in enumerate(cols):
        row = torch.randn(V, generator=g) * (0.5 * 2.0 ** (i % 7))
        row[c] = -math.inf
        row[c] = float(row.max()) + 4.0
        rows.append(row)
        tg.append(c if i % 2 == 0 else cols[(i + 1) % len(cols)])
        if i % 2 == 1:
            rows.append(torch.randn(V, generator=g))
            tg.append(IGNORE)
    tower = torch.randn(V, generator=g)
    tower[V - 1] = 120.0
    rows.append(tower)
    tg.append(0)
    return torch.stack(rows).to(BF).to(device), torch.tensor(tg).to(device)


ID_KINDS = ("bait_a", "bait_b", "run0", "runV", "random")


def make_ids(kind, n, V, seed=0, device="cpu"):
    """int64 [n] token ids. random: ids in [1, V - 2]. bait_a: a run of one at id 0 and a run of two at id V - 1, at
    scattered positions, the rest random in [1, V - 2] (so no random id lengthens a planted run); bait_b: the run of
    two at id 0 and the run of one at V - 1; run0 / runV: one run of n at id 0 / V - 1. With n < 3 the bait kinds
    hold id 0 (bait_a) or V - 1 (bait_b) only."""
    g = _gen(seed, n, V, 5)
    ids = torch.randint(1, V - 1, (n,), generator=g)
    if kind in ("run0", "runV") or (kind != "random" and n < 3):
        ids[:] = 0 if kind in ("run0", "bait_a") else V - 1
    elif kind in ("bait_a", "bait_b"):
        perm = torch.randperm(n, generator=g)
        one, two = (0, V - 1) if kind == "bait_a" else (V - 1, 0)
        ids[perm[0]] = one
        ids[perm[1:3]] = two
    elif kind != "random":
        raise ValueError(kind)
    return ids.to(device)


# ------------------------------------------------------------------------------------------ the plan, restated
def maxc_for(cols):
    c = (cols + 511) // 512
    for m in (1, 2, 4, 8, 16):
        if c <= m:
            return m
    return -1


def bwd_waves(maxc):
    return 16 if maxc <= 2 else (8 if maxc == 4 else 4)


def bwd_blocks(rows, cols):
    nw = bwd_waves(maxc_for(cols))
    return min(256, (rows + nw - 1) // nw)


def nch_for(vocab, nt=256):
    per = (vocab // 8 + nt - 1) // nt
    for n in (2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64):
        if per <= n:
            return n
    return -1


# ------------------------------------------------------------------------------------------ RMSNorm
def ref_rmsnorm_fwd(x, w, eps, res=None):
    """y = xe rstd w, rstd = rsqrt(mean(xe^2) + eps), xe = bf16(x + res) (the rounded residual stream is part of the
    operation: it is what the next layer reads). cond: y |y|; rstd |rstd| (a sum of non-negative terms);
    residual_out |x| + |res|."""
    xe = x.double() if res is None else (x.double() + res.double()).to(BF).double()
    rstd = torch.rsqrt(xe.pow(2).mean(-1) + eps)
    y = xe * rstd[:, None] * w.double()
    out = {"y": (y, y.abs()), "rstd": (rstd, rstd.abs())}
    if res is not None:
        out["residual_out"] = (x.double() + res.double(), x.double().abs() + res.double().abs())
    return out


def restate_rmsnorm_fwd(x, w, eps, res=None, mut=None):
    """fp32: residual add rounded to bf16 before the statistic; each lane sums its 8-element vectors, then the wave;
    y = bf16(xe rstd w). mut: None | "tail" (the row's last 8-vector left out of the statistic) | "mean512" (mean
    over cols rounded up to 512) | "rstd_next" (row r uses the rstd of row r - 1 within a 4-row workgroup) |
    "res_unrounded" (statistic and y from the fp32 sum)."""
    rows, cols = x.shape
    xe = x.float()
    ro = None
    if res is not None:
        s32 = x.float() + res.float()
        ro = s32.to(BF)
        xe = s32 if mut == "res_unrounded" else ro.float()
    sq = xe * xe
    if mut == "tail":
        sq = sq[:, :cols - 8]
    pad = (-sq.shape[1]) % 512
    lanes = torch.nn.functional.pad(sq, (0, pad)).view(rows, -1, 64, 8).permute(0, 2, 1, 3).reshape(rows, 64, -1)
    ss = lanes.sum(-1).sum(-1)
    n = float((cols + 511) // 512 * 512) if mut == "mean512" else float(cols)
    rstd = torch.rsqrt(ss / n + eps)
    use = rstd
    if mut == "rstd_next":
        use = rstd.clone()
        idx = torch.arange(rows)
        src = torch.where(idx % 4 != 0, idx - 1, idx)
        use = rstd[src]
    y = (xe * use[:, None] * w.float()).to(BF)
    out = {"y": y, "rstd": rstd}
    if res is not None:
        out["residual_out"] = ro
    return out


def ref_rmsnorm_bwd(dy, x, w, rstd, dres=None, mode=0, g0=None, scale=1.0):
    """dx = rstd (g - xhat mean(g xhat)) [+ dres], g = dy w, xhat = x rstd (rstd as given: an input of the backward);
    dw = sum_rows dy xhat; mode 1: g0 + dw (bf16), mode 2: (g0 + dw) scale (fp32).
    cond: dx rs (|dy w| + |xhat| mean|dy w xhat|) [+ |dres|]; dw (|g0| + sum_rows |dy xhat|) scale."""
    d, xh = dy.double(), x.double() * rstd.double()[:, None]
    g = d * w.double()
    rs = rstd.double()[:, None]
    dx = rs * (g - xh * (g * xh).mean(-1, keepdim=True))
    cdx = rs * (g.abs() + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    if dres is not None:
        dx, cdx = dx + dres.double(), cdx + dres.double().abs()
    dw, cdw = (d * xh).sum(0), (d * xh).abs().sum(0)
    if mode:
        dw, cdw = dw + g0.double(), cdw + g0.double().abs()
    if mode == 2:
        dw, cdw = dw * scale, cdw * abs(scale)
    return {"dx": (dx, cdx), "dw": (dw, cdw)}


def dw_finish(t, mode, g0, scale, mode_arith=None):
    """The dw modes on the fp32 column sums t: 0 bf16(t); 1 bf16(g0 + t); 2 (g0 + t) scale in fp32. mode_arith: the
    arithmetic of another mode written into this mode's buffer (a mutant)."""
    a = mode if mode_arith is None else mode_arith
    if a == 0:
        v = t
    elif a == 1:
        v = (g0.float() + t).to(BF).float()
    else:
        v = (g0.float() + t) * scale
    return v.to(BF) if mode in (0, 1) else v.float()


def dw_reduce_separate(part):
    """rmsnorm_dw_kernel's order over the partial rows [nb, cols] (fp32): 8 slices, slice s sums rows s, s + 8, ...
    one after the other; then the slices in order."""
    nb, cols = part.shape
    red = torch.zeros(8, cols, dtype=F32, device=part.device)
    for b in range(nb):
        red[b % 8] += part[b]
    t = red[0].clone()
    for s in range(1, 8):
        t += red[s]
    return t


def dw_reduce_chained(part, nw):
    """The chained form's order (rmsnorm_bwd_kernel with DwPrev) in a launch of nw waves: nw * 4 row groups, group g
    sums rows g, g + 4 nw, ... one after the other; a wave's four groups as (g0 + g1) + (g2 + g3); then the waves in
    order."""
    nb, cols = part.shape
    ng = nw * 4
    grp = torch.zeros(ng, cols, dtype=F32, device=part.device)
    for b in range(nb):
        grp[b % ng] += part[b]
    wave = (grp[0::4] + grp[1::4]) + (grp[2::4] + grp[3::4])
    t = torch.zeros(cols, dtype=F32, device=part.device)
    for k in range(nw):
        t += wave[k]
    return t


def restate_rmsnorm_bwd(dy, x, w, rstd, dres=None, mode=0, g0=None, scale=1.0, mut=None):
    """fp32. dx = bf16(rstd (dy w - xhat dot) [+ dres]), dot = sum(dy w xhat) / cols. dw in the kernel's order: a wave
    adds its rows (one per pass) one after the other, the workgroup adds its waves in order (one fp32 partial row per
    workgroup), rmsnorm_dw_kernel adds the partial rows (dw_reduce_separate). Returns dx, dw and the partial rows.
    mut: None | "part_missing" (the last workgroup's partial row left out) | "mode1_as_2" (mode 1 arithmetic under
    mode 2)."""
    rows, cols = x.shape
    nw, nb = bwd_waves(maxc_for(cols)), bwd_blocks(rows, cols)
    rs = rstd.float()[:, None]
    d, xh, wf = dy.float(), x.float() * rs, w.float()
    dot = (d * wf * xh).sum(-1, keepdim=True) / float(cols)
    v = rs * (d * wf - xh * dot)
    if dres is not None:
        v = v + dres.float()
    c = d * xh
    stride = nb * nw
    passes = (rows + stride - 1) // stride
    c = torch.nn.functional.pad(c, (0, 0, 0, passes * stride - rows)).view(passes, nb, nw, cols)
    wave = torch.zeros(nb, nw, cols, dtype=F32, device=x.device)
    for p in range(passes):
        wave += c[p]
    part = torch.zeros(nb, cols, dtype=F32, device=x.device)
    for k in range(nw):
        part += wave[:, k]
    t = dw_reduce_separate(part[:-1] if mut == "part_missing" else part)
    dw = dw_finish(t, mode, g0, scale, mode_arith=1 if mut == "mode1_as_2" else None)
    return {"dx": v.to(BF), "dw": dw, "part": part}


def ref_dw_reduce(part, mode=0, g0=None, scale=1.0):
    """The dw reduction alone, from given fp32 partial rows: sum_b part[b], then the mode. cond (|g0| + sum|part|)
    scale."""
    t, c = part.double().sum(0), part.double().abs().sum(0)
    if mode:
        t, c = t + g0.double(), c + g0.double().abs()
    if mode == 2:
        t, c = t * scale, c * abs(scale)
    return {"dw": (t, c)}


# ------------------------------------------------------------------------------------------ RoPE
def ref_rope(x, cos, sin, conjugate=False):
    """fp64 rotate-half RoPE of x [B, S, H, D] by the bf16 tables [S, D/2]. cond |x1 c| + |x2 s| (and the other
    pair): the two products each output adds."""
    out = H.rope_fused(x.double(), cos.double(), sin.double(), conjugate)
    h = x.shape[-1] // 2
    c, s = cos.double()[None, :x.shape[1], None, :h].abs(), sin.double()[None, :x.shape[1], None, :h].abs()
    a, b = x.double()[..., :h].abs(), x.double()[..., h:].abs()
    return {"out": (out, torch.cat((a * c + b * s, b * c + a * s), -1))}


def restate_rope(x, cos, sin, conjugate=False, mut=None):
    """fp32, both products rounded before the sum, one rounding of the result: the arithmetic H.rope_fused states
    (bit-equal to it). mut: None | "no_conj" (conjugate ignored) | "flat_pos" (position = flat (b, s) row index for
    batch > 0: what a wrong index division gives; tables must have B S rows) | "fma" (the second product contracted
    into a fused multiply-add)."""
    B, S, _, D = x.shape
    h = D // 2
    pos = torch.arange(S, device=x.device).repeat(B, 1)
    if mut == "flat_pos":
        pos = pos + torch.arange(B, device=x.device)[:, None] * S
    c, s = cos.float()[pos, :h][:, :, None, :], sin.float()[pos, :h][:, :, None, :]
    if conjugate and mut != "no_conj":
        s = -s
    a, b = x.float()[..., :h], x.float()[..., h:]
    if mut == "fma":  # fma(a, c, -(b s)) and fma(b, c, a s): the first product unrounded (exact in fp64)
        o1 = (a.double() * c.double() - (b * s).double()).float()
        o2 = (b.double() * c.double() + (a * s).double()).float()
    else:
        o1, o2 = a * c - b * s, b * c + a * s
    return {"out": torch.cat((o1, o2), -1).to(BF)}


# ------------------------------------------------------------------------------------------ SwiGLU
def ref_swiglu_fwd(g, u):
    """h = g sigma(g) u. cond |h| (1 + |g| (1 - sigma)): the relative sensitivity of sigma to the argument of its
    exp."""
    gd, ud = g.double(), u.double()
    sg = torch.sigmoid(gd)
    h = gd * sg * ud
    return {"h": (h, h.abs() * (1 + gd.abs() * (1 - sg)))}


def ref_swiglu_bwd(dh, g, u):
    """du = dh g sigma, dg = dh u sigma (1 + g (1 - sigma)). cond: du |du| (1 + |g| (1 - sigma));
    dg |dh u| sigma (1 + |g| (1 - sigma))^2: the two terms the kernel adds, times the exp's sensitivity."""
    d, gd, ud = dh.double(), g.double(), u.double()
    sg = torch.sigmoid(gd)
    k = 1 + gd.abs() * (1 - sg)
    du = d * gd * sg
    dg = d * ud * sg * (1 + gd * (1 - sg))
    return {"dg": (dg, (d * ud).abs() * sg * k * k), "du": (du, du.abs() * k)}


def _sig32(gf):
    """fp32 sigma = 1 / (1 + exp(-g)); from g = -87 down (where exp(-g) nears the fp32 overflow and the quotient would
    flush to 0 while silu(g) u is still a normal number) e^g, as 2^64 e^g scaled back: the kernel's formulation."""
    tail = torch.exp2(gf * LOG2E + 64.0) * 2.0 ** -64
    return torch.where(gf < -87.0, tail, 1.0 / (1.0 + torch.exp(-gf)))


def restate_swiglu_fwd(g, u, mut=None):
    """fp32: h = bf16(g sigma u), sigma as _sig32. mut: "halves" (gate and up swapped)."""
    if mut == "halves":
        g, u = u, g
    gf = g.float()
    return {"h": (gf * _sig32(gf) * u.float()).to(BF)}


def restate_swiglu_bwd(dh, g, u, mut=None):
    """fp32, one rounding per output. mut: "no_term" (dg without g (1 - sigma)) | "swapped" (du and dg swapped)."""
    d, gf, uf = dh.float(), g.float(), u.float()
    sg = _sig32(gf)
    du = d * (gf * sg)
    dg = d * uf * sg * ((1.0 + gf * (1.0 - sg)) if mut != "no_term" else 1.0)
    if mut == "swapped":
        dg, du = du, dg
    return {"dg": dg.to(BF), "du": du.to(BF)}


# ------------------------------------------------------------------------------------------ cross-entropy
def _valid(t, V):
    return (t != IGNORE) & (t >= 0) & (t < V)


def ref_ce(x, t, gscale=1.0, lse_in=None):
    """lse = m + log s, s = sum exp(x - m); loss = lse - x[t] (0 for an ignored row); dlogits = g (p - onehot(t)),
    p = exp(x - lse), 0 for an ignored row. lse_in: the backward's lse input (dlogits
    from it instead of this function's lse).
    cond: lse 1 + |m| + |log s|; loss that + |x[t]|; dlogits g (p + onehot) (1 + |x - lse|)."""
    xd = x.double()
    rows, V = xd.shape
    m = xd.amax(-1)
    s = torch.exp(xd - m[:, None]).sum(-1)
    lse = m + torch.log(s)
    clse = 1 + m.abs() + torch.log(s).abs()
    ok = _valid(t, V)
    tc = torch.where(ok, t, torch.zeros_like(t))
    xt = xd.gather(1, tc[:, None])[:, 0]
    loss = torch.where(ok, lse - xt, torch.zeros_like(lse))
    closs = torch.where(ok, clse + xt.abs(), torch.zeros_like(lse))
    l = lse if lse_in is None else lse_in.double()
    p = torch.exp(xd - l[:, None])
    oh = torch.zeros_like(xd)
    oh[torch.arange(rows, device=x.device)[ok], tc[ok]] = 1.0
    g = torch.where(ok, gscale, 0.0).double()[:, None]
    dl = g * (p - oh)
    cdl = g.abs() * (p + oh) * (1 + (xd - l[:, None]).abs())
    return {"lse": (lse, clse), "loss": (loss, closs), "dlogits": (dl, cdl)}


def ref_ce_mean(x, t):
    """fp64 mean loss over the rows that are not ignored."""
    loss = ref_ce(x, t)["loss"][0]
    return float(loss.sum() / max(1, int(_valid(t, x.shape[1]).sum())))


def _fma32(a, b, c):
    """fp32 fused multiply-add: a (fp32 holding bf16 values) times the fp32 constant b is exact in fp64, so the sum
    is rounded once (a second rounding from fp64 to fp32 aside)."""
    return (a.double() * float(torch.tensor(b, dtype=F32)) + c.double()).float()


def restate_ce(x, t, gscale=1.0, form="fwd_grad", mut=None, nt=256):
    """fp32, in the kernels' formulation. m = max; s = sum exp2(x log2e - m log2e); lse = m + log s; loss = lse - x[t].
    form "fwd_grad": dlogits = bf16(exp(x - lse) g), the target's element rewritten as bf16(exp(x[t] - lse) g - g)
    (the kernel folds lse and g into one exponent offset, c2 = -lse log2e + log2 g, whose rounding at the magnitude
    of lse log2e the K term has to absorb on a nearly one-hot target; the restatement takes the difference first);
    form "bwd": bf16((exp(x - lse) - onehot) g).
    mut: "t_plus_1" (one-hot at t + 1) | "ignored_grad" (an ignored row treated as target 0) | "max_first_pass" (the
    row maximum over the first nt * 8 columns only) | "tail_chunk" (the last 8-vector of the vocabulary skipped in the
    sum and left unwritten (zero))."""
    xf = x.float()
    rows, V = xf.shape
    if mut == "ignored_grad":
        t = torch.where(t == IGNORE, torch.zeros_like(t), t)
    ok = _valid(t, V)
    tc = torch.where(ok, t, torch.zeros_like(t))
    m = (xf[:, :nt * 8] if mut == "max_first_pass" else xf).amax(-1)
    if form == "fwd_grad":  # exp2(fma(x, log2e, -m log2e)); the plain forward: exp2((x - m) log2e)
        e = torch.exp2(_fma32(xf, LOG2E, (-m * LOG2E)[:, None]))
    else:
        e = torch.exp2((xf - m[:, None]) * LOG2E)
    if mut == "tail_chunk":
        e = e[:, :V - 8]
    s = e.sum(-1)
    lse = m + torch.log(s)
    xt = xf.gather(1, tc[:, None])[:, 0]
    loss = torch.where(ok, lse - xt, torch.zeros_like(lse))
    g = torch.where(ok, float(gscale), 0.0).float()
    hot = tc + 1 if mut == "t_plus_1" else tc
    hot_ok = ok & (hot < V)
    r = torch.arange(rows, device=x.device)
    if form == "fwd_grad":
        dl = (torch.exp(xf - lse[:, None]) * g[:, None]).to(BF)
        fix = (torch.exp(xf[r, hot.clamp_max(V - 1)] - lse) * g - g).to(BF)
        dl[r[hot_ok], hot[hot_ok]] = fix[hot_ok]
    else:
        p = torch.exp(xf - lse[:, None])
        p[r[hot_ok], hot[hot_ok]] -= 1.0
        dl = (p * g[:, None]).to(BF)
    if mut == "tail_chunk":
        dl[:, V - 8:] = 0
    return {"lse": lse, "loss": loss, "dlogits": dl}


def fwd_grad_target(x, t, lse, gscale):
    """The target column of pico_cross_entropy_fwd_grad recomputed in the kernel's own formulation from the lse the
    kernel returned: bf16(exp2(fma(x[t], log2e, c2)) - g), c2 = fma(-lse, log2e, log2 g). Returns (rows, values) for
    the rows that are not ignored. The kernel's exp2 / log2 are 1-ulp hardware functions, so the comparison allows
    one bf16 ulp."""
    ok = _valid(t, x.shape[1])
    r = torch.arange(len(t), device=x.device)[ok]
    g = torch.full((len(r),), float(gscale), dtype=F32, device=x.device)
    c2 = _fma32(-lse.float()[ok], LOG2E, torch.log2(g))
    xt = x.float()[r, t[ok]]
    return r, (torch.exp2(_fma32(xt, LOG2E, c2)) - g).to(BF)


def restate_ce_vp(x, t, splits, gscale=1.0, mut=None):
    """The vocab-parallel form over column shards [splits[i], splits[i + 1]): per shard (m, s, xt), combined in rank
    order (M = max m_r, S = sum s_r exp(m_r - M), lse = M + log S, loss = lse - sum xt_r), and each shard's
    dlogits = bf16((exp2(x log2e - lse log2e) - [j + start == t]) g); zeros for an ignored row.
    mut: "wrong_shard" (the one-hot applied with the local index on every shard: the start offset forgotten)."""
    xf = x.float()
    rows, V = xf.shape
    ok = _valid(t, V)
    parts = []
    for a, b in zip(splits[:-1], splits[1:]):
        sh = xf[:, a:b]
        m = sh.amax(-1)
        s = torch.exp2(_fma32(sh, LOG2E, (-m * LOG2E)[:, None])).sum(-1)
        tl = t - a
        here = (tl >= 0) & (tl < b - a)
        xt = torch.where(here, sh.gather(1, tl.clamp(0, b - a - 1)[:, None])[:, 0], torch.zeros_like(m))
        parts.append((m, s, xt))
    M = torch.stack([p[0] for p in parts]).amax(0)
    S = torch.zeros_like(M)
    XT = torch.zeros_like(M)
    for m, s, xt in parts:
        S = S + s * torch.exp(m - M)
        XT = XT + xt
    lse = M + torch.log(S)
    loss = torch.where(ok, lse - XT, torch.zeros_like(lse))
    dl = torch.zeros(rows, V, dtype=BF, device=x.device)
    r = torch.arange(rows, device=x.device)
    for a, b in zip(splits[:-1], splits[1:]):
        p = torch.exp2(_fma32(xf[:, a:b], LOG2E, (-lse * LOG2E)[:, None]))
        tl = t if mut == "wrong_shard" else t - a
        here = ok & (tl >= 0) & (tl < b - a)
        p[r[here], tl[here]] -= 1.0
        dl[:, a:b] = (p * float(gscale)).to(BF) * ok[:, None]
    return {"lse": lse, "loss": loss, "dlogits": dl, "parts": parts}


def ref_scale(x, s):
    """x s with s the upstream gradient rounded to bf16. cond |x s|."""
    v = x.double() * float(torch.tensor(s).to(BF))
    return {"dx": (v, v.abs())}


def restate_scale(x, s):
    return {"dx": (x.float() * torch.tensor(s).to(BF).float()).to(BF)}


# ------------------------------------------------------------------------------------------ embedding backward
def ref_embedding(g0, ids, dy, scale):
    """grad[id] = (g0[id] + sum of dy over the positions holding id) scale on touched rows; other rows unchanged.
    cond (|g0| + sum|dy|) |scale| on touched rows, 0 elsewhere (they must be bit-identical)."""
    acc = torch.zeros(g0.shape, dtype=F64, device=g0.device).index_add_(0, ids, dy.double())
    cacc = torch.zeros(g0.shape, dtype=F64, device=g0.device).index_add_(0, ids, dy.double().abs())
    touched = torch.zeros(g0.shape[0], dtype=torch.bool, device=g0.device)
    touched[ids] = True
    ref = torch.where(touched[:, None], (g0.double() + acc) * scale, g0.double())
    cond = torch.where(touched[:, None], (g0.double().abs() + cacc) * abs(scale), torch.zeros_like(acc))
    return {"grad": (ref, cond)}


def restate_embedding(g0, ids, dy, scale, mut=None):
    """fp32: a run's dy rows added in position order in blocks of 64 positions (each block from zero, the block sums
    added in order: the kernel's order), then (g0 + sum) scale rounded once to the gradient's dtype. mut: "drop_last" (the last position of every run left out) | "scale_untouched"
    (every row scaled) | "cols_2048" (columns >= 2048 not updated)."""
    order = torch.sort(ids, stable=True)
    sid, pos = order.values, order.indices
    uniq, counts = torch.unique_consecutive(sid, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    if mut == "drop_last":
        counts = counts - 1
    acc = torch.zeros(len(uniq), g0.shape[1], dtype=F32, device=g0.device)
    blk = torch.zeros_like(acc)
    last = int(counts.max()) if len(uniq) else 0
    for k in range(last):  # the k-th position of every run that has one
        live = counts > k
        blk[live] += dy[pos[start[live] + k]].float()
        if (k + 1) % 64 == 0 or k + 1 == last:
            acc += blk
            blk.zero_()
    out = (g0.float() * scale).to(g0.dtype) if mut == "scale_untouched" else g0.clone()
    v = ((g0[uniq].float() + acc) * scale).to(g0.dtype)
    if mut == "cols_2048":
        v[:, 2048:] = g0[uniq, 2048:]
    out[uniq] = v
    return {"grad": out}


# ------------------------------------------------------------------------------------------ GPU case tables
RMS_FWD_COLS = (8, 64, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 8192)  # both ends of every MAXC
RMS_FWD_ROWS = (1, 3, 5)
RMS_FWD_T = ((32, 1024), (64, 2048))
RMS_BWD_COLS = (64, 512, 520, 1024, 1032, 2048, 2056, 4096)


def rms_bwd_rows(cols):
    """3 (fewer rows than waves: waves with no row) and 256 NW + NW + 1 (every workgroup runs a ragged second pass)."""
    nw = bwd_waves(maxc_for(cols))
    return (3, 256 * nw + nw + 1)


# chained dw: (rows, cols of the launch, prev_cols); prev_nb in CHAIN_NB, every prev_mode, reduce_own 0 / 1
RMS_CHAIN = (
    (512, 512, 512),     # 16 waves, nb 32: cpw exactly 16
    (512, 512, 520),     # cpw 17: the fallback launch
    (1024, 1024, 1024),  # 16 waves at MAXC 2, nb 64
    (512, 2048, 1024),   # 1024 columns into a 2048-column launch (8 waves)
    (4096, 512, 4096),   # 4096 columns into a 512-column launch
    (128, 4096, 512),    # 4 waves
)
CHAIN_NB = (1, 37, 256)

ROPE_D, ROPE_H, ROPE_S, ROPE_B = (16, 32, 64, 128, 256), (1, 3, 32), (1, 37), (1, 3)
ROPE_BIG = (4, 2056, 32, 128)  # 2,105,344 vectors: a second trip of the grid-stride loop

# SwiGLU: (rows, cols, fused halves (in_stride = 2 cols), base shift in elements)
SWIGLU_CASES = ([(r, c, f, 0) for c in (8, 4096) for r in (1, 5) for f in (False, True)]
                + [(r, c, f, 0) for c in (1, 7, 12, 4099) for r in (1, 5) for f in (False, True)]
                + [(5, 4096, False, 1), (5, 8, True, 1)])               # unaligned base: the scalar fallback
SWIGLU_BIG = ((2056, 4096, False, 0), (1, 4096 * 256 + 3, False, 0))    # second loop trip: vector, scalar
SWIGLU_T = ((64, 64), (64, 128), (128, 192))

CE_FIRST = (8, 4104, 6152, 8200, 12296, 16392, 24584, 32776, 49160, 65544, 98312)  # first vocab of every NCH
CE_VOCABS_256 = tuple(sorted(set(CE_FIRST + tuple(v - 8 for v in CE_FIRST[1:]) + (131072, 128256))))
CE_VOCABS_512 = tuple(sorted(set(tuple(2 * v - 8 if v > 8 else 8 for v in CE_FIRST) + tuple(2 * (v - 8) for v in CE_FIRST[1:])
                                 + (262144, 128256))))
CE_GSCALE = 0.25 / 3
SCALE_N = 8 * 4096 * 256 + 8 * 5 + 3

EMB_DIMS = (8, 2048, 2056, 4096)
EMB_N = (1, 8192, 8193)
EMB_V = 512


def plan_cases():
    """The argument strings of tests/rowwise_plan_check.cpp for every case of the tables above."""
    c = [f"rms_fwd:{r}:{k}" for k in RMS_FWD_COLS for r in RMS_FWD_ROWS]
    c += [f"rms_bwd:{r}:{k}:{res}" for k in RMS_BWD_COLS for r in rms_bwd_rows(k) for res in (0, 1)]
    c += [f"rms_chain:{r}:{k}:{p}" for r, k, p in RMS_CHAIN]
    c += [f"ce:256:{v}" for v in CE_VOCABS_256] + [f"ce:512:{v}" for v in CE_VOCABS_512]
    for r, k, fused, shift in SWIGLU_CASES + list(SWIGLU_BIG):
        st = 2 * k if fused else k
        c.append(f"swiglu:{r}:{k}:{st}:{k}:{2 * shift}")
    c += [f"rope:{b}:{s}:{h}:{d}" for d in ROPE_D for h in ROPE_H for s in ROPE_S for b in ROPE_B]
    c += ["rope:%d:%d:%d:%d" % ROPE_BIG, f"scale:{SCALE_N}"] + [f"emb:{d}" for d in EMB_DIMS]
    return c


# ------------------------------------------------------------------------------------------ launches (HIP device)
def _lib():
    from picotron_amd import _lib as L
    return L, L.load()


def _run(G, fn, op, written=()):
    L, _ = _lib()
    G.arm()
    L.check(fn(), op)
    torch.cuda.synchronize()
    G.check(written=written)


def launch_rmsnorm_fwd(x, w, eps, res=None, want_res_out=True, transposed=False):
    """pico_rmsnorm_fwd (or _fwd_t) on guarded buffers. Returns {"y", "rstd", "residual_out", "y_t"}."""
    L, lib = _lib()
    rows, cols = x.shape
    G = A.Guards(x.device)
    xg, wg = G.mat("x", rows, cols, data=x), G.mat("w", 1, cols, data=w)
    rg = G.mat("res", rows, cols, data=res) if res is not None else None
    y, rstd = G.mat("y", rows, cols), G.mat("rstd", 1, rows, dtype=F32)
    ro = G.mat("residual_out", rows, cols) if res is not None and want_res_out else None
    st = L.stream_of(x)
    if transposed:
        yt = G.mat("y_t", cols, rows, ld=rows + 8)
        _run(G, lambda: lib.pico_rmsnorm_fwd_t(L.ptr(xg), L.ptr(rg), L.ptr(wg), L.ptr(y), L.ptr(ro), L.ptr(rstd),
                                               L.ptr(yt), yt.stride(0), rows, cols, eps, st), "pico_rmsnorm_fwd_t")
    else:
        yt = None
        _run(G, lambda: lib.pico_rmsnorm_fwd(L.ptr(xg), L.ptr(rg), L.ptr(wg), L.ptr(y), L.ptr(ro), L.ptr(rstd), rows,
                                             cols, eps, st), "pico_rmsnorm_fwd")
    out = {"y": y, "rstd": rstd[0], "y_t": yt}
    if ro is not None:
        out["residual_out"] = ro
    return out


def launch_rmsnorm_bwd(dy, x, w, rstd, dres=None, mode=0, g0=None, scale=1.0, reduce_own=1, prev=None):
    """pico_rmsnorm_bwd_chain on guarded buffers (workspace sized by pico_rmsnorm_bwd_workspace_bytes). prev: optional
    {"part" fp32 [nb, cols], "mode", "g0", "scale"}: a previous call's partial rows to reduce in this launch.
    Returns {"dx", "dw" (None without reduce_own), "part" (this launch's partial rows), "prev_dw"}."""
    L, lib = _lib()
    rows, cols = x.shape
    G = A.Guards(x.device)
    dyg, xg, wg = G.mat("dy", rows, cols, data=dy), G.mat("x", rows, cols, data=x), G.mat("w", 1, cols, data=w)
    rsg = G.mat("rstd", 1, rows, dtype=F32, data=rstd)
    drg = G.mat("dres", rows, cols, data=dres) if dres is not None else None
    dx = G.mat("dx", rows, cols)
    dwt = F32 if mode == 2 else BF
    dw = G.mat("dw", 1, cols, dtype=dwt, data=g0 if mode else None, inout=bool(mode)) if reduce_own else None
    nb = lib.pico_rmsnorm_bwd_partial_rows(rows, cols)
    assert lib.pico_rmsnorm_bwd_workspace_bytes(rows, cols) == nb * cols * 4
    ws = G.mat("workspace", nb, cols, dtype=F32)
    pp = pdw = None
    pn = pc = pm = 0
    ps = 1.0
    if prev is not None:
        pn, pc = prev["part"].shape
        pm, ps = prev["mode"], prev["scale"]
        pp = G.mat("prev_part", pn, pc, dtype=F32, data=prev["part"])
        pdw = G.mat("prev_dw", 1, pc, dtype=F32 if pm == 2 else BF, data=prev["g0"] if pm else None, inout=bool(pm))
    st = L.stream_of(x)
    _run(G, lambda: lib.pico_rmsnorm_bwd_chain(L.ptr(dyg), L.ptr(drg), L.ptr(xg), L.ptr(wg), L.ptr(rsg), L.ptr(dx),
                                               L.ptr(dw), mode, scale, L.ptr(ws), rows, cols, reduce_own, L.ptr(pp), pn,
                                               pc, L.ptr(pdw), pm, ps, st), "pico_rmsnorm_bwd_chain")
    return {"dx": dx, "dw": dw[0] if dw is not None else None, "part": ws, "prev_dw": pdw[0] if pdw is not None else None}


def launch_dw_reduce(part, mode=0, g0=None, scale=1.0):
    L, lib = _lib()
    nb, cols = part.shape
    G = A.Guards(part.device)
    pg = G.mat("part", nb, cols, dtype=F32, data=part)
    dw = G.mat("dw", 1, cols, dtype=F32 if mode == 2 else BF, data=g0 if mode else None, inout=bool(mode))
    _run(G, lambda: lib.pico_rmsnorm_dw_reduce(L.ptr(pg), nb, cols, L.ptr(dw), mode, scale, L.stream_of(part)),
         "pico_rmsnorm_dw_reduce")
    return dw[0]


def launch_rope(x, cos, sin, conjugate, alias=False):
    """pico_rope on guarded buffers: x a head slice of a wider buffer (one guard head), out with three guard heads
    (other strides), the tables with a padded row stride; alias: out == x (both the strided slice)."""
    L, lib = _lib()
    B, S, Hh, D = x.shape
    G = A.Guards(x.device)
    xg = G.bshd("x", B, S, Hh, D, data=x)
    og = xg if alias else G.bshd("out", B, S, Hh, D, pad_heads=3)
    cg, sg = G.table("cos", cos), G.table("sin", sin)
    _run(G, lambda: lib.pico_rope(L.ptr(xg), L.ptr(og), L.ptr(cg), L.ptr(sg), B, S, Hh, D, L.i64x3(xg.stride()[:3]),
                                  L.i64x3(og.stride()[:3]), cg.stride(0), 1 if conjugate else 0, L.stream_of(x)),
         "pico_rope", written=("x",) if alias else ())
    return {"out": og}


def launch_swiglu(g, u, dh=None, fused=False, shift=0):
    """pico_swiglu_fwd (dh None) or _bwd on guarded buffers. fused: gate | up (and dgate | dup) are the two column
    halves of one [rows, 2 cols] buffer; otherwise separate row-contiguous buffers. shift: base offset in elements of
    every buffer (1: the unaligned scalar fallback)."""
    L, lib = _lib()
    rows, cols = g.shape
    G = A.Guards(g.device)
    if fused:
        gu = G.mat("gate_up", rows, 2 * cols, data=torch.cat((g, u), 1), shift=shift)
        gg, ug, ist = gu[:, :cols], gu[:, cols:], 2 * cols
    else:
        gg, ug, ist = G.mat("gate", rows, cols, data=g, shift=shift), G.mat("up", rows, cols, data=u, shift=shift), cols
    st = L.stream_of(g)
    if dh is None:
        h = G.mat("h", rows, cols, shift=shift)
        _run(G, lambda: lib.pico_swiglu_fwd(L.ptr(gg), L.ptr(ug), L.ptr(h), rows, cols, ist, cols, st),
             "pico_swiglu_fwd")
        return {"h": h}
    dhg = G.mat("dh", rows, cols, data=dh, shift=shift)
    if fused:
        d2 = G.mat("dgate_dup", rows, 2 * cols, shift=shift)
        dg, du = d2[:, :cols], d2[:, cols:]
    else:
        dg, du = G.mat("dg", rows, cols, shift=shift), G.mat("du", rows, cols, shift=shift)
    _run(G, lambda: lib.pico_swiglu_bwd(L.ptr(dhg), L.ptr(gg), L.ptr(ug), L.ptr(dg), L.ptr(du), rows, cols, ist, cols,
                                        st), "pico_swiglu_bwd")
    return {"dg": dg, "du": du}


def launch_swiglu_t(g, u):
    L, lib = _lib()
    rows, cols = g.shape
    G = A.Guards(g.device)
    gu = G.mat("gate_up", rows, 2 * cols, data=torch.cat((g, u), 1))
    h, ht = G.mat("h", rows, cols, ld=cols + 8), G.mat("h_t", cols, rows, ld=rows + 8)
    _run(G, lambda: lib.pico_swiglu_fwd_t(L.ptr(gu[:, :cols]), L.ptr(gu[:, cols:]), L.ptr(h), L.ptr(ht), rows, cols,
                                          2 * cols, h.stride(0), ht.stride(0), L.stream_of(g)), "pico_swiglu_fwd_t")
    return {"h": h, "h_t": ht}


def _ce_common(G, x, t, pad=8):
    rows, V = x.shape
    return G.mat("target", 1, rows, dtype=torch.int64, data=t), rows, V, V + pad


def launch_ce_fwd(x, t):
    L, lib = _lib()
    G = A.Guards(x.device)
    tg, rows, V, ld = _ce_common(G, x, t)
    xg = G.mat("logits", rows, V, data=x, ld=ld)
    lse, loss = G.mat("lse", 1, rows, dtype=F32), G.mat("loss", 1, rows, dtype=F32)
    _run(G, lambda: lib.pico_cross_entropy_fwd(L.ptr(xg), ld, L.ptr(tg), L.ptr(lse), L.ptr(loss), rows, V, IGNORE,
                                               L.stream_of(x)), "pico_cross_entropy_fwd")
    return {"lse": lse[0], "loss": loss[0]}


def launch_ce_bwd(x, t, lse, gscale):
    L, lib = _lib()
    G = A.Guards(x.device)
    tg, rows, V, ld = _ce_common(G, x, t)
    xg = G.mat("logits", rows, V, data=x, ld=ld)
    lg = G.mat("lse", 1, rows, dtype=F32, data=lse)
    gs = G.mat("gscale", 1, 1, dtype=F32, data=torch.tensor([gscale], dtype=F32))
    dl = G.mat("dlogits", rows, V, ld=ld + 8)
    _run(G, lambda: lib.pico_cross_entropy_bwd(L.ptr(xg), ld, L.ptr(tg), L.ptr(lg), L.ptr(gs), L.ptr(dl), ld + 8, rows,
                                               V, IGNORE, L.stream_of(x)), "pico_cross_entropy_bwd")
    return {"dlogits": dl}


def launch_ce_fwd_grad(x, t, gscale):
    L, lib = _lib()
    G = A.Guards(x.device)
    tg, rows, V, ld = _ce_common(G, x, t)
    xg = G.mat("logits", rows, V, data=x, ld=ld, inout=True)
    lse, loss = G.mat("lse", 1, rows, dtype=F32), G.mat("loss", 1, rows, dtype=F32)
    gs = G.mat("gscale", 1, 1, dtype=F32, data=torch.tensor([gscale], dtype=F32))
    _run(G, lambda: lib.pico_cross_entropy_fwd_grad(L.ptr(xg), ld, L.ptr(tg), L.ptr(lse), L.ptr(loss), L.ptr(gs), rows,
                                                    V, IGNORE, L.stream_of(x)), "pico_cross_entropy_fwd_grad")
    return {"lse": lse[0], "loss": loss[0], "dlogits": xg}


def launch_ce_vp(x, t, splits, gscale, inplace):
    """pico_ce_vp_partial per shard, _combine over the planes, _grad per shard, all on guarded buffers."""
    L, lib = _lib()
    rows, V = x.shape
    tp = len(splits) - 1
    st = L.stream_of(x)
    G = A.Guards(x.device)
    tg = G.mat("target", 1, rows, dtype=torch.int64, data=t)
    shards = [G.mat(f"shard{i}", rows, b - a, data=x[:, a:b], ld=b - a + 8, inout=inplace)
              for i, (a, b) in enumerate(zip(splits[:-1], splits[1:]))]
    parts = G.mat("parts", tp, 3 * rows, dtype=F32)
    lse, loss = G.mat("lse", 1, rows, dtype=F32), G.mat("loss", 1, rows, dtype=F32)
    gs = G.mat("gscale", 1, 1, dtype=F32, data=torch.tensor([gscale], dtype=F32))
    outs = shards if inplace else [G.mat(f"dshard{i}", rows, b - a, ld=b - a + 16)
                                   for i, (a, b) in enumerate(zip(splits[:-1], splits[1:]))]

    def go():
        for i, (a, b) in enumerate(zip(splits[:-1], splits[1:])):
            rc = lib.pico_ce_vp_partial(L.ptr(shards[i]), shards[i].stride(0), L.ptr(tg), L.ptr(parts[i]), rows, b - a, a,
                                        V, IGNORE, st)
            if rc:
                return rc
        rc = lib.pico_ce_vp_combine(L.ptr(parts), tp, L.ptr(tg), rows, V, IGNORE, L.ptr(lse), L.ptr(loss), st)
        if rc:
            return rc
        for i, (a, b) in enumerate(zip(splits[:-1], splits[1:])):
            rc = lib.pico_ce_vp_grad(L.ptr(shards[i]), shards[i].stride(0), L.ptr(tg), L.ptr(lse), L.ptr(gs),
                                     L.ptr(outs[i]), outs[i].stride(0), rows, b - a, a, V, IGNORE, st)
            if rc:
                return rc
        return 0
    _run(G, go, "pico_ce_vp")
    return {"lse": lse[0], "loss": loss[0], "dlogits": torch.cat(outs, 1)}


def launch_scale(x, up):
    """pico_ce_scale_grad: x (bf16, flat) *= up (a 0-dim fp32 or bf16 tensor), in place."""
    L, lib = _lib()
    G = A.Guards(x.device)
    xg = G.mat("dx", 1, x.numel(), data=x, inout=True)
    ug = G.mat("upstream", 1, 1, dtype=up.dtype, data=up.reshape(1))
    flag = G.mat("nonunit", 1, 1, dtype=torch.int32, data=torch.zeros(1, dtype=torch.int32), inout=True)
    _run(G, lambda: lib.pico_ce_scale_grad(L.ptr(xg), x.numel(), L.ptr(ug), 1 if up.dtype == F32 else 0, L.ptr(flag),
                                           L.stream_of(x)), "pico_ce_scale_grad")
    return {"dx": xg[0], "nonunit": int(flag[0, 0])}


def launch_embedding(g0, ids, dy, scale):
    """pico_embedding_bwd on guarded buffers after the project's own sort (ops.sort_ids: pico_sort_ids up to 8192 ids,
    torch.sort beyond)."""
    from picotron_amd import ops
    L, lib = _lib()
    n, dim = dy.shape
    sid, spos = ops.sort_ids(ids, g0.shape[0])
    G = A.Guards(g0.device)
    sg = G.mat("sorted_ids", 1, n, dtype=torch.int64, data=sid)
    pg = G.mat("sorted_pos", 1, n, dtype=torch.int64, data=spos)
    dyg = G.mat("dy", n, dim, data=dy)
    gg = G.mat("grad", g0.shape[0], dim, dtype=g0.dtype, data=g0, inout=True)
    _run(G, lambda: lib.pico_embedding_bwd(L.ptr(sg), L.ptr(pg), L.ptr(dyg), L.ptr(gg), n, dim,
                                           1 if g0.dtype == F32 else 0, scale, L.stream_of(g0)), "pico_embedding_bwd")
    return {"grad": gg}
