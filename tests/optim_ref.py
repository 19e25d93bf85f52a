"""References, restatements, mutants, input sets, the tensor list and guarded launches for the whole-parameter-list
kernel tests (tests/test_optim_kernels_host.py, tests/test_optim_kernels_gpu.py): adamw.hip, grad_clip.hip, muon.hip,
dp_bucket.hip and optim_common.h. A plain helper module: no fixture, no conftest; plain torch on the CPU except the
launch helpers at the bottom, which need the library and a HIP device.

ref_*       fp64, the operation itself. Each returns {output: (reference, cond)} for rowwise_ref.elem_check
            (|got - ref| <= U |ref| + K 2^-23 cond + 2^-120; U = 2^-8 for a bf16 output, 0 for an fp32 one); the
            formula of cond is in each docstring. A rounding the operation *specifies* on the way (the fp32 main_grad
            rounded to bf16, CLIP's g = bf16(g coef), Muon's mul_ result, m' under u) is an input of the reference: it
            takes that value from the restatement (or from the kernel's own checked output), so a double rounding of
            an intermediate never shows as a whole bf16 step of the final result.
restate_*   the same operation at the kernel's own precision and order, written from the header comments of the .hip
            files. This is what "a correct kernel" means; the kernels' outputs calibrate nothing.
variant     the build leaves fp contraction to the compiler, so an fp32 `x + y * z` may be one fma. Each restatement
            with such a site takes a variant, one bool per site (True: contracted; _fma32 is exact). The tests require
            one and the same variant for every element of every tensor of a launch, vector and scalar path alike.
            adam_elem has no fp32 site (its last line is a quotient), but its double expressions p - lr_wd p,
            b1 m + (1 - b1) g and b2 v + (1 - b2) g g may each be fused: variant = (decay, m, v), see adam_elem.
undecided   adam_elem rounds each double expression once to fp32. Fused or not, the double value moves by at most ERR64
            = 4 * 2^-53 times the sum of the magnitudes of the expression's terms (at most three double operations,
            2^-53 relative each; 4 for room), so only an element whose double value lies within that term of an fp32
            rounding boundary (the midpoint of two adjacent fp32 values) can take either neighbour. Exactly those
            elements are marked ("sensitive"). They are not rare where the expected 2^-24 would have them: with fp32
            moments and b1 = 0.9 the real value (9 m + g) / 10 terminates in binary for one element in five and is
            then often an exact 25-bit value, a tie that only the rounding of the constants breaks: about 5 % of the
            master form's m. So they are not exempted: each is re-evaluated exactly (Fractions) under the variant, and
            the "undecided" set, the elements left out of the bit comparison, is empty. Cap: MAX_UNDECIDED.
mut=        planted mistakes (MUTANTS_*): the checks must catch every one.
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

import attn_ref as A
import rowwise_ref as R
from decode_linear_ref import MAX_UNDECIDED  # noqa: F401  (the cap the tests assert)
from test_adamw_sr_host import sr_bits, sr_round

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CHUNK = 65536          # OPT_CHUNK: elements per workgroup
ERR64 = 4 * 2.0 ** -53
SQNORM_BOUND = (256 + 9) * 2.0 ** -24  # tests/test_grad_clip_gpu.py: relative, on a chunk's sum of squares
K_HOST = R.K_ELEM / 2


def f32s(x):
    """A double as the 0-dim fp32 tensor the kernel's (float) cast gives."""
    return torch.tensor(float(x), dtype=F64).to(F32)


def _fma32(a, b, c):
    """fp32 fma(a, b, c), exact: the product of two fp32 values is exact in fp64; the sum's fp64 rounding error comes
    from TwoSum and the fp64 sum is then rounded to odd (truncated towards zero, last bit set when inexact), which a
    following round-to-nearest to fp32 cannot tell from the exact value (53 >= 24 + 2 bits)."""
    p = a.double() * b.double()
    c = c.double().expand_as(p)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.contiguous().view(torch.int64)
    inexact = e != 0
    bits = torch.where(inexact & ((e > 0) != (s > 0)), bits - 1, bits)
    bits = torch.where(inexact, bits | 1, bits)
    return bits.view(F64).to(F32)


def sqrt32(x):
    """sqrtf, correctly rounded, as the device's is: the fp64 root rounded to fp32 (53 >= 2 * 24 + 2 bits, so the
    second rounding cannot differ from one). torch's own fp32 sqrt on the CPU is not correctly rounded everywhere
    (one step low in 17 % of 4 M values over 10^-12 .. 10^8, measured), so it cannot restate the kernel."""
    return x.double().sqrt().to(F32)


def bits_equal(a, b):
    """Bit for bit, as integers (NaN payloads and the sign of zero count)."""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    it = A._INT.get(a.dtype, torch.int64)
    return a.contiguous().view(it) == b.contiguous().view(it)


# ------------------------------------------------------------------------------------------ the tensor list
# off_p / off_g / off_s: 0 = aligned (256 bytes); 1 = moved by the smallest amount that turns the kernel's alignment
# predicate: one element (2 bytes) for a bf16 buffer, four elements (16 bytes: aligned to 16, not to 32) for an fp32
# one. p: the parameter (Muon: also work and O's partner); g: the gradient (Muon update: O); s: the states (AdamW m,
# v and the master p32; Muon's momentum buffer).
Row = namedtuple("Row", "n gf32 off_p off_g off_s note")
ROWS = (
    Row(8, False, 0, 0, 0, "one vector, 255 idle lanes"),
    Row(7, False, 0, 0, 0, "scalar, n < 8"),
    Row(1, False, 0, 0, 0, "single element"),
    Row(2056, False, 0, 0, 0, "lane 0 makes a second vector trip"),
    Row(3000, False, 1, 1, 1, "n % 8 == 0 but every pointer unaligned: scalar"),
    Row(2999, False, 0, 0, 0, "aligned, n % 8 != 0: scalar"),
    Row(CHUNK, False, 0, 0, 0, "one full chunk and nothing else"),
    Row(CHUNK + 8, False, 0, 0, 0, "a one-vector second chunk"),
    Row(CHUNK + 1, False, 0, 0, 0, "scalar across the seam, second chunk of one element"),
    Row(2 * CHUNK + 2056, False, 0, 0, 0, "three chunks"),
    Row(2056, False, 0, 1, 0, "only the gradient unaligned"),
    Row(2056, False, 0, 0, 1, "only a state unaligned (master: p32 / m / v at 16 but not 32 bytes)"),
    Row(CHUNK + 2056, True, 0, 0, 0, "fp32 gradient at 32 bytes: vector, with a seam"),
    Row(2056, True, 0, 1, 0, "fp32 gradient at 16 but not 32 bytes: scalar"),
    Row(2999, True, 0, 0, 0, "fp32 gradient, n % 8 != 0: scalar"),
)
KERNELS = ("adamw_bf16", "adamw_master", "grad", "muon_momentum", "muon_normalize", "muon_update")


def _byte_off(off, dtype):
    return off * (2 if dtype == BF else 16)


def shift_of(off, dtype):
    """Guards.mat's shift (elements) of an off_* flag."""
    return off * (1 if dtype == BF else 4)


def is_vec(kernel, row, ptrs=None):
    """The kernel's own choice between its vector and its scalar loop, from the predicates in the code (pointer % 16
    for bf16, % 32 for fp32 operands, n % 8). ptrs: {"p", "g", "s"} addresses of a real launch (default: the byte
    offsets the row asks for)."""
    gd = F32 if row.gf32 and kernel != "muon_update" else BF  # Muon's O is bf16 whatever the gradient is
    a = ptrs or {"p": _byte_off(row.off_p, BF), "g": _byte_off(row.off_g, gd),
                 "s": _byte_off(row.off_s, F32 if kernel == "adamw_master" else BF)}
    g_ok = a["g"] % (32 if row.gf32 else 16) == 0 and row.n % 8 == 0
    if kernel == "adamw_bf16":
        return a["p"] % 16 == 0 and a["s"] % 16 == 0 and g_ok
    if kernel == "adamw_master":
        return a["p"] % 16 == 0 and a["s"] % 32 == 0 and g_ok
    if kernel == "grad":
        return g_ok
    if kernel == "muon_momentum":  # m (s) and u (p's slot)
        return a["s"] % 16 == 0 and a["p"] % 16 == 0 and g_ok
    if kernel == "muon_normalize":
        return a["p"] % 16 == 0 and row.n % 8 == 0
    if kernel == "muon_update":  # p and O (g's slot, always bf16)
        return a["p"] % 16 == 0 and a["g"] % 16 == 0 and row.n % 8 == 0
    raise ValueError(kernel)


def chunks_of(sizes):
    """The chunk table: (tensor index, first element) in list order."""
    return [(ti, c0) for ti, n in enumerate(sizes) for c0 in range(0, n, CHUNK)]


def reach(kernel, rows=ROWS):
    """What the list reaches for one kernel: counts of vector / scalar tensors, full / partial chunks, and tensors on
    each path in which a lane makes more than one trip (vector: a chunk of more than 2048 elements; scalar: more than
    256)."""
    c = {"vec": 0, "scalar": 0, "full": 0, "partial": 0, "multi_vec": 0, "multi_scalar": 0, "seam_vec": 0,
         "seam_scalar": 0}
    for r_ in rows:
        v = is_vec(kernel, r_)
        c["vec" if v else "scalar"] += 1
        lens = [min(CHUNK, r_.n - c0) for c0 in range(0, r_.n, CHUNK)]
        c["full"] += sum(x == CHUNK for x in lens)
        c["partial"] += sum(x < CHUNK for x in lens)
        c["multi_vec" if v else "multi_scalar"] += any(x > (2048 if v else 256) for x in lens)
        c["seam_vec" if v else "seam_scalar"] += len(lens) > 1
    return c


# ------------------------------------------------------------------------------------------ input sets
KINDS = ("randn", "wide", "zeros")


def _wide(n, g, lo=-6.0, hi=4.0):
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return sign * torch.pow(10.0, torch.rand(n, generator=g) * (hi - lo) + lo)


def make_row(kind, row, seed=0):
    """One row's data on the CPU: p, m, v (bf16), g (bf16, or fp32 values that are not bf16 values), and fp32 p32,
    m32, v32 for the master form (p = bf16(p32)); o (bf16) is Muon's orthogonalised update. randn; wide: magnitudes
    10^-6 .. 10^4 across elements, mixed signs (v: 10^-12 .. 10^8); zeros: the gradient is zero in every second
    run of 5 elements and the second moment in every second run of 3 (so both, one and neither occur)."""
    g_ = torch.Generator().manual_seed(seed * 7919 + row.n * 31 + len(kind) + (5 if row.gf32 else 0))
    n = row.n
    if kind == "wide":
        p32, g32, m32, o32 = (_wide(n, g_) for _ in range(4))
        v32 = _wide(n, g_, -12.0, 8.0).abs()
    else:
        p32, g32, m32, o32 = (torch.randn(n, generator=g_) for _ in range(4))
        m32 = m32 * 0.3
        v32 = torch.randn(n, generator=g_).square() * 0.1
        if kind == "zeros":
            i = torch.arange(n)
            g32 = torch.where((i // 5) % 2 == 0, 0.0, g32)
            v32 = torch.where((i // 3) % 2 == 0, 0.0, v32)
        elif kind != "randn":
            raise ValueError(kind)
    g = g32 if row.gf32 else g32.to(BF)
    return {"p": p32.to(BF), "g": g, "m": m32.to(BF), "v": v32.to(BF), "p32": p32, "m32": m32, "v32": v32,
            "o": o32.to(BF)}


def make_list(kind, rows=ROWS, seed=0):
    return [make_row(kind, r_, seed + 13 * i) for i, r_ in enumerate(rows)]


def midpoint_distance(x):
    """Relative distance of x > 0 from the nearest midpoint between adjacent bf16 values (tests/test_muon_gpu.py)."""
    ulp = 2.0 ** (math.floor(math.log2(x)) - 7)
    return abs((x / ulp) % 1.0 - 0.5) * ulp / x


def make_muon_list(kind, momentum, nesterov, rows=ROWS, seed=0):
    """make_list whose every row meets the norm precondition of tests/test_muon_gpu.py: the fp64 norm of the
    restated u is at least 2^-12 relative from a bf16 midpoint (or zero); the next seed otherwise, 8 at the most."""
    out = []
    for i, r_ in enumerate(rows):
        for k in range(8):
            d = make_row(kind, r_, seed + 13 * i + 1000 * k)
            u = restate_muon_momentum(d["g"], d["m"], momentum, nesterov, vec=True)["u"]
            nrm = float(u.double().norm())
            if nrm == 0.0 or midpoint_distance(nrm) >= 2.0 ** -12:
                break
        else:
            raise AssertionError(f"no draw in 8 seeds met the precondition for row {i}")
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------ gradient value
def grad_value(g, coef=None, mut=None):
    """The fp32 value of a gradient element as the kernels take it (load_grad8 / load_grad1, then CLIP): an fp32
    main_grad is rounded to bf16 first; with a clip coefficient (0-dim fp32) g = float(bf16(g coef)), one fp32 product
    (no sum: nothing to contract)."""
    gf = g.float() if (g.dtype == BF or mut == "g_f32") else g.to(BF).float()
    if coef is not None:
        prod = gf * coef.to(F32)
        gf = prod if mut == "clip_f32" else prod.to(BF).float()
    return gf


# ------------------------------------------------------------------------------------------ AdamW
Hyper = namedtuple("Hyper", "lr wd step b1 b2 eps lr_wd bc2_sqrt step_size")


def hyper(lr, wd, step, b1=0.9, b2=0.999, eps=1e-8):
    """adamw_prepare's host prologue: bias corrections in double, step_size = (float)(lr / bc1)."""
    bc1 = 1.0 - math.pow(b1, float(step))
    bc2 = 1.0 - math.pow(b2, float(step))
    return Hyper(lr, wd, step, b1, b2, eps, lr * wd, math.sqrt(bc2), float(np.float32(lr / bc1)))


def _near_boundary(x, err):
    """x (fp64) within err of the midpoint of two adjacent fp32 values."""
    r_ = x.to(F32)
    inf = torch.tensor(math.inf, dtype=F32)
    up, dn = torch.nextafter(r_, inf), torch.nextafter(r_, -inf)
    dist = torch.minimum((x - (r_.double() + up.double()) / 2).abs(), (x - (r_.double() + dn.double()) / 2).abs())
    return (dist <= err) & (err > 0)


VARIANTS_ADAMW = tuple((a, b, c) for a in (0, 1) for b in (0, 1, 2) for c in (0, 1, 2))


class _Items:
    """t[i] as a Python float, converted on demand."""

    def __init__(self, t):
        self.t = t

    def __getitem__(self, i):
        return float(self.t[i])


def _contracted(x, err, exact):
    """x: a double expression evaluated operation by operation; exact(i): element i of the same expression with one
    product fused (Fractions: one rounding of the exact value). The two differ by less than err, so they can round to
    different fp32 values only where x is within err of a rounding boundary: only those elements are re-evaluated.
    Returns (x with them replaced, their mask)."""
    near = _near_boundary(x, err)
    idx = near.nonzero().flatten().tolist()
    if idx:
        x = x.clone()
        for i in idx:
            x[i] = exact(i)
    return x, near


def adam_elem(p, g, m, v, h, mut=None, variant=(0, 0, 0), track=False):
    """adam_elem on fp32 tensors: each of p - lr_wd p, m, v, denom in double and rounded once to fp32; sqrtf, the
    quotient step_size m / denom and the last difference in fp32. variant = (decay, m, v): 0 the double expression
    operation by operation; decay 1: fma(-lr_wd, p, p); m 1: fma(b1, m, (1 - b1) g), 2: fma(1 - b1, g, b1 m); v 1:
    fma(b2, v, ((1 - b2) g) g), 2: fma((1 - b2) g, g, b2 v). Returns (p, m, v, sensitive): sensitive marks the elements
    within ERR64 of an fp32 rounding boundary in some expression, the only ones a variant can change (looked for
    only under a variant other than (0, 0, 0) or with track; all False otherwise)."""
    Fr = Fraction
    vp, vm, vv = variant
    track = track or any(variant)
    fuse = _contracted if track else (lambda x, err, exact: (x, False))

    def decay(pf):
        pd = pf.double()
        x = pd - h.lr_wd * pd
        pl = _Items(pd)
        x, near = fuse(x, ERR64 * (pd.abs() + (h.lr_wd * pd).abs()),
                              (lambda i: float(Fr(pl[i]) - Fr(h.lr_wd) * Fr(pl[i]))) if vp else (lambda i: float(x[i])))
        return x.to(F32), near

    sens = torch.zeros(p.shape, dtype=torch.bool)
    if mut != "decay_after":
        p, s_ = decay(p)
        sens |= s_
    gd, md, vd = g.double(), m.double(), v.double()
    gl, ml, vl = _Items(gd), _Items(md), _Items(vd)
    c1, c2 = 1 - h.b1, 1 - h.b2
    t1, t2 = h.b1 * md, c1 * gd
    exact = {0: lambda i: ml[i] * h.b1 + c1 * gl[i], 1: lambda i: float(Fr(h.b1) * Fr(ml[i]) + Fr(c1 * gl[i])),
             2: lambda i: float(Fr(c1) * Fr(gl[i]) + Fr(h.b1 * ml[i]))}[vm]
    x, s_ = fuse(t1 + t2, ERR64 * (t1.abs() + t2.abs()), exact)
    sens |= s_
    m = x.to(F32)
    t1, t2 = h.b2 * vd, c2 * gd * gd
    exact = {0: lambda i: h.b2 * vl[i] + c2 * gl[i] * gl[i],
             1: lambda i: float(Fr(h.b2) * Fr(vl[i]) + Fr(c2 * gl[i] * gl[i])),
             2: lambda i: float(Fr(c2 * gl[i]) * Fr(gl[i]) + Fr(h.b2 * vl[i]))}[vv]
    x, s_ = fuse(t1 + t2, ERR64 * (t1.abs() + t2.abs()), exact)
    sens |= s_
    v = x.to(F32)
    if mut == "eps_in_sqrt":
        x = sqrt32(v + f32s(h.eps)).double() / h.bc2_sqrt
    else:
        x = sqrt32(v).double() / (1.0 if mut == "no_bc2" else h.bc2_sqrt) + h.eps  # a quotient: nothing to contract
    denom = x.to(F32)
    p = p - (f32s(h.step_size) * m) / denom
    if mut == "decay_after":
        p, s_ = decay(p)
        sens |= s_
    return p, m, v, sens


def _sr_store(x, seed, step, tid, quantity, idx0, mut=None):
    """fp32 -> bf16 by the stochastic rounding rule, elements idx0 .. idx0 + n - 1 of tensor id tid."""
    n = x.numel()
    bits = sr_bits(seed, step, tid, quantity, (idx0 + n + 7) // 8 * 8)
    if mut == "sr_lane":  # lane j of the wrong word: j ^ 2
        bits = bits.reshape(-1, 8)[:, np.arange(8) ^ 2].reshape(-1)
    out = sr_round(x.contiguous().numpy().view(np.uint32), bits[idx0:idx0 + n])
    return torch.from_numpy(out.view(np.int16).copy()).view(BF)


def restate_adamw(form, d, h, vec, coef=None, sr=None, mut=None, variant=(0, 0, 0), track=False):
    """One tensor's step. form: "bf16" (p, m, v bf16, rounded to nearest even), "sr" (rounded by sr = (seed, tensor
    id): counter (element >> 3, id, step, quantity), lane i & 7) or "master" (fp32 p32, m, v; p = bf16(p32)). d: a
    make_row dict; coef: 0-dim fp32 clip coefficient or None; vec: the tensor runs on the vector loop (the tail mutant
    needs it); track: also mark the variant-sensitive elements under variant (0, 0, 0). Returns {"p", "m", "v"
    (, "p32"), "undecided", "sensitive", "pre": the fp32 (p, m, v) before the store}."""
    def run(lo, hi, src):
        if form == "master":
            pf, mf, vf = src["p32"][lo:hi], src["m"][lo:hi], src["v"][lo:hi]
        else:
            pf, mf, vf = (src[k][lo:hi].float() for k in ("p", "m", "v"))
        p2, m2, v2, sens = adam_elem(pf, grad_value(d["g"][lo:hi], coef, mut), mf, vf, h, mut, variant, track)
        und = torch.zeros_like(sens)  # every variant is evaluated exactly: nothing is left undecided
        if form == "master":
            return {"p": p2.to(BF), "p32": p2, "m": m2, "v": v2, "undecided": und, "sensitive": sens,
                    "pre": (p2, m2, v2)}
        if form == "sr":
            st = [_sr_store(x, sr[0], h.step, sr[1], q, lo, mut) for q, x in enumerate((p2, m2, v2))]
        else:
            st = [x.to(BF) for x in (p2, m2, v2)]
        return {"p": st[0], "m": st[1], "v": st[2], "undecided": und, "sensitive": sens, "pre": (p2, m2, v2)}

    src = dict(d, m=d["m32"], v=d["v32"]) if form == "master" else d
    n = d["g"].numel()
    out = run(0, n, src)
    keys = [k for k in ("p", "p32", "m", "v") if k in out]
    if mut == "tail" and vec and n % CHUNK:  # the last vector of the tail chunk left unprocessed
        for k in keys:
            out[k] = out[k].clone()
            out[k][n - 8:] = src[k][n - 8:]
    if mut == "seam" and n > CHUNK:  # the first element after the seam processed twice
        again = run(CHUNK, CHUNK + 1, out)
        for k in keys:
            out[k] = out[k].clone()
            out[k][CHUNK] = again[k][0]
    return out


def ref_adamw(d, h, g_eff, master=False):
    """fp64 AdamW on one tensor; g_eff: the gradient value the step is specified to take (grad_value).
    cond: p (and p32): |p| + |lr wd p| + |step_size m' / denom|; m: |b1 m| + |(1 - b1) g|; v: b2 v + (1 - b2) g^2."""
    p, m, v = (d[k].double() for k in (("p32", "m32", "v32") if master else ("p", "m", "v")))
    g = g_eff.double()
    bc1, bc2 = 1.0 - math.pow(h.b1, float(h.step)), 1.0 - math.pow(h.b2, float(h.step))
    m1 = h.b1 * m + (1 - h.b1) * g
    v1 = h.b2 * v + (1 - h.b2) * g * g
    upd = (h.lr / bc1) * m1 / (v1.sqrt() / math.sqrt(bc2) + h.eps)
    p1 = p - h.lr * h.wd * p - upd
    cp = p.abs() + (h.lr * h.wd * p).abs() + upd.abs()
    out = {"p": (p1, cp), "m": (m1, (h.b1 * m).abs() + ((1 - h.b1) * g).abs()), "v": (v1, v1.abs())}
    if master:
        out["p32"] = (p1, cp)
    return out


def sr_widen(ref, k):
    """ref's bounds for a stochastically rounded bf16 output: either neighbour is a legal store, a whole bf16 step
    (2^-7 |ref| at the most) instead of half of one, carried into cond as extra / (k 2^-23) (decode_linear_ref's way)."""
    return {n: (r_, c_ + U_SR_EXTRA * r_.abs() / (k * R.ULP32)) for n, (r_, c_) in ref.items()}


U_SR_EXTRA = 2.0 ** -7 - R.U_BF16

MUTANTS_ADAMW = ("decay_after", "no_bc2", "eps_in_sqrt", "g_f32", "clip_f32", "tail", "seam", "sr_lane")


# ------------------------------------------------------------------------------------------ sum of squares
def _pairwise(x):
    """Adjacent pairs along the last dimension, once."""
    return x[..., 0::2] + x[..., 1::2]


def block_sum(s):
    """block_sum_store: s fp32 [..., 256] (the lanes' sums) -> [...]: the balanced pairwise tree over each wave's 64
    lanes in lane order (every level of wave_sum_dpp adds neighbours of 1, 2, 4, 8, 16, 32), then (w0 + w1) + (w2 + w3)."""
    for _ in range(8):
        s = _pairwise(s)
    return s[..., 0]


def chunk_partial(sq, vec):
    """One chunk's partial from its elements' squares (fp32 [len], len <= 65536), in the documented order. vector:
    lane t, slot j takes element 8 t + 2048 trip + j into acc[j] in trip order, then ((0+1)+(2+3))+((4+5)+(6+7));
    scalar: lane t takes t, t + 256, ... into one accumulator. Missing elements add +0, which changes no bit of a sum
    of non-negative terms."""
    per = 2048 if vec else 256
    trips = max(1, -(-sq.numel() // per))
    x = torch.zeros(trips * per, dtype=F32)
    x[:sq.numel()] = sq
    x = x.view(trips, 256, 8) if vec else x.view(trips, 256)
    acc = torch.zeros_like(x[0])
    for t in range(trips):
        acc = acc + x[t]
    if vec:
        acc = _pairwise(_pairwise(_pairwise(acc)))[..., 0]
    return block_sum(acc)


def list_partials(values, vecs, mut=None):
    """Chunk partials (fp32 [n_chunks]) of a list of fp32 value tensors (squares are formed here; the square of a bf16
    value is exact in fp32, so contraction changes nothing). mut: "tail" (the last vector of a vector tensor's tail
    chunk unsummed) or "seam" (the first element after a seam summed twice)."""
    out = []
    for x, vec in zip(values, vecs):
        n = x.numel()
        sq = x.float() * x.float()
        for c0 in range(0, n, CHUNK):
            s = sq[c0:min(n, c0 + CHUNK)]
            if mut == "tail" and vec and c0 + CHUNK > n:
                s = s[:-8]
            if mut == "seam" and c0 == CHUNK:
                s = torch.cat([s[:1], s])
            out.append(chunk_partial(s, vec))
    return torch.stack(out) if out else torch.zeros(0, dtype=F32)


def final_sum(partials):
    """grad_sqnorm_final_kernel: lane t adds partials t, t + 256, ... in double, then the LDS tree sh[t] += sh[t + w],
    w = 128 .. 1."""
    trips = max(1, -(-partials.numel() // 256))
    x = torch.zeros(trips * 256, dtype=F64)
    x[:partials.numel()] = partials.double()
    x = x.view(trips, 256)
    a = torch.zeros(256, dtype=F64)
    for t in range(trips):
        a = a + x[t]
    w = 128
    while w:
        a = a[:w] + a[w:2 * w]
        w //= 2
    return a[0]


def clip_coef(sumsq, max_norm):
    """grad_clip_coef_kernel: (norm, coef) = ((float)sqrt(sumsq), fminf(1, max_norm / (norm + 1e-6f))), fp32 [2]."""
    norm = sumsq.double().sqrt().to(F32)
    coef = torch.minimum(torch.ones((), dtype=F32), f32s(max_norm) / (norm + f32s(1e-6)))
    return torch.stack([norm, coef])


def restate_grad_sqnorm(grads, vecs, max_norm=1.0, mut=None, omit=None):
    """pico_grad_sqnorm then pico_grad_clip_coef over a gradient list. omit: a tensor index whose partials are left
    out of the final sum (the "omit" mutant). Returns {"partials", "sumsq", "norm_coef"}."""
    parts = list_partials([grad_value(g) for g in grads], vecs, mut)
    used = parts
    if omit is not None:
        ch = chunks_of([g.numel() for g in grads])
        used = parts[torch.tensor([ti != omit for ti, _ in ch])]
    sumsq = final_sum(used)
    return {"partials": parts, "sumsq": sumsq, "norm_coef": clip_coef(sumsq, max_norm)}


def ref_sumsq(values):
    """fp64 sum of squares per chunk of a list of value tensors (the bound on a partial: SQNORM_BOUND relative)."""
    return torch.stack([x[c0:c0 + CHUNK].double().square().sum() for x in values for c0 in range(0, x.numel(), CHUNK)])


def restate_grad_scale(g, coef, mut=None):
    """pico_grad_scale on one tensor: bf16(float(g) coef); an fp32 main_grad holds float(bf16(float(bf16(g)) coef))."""
    v = grad_value(g, coef, mut)
    return v if g.dtype == F32 else v.to(BF)


def ref_grad_scale(g, coef):
    """g coef in fp64 with g the bf16 gradient value. cond |g coef|."""
    v = grad_value(g).double() * float(coef)
    return {"g": (v, v.abs())}


# ------------------------------------------------------------------------------------------ Muon
VARIANTS_MOMENTUM = tuple((a, b) for a in (False, True) for b in (False, True))  # (a + w d, b - d (1 - w)) contracted
VARIANTS_UPDATE = ((False,), (True,))                                              # pf + alpha o contracted


def lerp32(a, b, w, variant=(False, False), mut=None):
    """ATen's lerp in fp32: d = b - a; |w| < 0.5 ? a + w d : b - d (1 - w); w a 0-dim fp32."""
    d = b - a
    first = bool(w.abs() <= 0.5) if mut == "lerp_le" else bool(w.abs() < 0.5)
    if mut == "lerp_first":
        first = True
    if first:
        return _fma32(w, d, a) if variant[0] else a + w * d
    om = torch.ones((), dtype=F32) - w
    return _fma32(-d, om, b) if variant[1] else b - d * om


def restate_muon_momentum(g, m, momentum, nesterov, vec, variant=(False, False), mut=None):
    """One tensor of pico_muon_momentum: m' = bf16(lerp(m, g, (float)(1 - momentum))); u = nesterov ?
    bf16(lerp(g, m', (float)momentum)) : m'. Returns {"m", "u"} (the partials: list_partials of u)."""
    gf = grad_value(g)
    wg, mo = f32s(1.0 - momentum), f32s(momentum)

    def elem(gf, mf):
        m1 = lerp32(mf, gf, wg, variant, mut).to(BF)
        if not nesterov:
            return m1, m1
        return m1, lerp32(gf, m1.float(), wg if mut == "swap_w" else mo, variant, mut).to(BF)

    m1, u = elem(gf, m.float())
    n = g.numel()
    if mut == "tail" and vec and n % CHUNK:
        m1, u = m1.clone(), u.clone()
        m1[n - 8:] = m[n - 8:]
        u[n - 8:] = 0.0
    if mut == "seam" and n > CHUNK:
        m2, u2 = elem(gf[CHUNK:CHUNK + 1], m1[CHUNK:CHUNK + 1].float())
        m1, u = m1.clone(), u.clone()
        m1[CHUNK], u[CHUNK] = m2[0], u2[0]
    return {"m": m1, "u": u}


def ref_muon_momentum(g, m, momentum, nesterov, m1):
    """fp64 lerps with the weights cast to fp32 as the operation specifies. m1: the bf16 m' the second lerp starts
    from (the checked output). cond: |a| + |b| + |w (b - a)| for lerp(a, b, w), the magnitudes of either form's terms."""
    gd, md = grad_value(g).double(), m.double()
    wg, mo = float(f32s(1.0 - momentum)), float(f32s(momentum))
    r1 = md + wg * (gd - md)
    out = {"m": (r1, md.abs() + gd.abs() + (wg * (gd - md)).abs())}
    if nesterov:
        m1d = m1.double()
        out["u"] = (gd + mo * (m1d - gd), gd.abs() + m1d.abs() + (mo * (m1d - gd)).abs())
    else:
        out["u"] = (m1.double(), m1.double().abs())
    return out


def restate_muon_norm(partials, eps):
    """muon_norm_kernel for one tensor: its chunk partials added in index order in double, then
    max(float(bf16((float)sqrt)), (float)eps). Returns a 0-dim fp32."""
    a = torch.zeros((), dtype=F64)
    for x in partials.double():
        a = a + x
    return torch.maximum(a.sqrt().to(F32).to(BF).float(), f32s(eps))


def restate_muon_normalize(u, nrm):
    """work = bf16(work / norm): a true fp32 division."""
    return (u.float() / nrm).to(BF)


def ref_muon_normalize(u, nrm):
    """u / norm in fp64 with the norm the kernel's own. cond |u / norm|."""
    v = u.double() / float(nrm)
    return {"work": (v, v.abs())}


def restate_muon_update(p, o, lr, wd, ratio, variant=(False,), mut=None, vec=True):
    """p = bf16(p (float)(1 - lr wd)) (mul_: its own rounding), then p = bf16(p + (float)(-(lr ratio)) O)."""
    decay, alpha = f32s(1.0 - lr * wd), f32s(-(lr * ratio))

    def elem(pf, of):
        prod = pf * decay
        pf = prod if mut == "no_mul_round" else prod.to(BF).float()
        return (_fma32(alpha, of, pf) if variant[0] else pf + alpha * of).to(BF), pf

    out, mid = elem(p.float(), o.float())
    n = p.numel()
    if mut == "tail" and vec and n % CHUNK:
        out = out.clone()
        out[n - 8:] = p[n - 8:]
    if mut == "seam" and n > CHUNK:
        out = out.clone()
        out[CHUNK] = elem(out[CHUNK:CHUNK + 1].float(), o[CHUNK:CHUNK + 1].float())[0][0]
    return {"p": out, "mul": mid}


def ref_muon_update(mul, o, lr, ratio):
    """mul + alpha O in fp64, mul the specified bf16 result of mul_ (the restatement's "mul"), alpha cast to fp32.
    cond |mul| + |alpha O|."""
    alpha = float(f32s(-(lr * ratio)))
    a, b = mul.double(), alpha * o.double()
    return {"p": (a + b, a.abs() + b.abs())}


MUTANTS_MUON = ("lerp_le", "lerp_first", "swap_w", "tail", "seam")
MUTANTS_UPDATE = ("no_mul_round", "tail", "seam")
MUTANTS_NORM = ("tail", "seam", "omit")


# ------------------------------------------------------------------------------------------ bucket kernels
def restate_grad_accum(main, g, divide_by):
    """main += g, then (divide_by != 1) * (1.f / divide_by): two correctly rounded fp32 operations."""
    v = main + g.float()
    return v * (torch.ones((), dtype=F32) / f32s(divide_by)) if divide_by != 1.0 else v


def ref_grad_accum(main, g, divide_by):
    """(main + g) * fp32(1 / W) in fp64. cond (|main| + |g|) / W."""
    inv = float(torch.ones((), dtype=F32) / f32s(divide_by))
    return {"main": ((main.double() + g.double()) * inv, (main.double().abs() + g.double().abs()) * inv)}


def restate_scale_f32(x, divide_by):
    return x * (torch.ones((), dtype=F32) / f32s(divide_by)) if divide_by != 1.0 else x.clone()


def restate_cast(x):
    return x.to(BF)


def restate_sr_round(x, seed, step, tid, quantity, mut=None):
    return _sr_store(x, seed, step, tid, quantity, 0, mut)


# ------------------------------------------------------------------------------------------ the criteria of today
def criterion_e(x, y):
    """Criterion E of tests/test_optim_gpu.py / test_muon_gpu.py on two bf16 tensors: no element off by more than one
    bf16 step (except both below 1e-12) and fewer than 1e-3 of the elements differ."""
    d = (x.view(torch.int16).to(torch.int32) - y.view(torch.int16).to(torch.int32)).abs()
    bad = (d > 1) & ~((x.float().abs() < 1e-12) & (y.float().abs() < 1e-12))
    return not bool(bad.any()) and float((d > 0).float().mean()) < 1e-3


def criterion_2x(ours, other32, ref64):
    """tests/test_adamw_master_gpu.py: max|ours - f64| <= 2 max|other fp32 evaluation - f64| over a tensor."""
    return float((ours.double() - ref64).abs().max()) <= 2 * float((other32.double() - ref64).abs().max())


def criterion_norm(norm, ref64):
    """tests/test_grad_clip_gpu.py: the list norm within 2^-16 relative of fp64."""
    return abs(float(norm) - ref64) <= 2.0 ** -16 * ref64


def matching_variants(got, restate, variants):
    """The variants under which every tensor of got (a list of dicts) is bit-equal to restate(i, variant) (same keys),
    outside an optional "undecided" mask; and whether every element at least lies in the candidate set."""
    ok, member = [], None
    for var in variants:
        all_eq = True
        eqs = []
        for i, gt in enumerate(got):
            want = restate(i, var)
            und = want.get("undecided")
            e = {k: bits_equal(gt[k], want[k]) | (und if und is not None else False) for k in gt}
            eqs.append(e)
            all_eq &= all(bool(v.all()) for v in e.values())
        if all_eq:
            ok.append(var)
        member = eqs if member is None else [{k: a[k] | b[k] for k in a} for a, b in zip(member, eqs)]
    return ok, all(bool(v.all()) for e in member for v in e.values())


# ------------------------------------------------------------------------------------------ launches (HIP device)
def _i64(G, name, data):
    return G.mat(name, 1, len(data), dtype=torch.int64, data=torch.tensor(data, dtype=torch.int64))


def _tables(G, cols, sizes):
    """The three device tables, built by hand from include/picotron_hip.h: tensors [n][5] int64, sizes [n], chunks
    [n_chunks][2]. Returns (tensors, sizes, chunks, n_chunks)."""
    ch = chunks_of(sizes)
    return (_i64(G, "tensors", [x for row in cols for x in row]), _i64(G, "sizes", sizes),
            _i64(G, "chunks", [x for c in ch for x in c]), len(ch))


def _unread(G, name):
    """A guard-only NaN buffer for a column the header says a kernel does not read: a write there changes a guard, a
    read brings a NaN into an output."""
    return G.mat(name, 1, 8, data=torch.full((8,), math.nan, dtype=BF, device="cuda")).data_ptr()


def _put(G, name, data, off, inout=False, dev="cuda"):
    return G.mat(name, 1, data.numel(), dtype=data.dtype, data=data.to(dev), shift=shift_of(off, data.dtype),
                 inout=inout)


def _cpu(ts):
    return [t[0].cpu() for t in ts]


def launch_adamw(form, rows, data, h, norm_coef=None, seed=0, ids=None, clip_entry=False):
    """pico_adamw_bf16 / _bf16_clip (clip_entry) / _master / _bf16_sr over a list on guarded buffers. norm_coef: fp32
    [2] or None. Returns {"p", "m", "v" (, "p32")}: lists of CPU tensors, and "ptrs": per row {"p", "g", "s"}."""
    L, lib = R._lib()
    G = A.Guards("cuda")
    master = form == "master"
    P, Gr, M, V, P32, cols, ptrs = [], [], [], [], [], [], []
    for i, (r_, d) in enumerate(zip(rows, data)):
        P.append(_put(G, f"p{i}", d["p"], r_.off_p, inout=True))
        Gr.append(_put(G, f"g{i}", d["g"], r_.off_g))
        M.append(_put(G, f"m{i}", d["m32" if master else "m"], r_.off_s, inout=True))
        V.append(_put(G, f"v{i}", d["v32" if master else "v"], r_.off_s, inout=True))
        if master:
            P32.append(_put(G, f"p32_{i}", d["p32"], r_.off_s, inout=True))
        cols.append([P[i].data_ptr(), Gr[i].data_ptr(), M[i].data_ptr(), V[i].data_ptr(), int(r_.gf32)])
        ptrs.append({"p": P[i].data_ptr(), "g": Gr[i].data_ptr(),
                     "s": M[i].data_ptr() | V[i].data_ptr() | (P32[i].data_ptr() if master else 0)})
    T, S, C, nch = _tables(G, cols, [r_.n for r_ in rows])
    nc = G.mat("norm_coef", 1, 2, dtype=F32, data=norm_coef.cuda()) if norm_coef is not None else None
    hy = (h.lr, h.b1, h.b2, h.eps, h.wd, h.step)
    st = L.stream_of(P[0])
    if master:
        X = _i64(G, "masters", [t.data_ptr() for t in P32])
        fn = lambda: lib.pico_adamw_master(L.ptr(T), L.ptr(X), L.ptr(S), L.ptr(C), nch, *hy, L.ptr(nc), st)  # noqa: E731
    elif form == "sr":
        X = _i64(G, "ids", ids)
        fn = lambda: lib.pico_adamw_bf16_sr(L.ptr(T), L.ptr(X), L.ptr(S), L.ptr(C), nch, *hy, L.ptr(nc), seed, st)  # noqa: E731
    elif clip_entry:
        fn = lambda: lib.pico_adamw_bf16_clip(L.ptr(T), L.ptr(S), L.ptr(C), nch, *hy, L.ptr(nc), st)  # noqa: E731
    else:
        assert nc is None
        fn = lambda: lib.pico_adamw_bf16(L.ptr(T), L.ptr(S), L.ptr(C), nch, *hy, st)  # noqa: E731
    R._run(G, fn, "pico_adamw_" + form)
    out = {"p": _cpu(P), "m": _cpu(M), "v": _cpu(V), "ptrs": ptrs}
    if master:
        out["p32"] = _cpu(P32)
    return out


def launch_grad_norm(rows, grads, max_norm=1.0, scale_with=None):
    """pico_grad_sqnorm + pico_grad_clip_coef (and, scale_with = fp32 [2] or "own", pico_grad_scale) on guarded
    buffers. Every column but the gradient's and grad_is_f32 points at a guard-only NaN buffer. Returns {"partials",
    "sumsq", "norm_coef", "g" (the gradients after the launch), "ptrs"}."""
    L, lib = R._lib()
    G = A.Guards("cuda")
    scaled = scale_with is not None
    Gr = [_put(G, f"g{i}", g, r_.off_g, inout=scaled) for i, (r_, g) in enumerate(zip(rows, grads))]
    dead = [_unread(G, f"unread{k}") for k in range(3)]
    T, S, C, nch = _tables(G, [[dead[0], g.data_ptr(), dead[1], dead[2], int(r_.gf32)] for r_, g in zip(rows, Gr)],
                           [r_.n for r_ in rows])
    assert lib.pico_grad_sqnorm_workspace_bytes(nch) == 4 * nch
    ws = G.mat("workspace", 1, nch, dtype=F32)
    sumsq = G.mat("sumsq", 1, 1, dtype=torch.int64)  # the device double, held as its bits
    nc = G.mat("norm_coef", 1, 2, dtype=F32)
    st = L.stream_of(Gr[0])

    def go():
        rc = lib.pico_grad_sqnorm(L.ptr(T), L.ptr(S), L.ptr(C), nch, L.ptr(ws), L.ptr(sumsq), st)
        return rc or lib.pico_grad_clip_coef(L.ptr(sumsq), max_norm, L.ptr(nc), st)
    R._run(G, go, "pico_grad_sqnorm")
    out = {"partials": ws[0].cpu(), "sumsq": sumsq[0].cpu().view(F64)[0], "norm_coef": nc[0].cpu(),
           "ptrs": [{"g": g.data_ptr()} for g in Gr]}
    if scaled:
        if not isinstance(scale_with, str):
            nc.copy_(scale_with.cuda().view(1, 2))
        R._run(G, lambda: lib.pico_grad_scale(L.ptr(T), L.ptr(S), L.ptr(C), nch, L.ptr(nc), st), "pico_grad_scale")
    out["g"] = _cpu(Gr)
    return out


def launch_muon_momentum(rows, data, momentum, nesterov):
    """pico_muon_momentum: the param column points at a guard-only NaN buffer. Returns {"m", "u", "partials", "ptrs"}."""
    L, lib = R._lib()
    G = A.Guards("cuda")
    Gr = [_put(G, f"g{i}", d["g"], r_.off_g) for i, (r_, d) in enumerate(zip(rows, data))]
    M = [_put(G, f"m{i}", d["m"], r_.off_s, inout=True) for i, (r_, d) in enumerate(zip(rows, data))]
    U = [G.mat(f"u{i}", 1, r_.n, shift=shift_of(r_.off_p, BF)) for i, r_ in enumerate(rows)]
    dead = _unread(G, "unread_param")
    T, S, C, nch = _tables(G, [[dead, g.data_ptr(), m.data_ptr(), u.data_ptr(), int(r_.gf32)]
                               for r_, g, m, u in zip(rows, Gr, M, U)], [r_.n for r_ in rows])
    part = G.mat("partials", 1, nch, dtype=F32)
    R._run(G, lambda: lib.pico_muon_momentum(L.ptr(T), L.ptr(S), L.ptr(C), nch, momentum, int(nesterov), L.ptr(part),
                                             L.stream_of(part)), "pico_muon_momentum")
    return {"m": _cpu(M), "u": _cpu(U), "partials": part[0].cpu(),
            "ptrs": [{"p": u.data_ptr(), "g": g.data_ptr(), "s": m.data_ptr()} for u, g, m in zip(U, Gr, M)]}


def launch_muon_normalize(rows, work, partials, eps, chunk_start=None):
    """pico_muon_normalize: only the work column is real. chunk_start: default from the list. Returns {"work", "norms"}."""
    L, lib = R._lib()
    G = A.Guards("cuda")
    W = [_put(G, f"work{i}", w, r_.off_p, inout=True) for i, (r_, w) in enumerate(zip(rows, work))]
    dead = [_unread(G, f"unread{k}") for k in range(3)]
    sizes = [r_.n for r_ in rows]
    T, S, C, nch = _tables(G, [[dead[0], dead[1], dead[2], w.data_ptr(), 0] for w in W], sizes)
    if chunk_start is None:
        chunk_start = [0]
        for n in sizes:
            chunk_start.append(chunk_start[-1] + -(-n // CHUNK))
    CS = _i64(G, "chunk_start", chunk_start)
    part = _put(G, "partials", partials, 0)
    norms = G.mat("norms", 1, len(rows), dtype=F32)
    R._run(G, lambda: lib.pico_muon_normalize(L.ptr(T), L.ptr(S), L.ptr(C), nch, L.ptr(CS), len(rows), L.ptr(part),
                                              eps, L.ptr(norms), L.stream_of(part)), "pico_muon_normalize")
    return {"work": _cpu(W), "norms": norms[0].cpu()}


def launch_muon_update(rows, data, lr, wd, ratios):
    """pico_muon_update: every column but the parameter's points at a guard-only NaN buffer; O comes from out_ptrs."""
    L, lib = R._lib()
    G = A.Guards("cuda")
    P = [_put(G, f"p{i}", d["p"], r_.off_p, inout=True) for i, (r_, d) in enumerate(zip(rows, data))]
    O = [_put(G, f"o{i}", d["o"], r_.off_g) for i, (r_, d) in enumerate(zip(rows, data))]
    dead = [_unread(G, f"unread{k}") for k in range(3)]
    T, S, C, nch = _tables(G, [[p.data_ptr(), dead[0], dead[1], dead[2], 0] for p in P], [r_.n for r_ in rows])
    OP = _i64(G, "out_ptrs", [o.data_ptr() for o in O])
    RT = _i64(G, "ratios", torch.tensor(ratios, dtype=F64).view(torch.int64).tolist())  # doubles, as their bits
    R._run(G, lambda: lib.pico_muon_update(L.ptr(T), L.ptr(OP), L.ptr(S), L.ptr(C), nch, lr, wd, L.ptr(RT),
                                           L.stream_of(RT)), "pico_muon_update")
    return {"p": _cpu(P), "ptrs": [{"p": p.data_ptr(), "g": o.data_ptr()} for p, o in zip(P, O)]}


def launch_bucket(op, x, g=None, divide_by=1.0, shift=0, sr=None, keep_device=False):
    """pico_grad_accum (x fp32 += g bf16), pico_scale_f32 (x fp32), pico_cast_f32_bf16 or pico_sr_round_bf16
    (sr = (seed, step, id, quantity)) (x fp32 -> bf16) on guarded buffers; shift moves every buffer by that many
    elements. Returns the output (on the device with keep_device)."""
    L, lib = R._lib()
    G = A.Guards("cuda")
    n = x.numel()
    st = None
    if op in ("accum", "scale"):
        xg = G.mat("x", 1, n, dtype=F32, data=x.cuda(), shift=shift, inout=True)
        if op == "accum":
            gg = G.mat("g", 1, n, data=g.cuda(), shift=shift)
            fn = lambda: lib.pico_grad_accum(L.ptr(xg), L.ptr(gg), n, divide_by, st)  # noqa: E731
        else:
            fn = lambda: lib.pico_scale_f32(L.ptr(xg), n, divide_by, st)  # noqa: E731
        out = xg
    else:
        xg = G.mat("x", 1, n, dtype=F32, data=x.cuda(), shift=shift)
        out = G.mat("y", 1, n, shift=shift)
        if op == "cast":
            fn = lambda: lib.pico_cast_f32_bf16(L.ptr(xg), L.ptr(out), n, st)  # noqa: E731
        else:
            fn = lambda: lib.pico_sr_round_bf16(L.ptr(xg), L.ptr(out), n, sr[0], sr[1], sr[2], sr[3], st)  # noqa: E731
    st = L.stream_of(xg)
    R._run(G, fn, "pico_" + op)
    return out[0] if keep_device else out[0].cpu()
