"""Reference, emulation, per-tile error check, input sets and guard bands for the attention kernel tests
(tests/test_attn_tiles_host.py, tests/test_attn_tiles_gpu.py). A plain helper module: no fixture, no conftest; plain
torch on any device except the launch helpers at the bottom, which need the library and a HIP device.

Layout everywhere: q / o / do / dq [B, Sq, Hq, D], k / v / dk / dv [B, Sk, Hkv, D], lse [B, Hq, Sq] (natural log).

reference_*   fp64, the operation itself (GQA, top-left causal mask, Sq != Sk when non-causal).
emulate_*     the same operation at the kernels' precision: fp32 math, P and dS rounded to bf16 before their matmuls,
              bf16 outputs (fp32 dQ in the accumulate mode). Dense, or blockwise over 64-key tiles (online softmax in
              the forward). Written from the formulas, not from the kernels.
tile_check    per (batch, head, 32 consecutive rows) tile T of an output X:
                  ||X_kernel[T] - X_ref[T]|| <= M * ||X_emul_dense[T] - X_ref[T]|| + 2^-9 * ||X_ref[T]||
              M = 2: the margin the project gives decode logits over the training forward's own error (another
              accumulation order, another rescale history). 2^-9: one bf16 round-to-nearest of the output, which also
              covers tiles where the emulation happens to be exact; dropped for an fp32 output.
"""
import math

import torch

BF = torch.bfloat16
TILE = 32          # rows per tile of the check
M_TILE = 2.0       # the margin m
BF16_RN = 2.0 ** -9
LSE_TOL = 2e-3     # max-abs per row against fp64: the project's existing bound
FWD_TOL, BWD_TOL = 4e-3, 1e-2  # the suite's whole-tensor rel_l2 tolerances
BETA = 16.0        # diag / bait inputs: scaled score of the planted key (see make_inputs)
_CHUNK = 1 << 25   # scores per chunk of (kv head, group, Sq, Sk): 256 MB in fp64, under 1 GB with the temporaries


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------ the operation
def _chunks(Hkv, G, Sq, Sk):
    step = max(1, _CHUNK // max(1, G * Sq * Sk))
    return [(h0, min(Hkv, h0 + step)) for h0 in range(0, Hkv, step)]


def _mask(Sq, Sk, causal, dev, allow=None, b=0, hq0=0, hq1=0, G=1):
    """bool [Hc, G, Sq, Sk] or [Sq, Sk] (True = visible). allow: optional override {(b, hq): bool [Sq, Sk]}."""
    base = torch.ones(Sq, Sk, dtype=torch.bool, device=dev)
    if causal:
        base = torch.tril(base)
    if not allow or not any(key[0] == b and hq0 <= key[1] < hq1 for key in allow):
        return base
    m = base.expand((hq1 - hq0) // G, G, Sq, Sk).clone()
    for (bb, hq), mm in allow.items():
        if bb == b and hq0 <= hq < hq1:
            m[(hq - hq0) // G, (hq - hq0) % G] = mm.to(dev)
    return m


def _heads(t, b, h0, h1, dt):
    return t[b, :, h0:h1].permute(1, 0, 2).to(dt)  # [h, S, D]


def _kv_heads(t, b, h0, h1, G, dt):
    """[Hc, G, Sk, D]: the kv head of every query head."""
    return _heads(t, b, h0, h1, dt).unsqueeze(1).expand(h1 - h0, G, t.shape[1], t.shape[3])


def _fwd(q, k, v, scale, causal, dt, round_p, block, allow=None):
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    dev = q.device
    o = torch.empty(B, Sq, Hq, D, dtype=dt, device=dev)
    lse = torch.empty(B, Hq, Sq, dtype=dt, device=dev)
    for b in range(B):
        for h0, h1 in _chunks(Hkv, G, Sq, Sk):
            qc = _heads(q, b, h0 * G, h1 * G, dt).reshape(h1 - h0, G, Sq, D)
            kc, vc = _kv_heads(k, b, h0, h1, G, dt), _kv_heads(v, b, h0, h1, G, dt)
            msk = _mask(Sq, Sk, causal, dev, allow, b, h0 * G, h1 * G, G)
            if block is None:
                s = (qc @ kc.transpose(-1, -2) * scale).masked_fill(~msk, -math.inf)
                mx = s.amax(-1, keepdim=True)
                p = torch.exp(s - mx)
                l = p.sum(-1, keepdim=True)
                if round_p:
                    p = p.to(BF).to(dt)
                oc = (p @ vc) / l
            else:  # online softmax over `block`-key tiles
                mx = torch.full((h1 - h0, G, Sq, 1), -math.inf, dtype=dt, device=dev)
                l = torch.zeros_like(mx)
                acc = torch.zeros(h1 - h0, G, Sq, D, dtype=dt, device=dev)
                for j0 in range(0, Sk, block):
                    j1 = min(Sk, j0 + block)
                    s = (qc @ kc[:, :, j0:j1].transpose(-1, -2) * scale).masked_fill(~msk[..., j0:j1], -math.inf)
                    mn = torch.maximum(mx, s.amax(-1, keepdim=True))
                    live = mn > -math.inf
                    alpha = torch.where(live, torch.exp(mx - mn), torch.ones_like(mn))
                    p = torch.where(live, torch.exp(s - mn), torch.zeros_like(s))
                    l = l * alpha + p.sum(-1, keepdim=True)
                    if round_p:
                        p = p.to(BF).to(dt)
                    acc = acc * alpha + p @ vc[:, :, j0:j1]
                    mx = mn
                oc = acc / l
            o[b, :, h0 * G:h1 * G] = oc.reshape(-1, Sq, D).permute(1, 0, 2)
            lse[b, h0 * G:h1 * G] = (mx + torch.log(l)).reshape(-1, Sq)
    return o, lse


def reference_fwd(q, k, v, scale, causal, **mut):
    """fp64 O and LSE."""
    return _fwd(q, k, v, scale, causal, torch.float64, False, None, **mut)


def emulate_fwd(q, k, v, scale, causal, block=None, **mut):
    """bf16 O and fp32 LSE at the kernels' precision; block = 64: blockwise online softmax, None: dense."""
    o, lse = _fwd(q, k, v, scale, causal, torch.float32, True, block, **mut)
    return o.to(BF), lse


def rope_inv(x, cos, sin):
    """RoPE^-1 (rotation by -theta, half-split layout) of x [B, S, H, D] in x's dtype; cos / sin [>= S, D/2]."""
    S, h = x.shape[1], x.shape[3] // 2
    c, s = cos[:S, :h].to(x.dtype)[None, :, None, :], sin[:S, :h].to(x.dtype)[None, :, None, :]
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat((x1 * c + x2 * s, x2 * c - x1 * s), -1)


def _bwd(do, q, k, v, o, lse, scale, causal, dt, rnd, block, rope, allow=None, drop=None):
    """P = exp(scale QK^T - LSE), delta = rowsum(dO O), dS = P (dO V^T - delta), dQ = scale dS K,
    dK = scale dS^T Q, dV = P^T dO. drop: optional {(b, hq): bool [Sq, Sk]} of (query, key) pairs whose contribution
    is missing from dK / dV only (the key-major kernels' work lists; dQ has its own kernel)."""
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    dev = q.device
    dq = torch.zeros(B, Sq, Hq, D, dtype=dt, device=dev)
    dk = torch.zeros(B, Sk, Hkv, D, dtype=dt, device=dev)
    dv = torch.zeros(B, Sk, Hkv, D, dtype=dt, device=dev)
    r = (lambda x: x.to(BF).to(dt)) if rnd else (lambda x: x)
    for b in range(B):
        for h0, h1 in _chunks(Hkv, G, Sq, Sk):
            Hc = h1 - h0
            qc = _heads(q, b, h0 * G, h1 * G, dt).reshape(Hc, G, Sq, D)
            doc = _heads(do, b, h0 * G, h1 * G, dt).reshape(Hc, G, Sq, D)
            oc = _heads(o, b, h0 * G, h1 * G, dt).reshape(Hc, G, Sq, D)
            kc, vc = _kv_heads(k, b, h0, h1, G, dt), _kv_heads(v, b, h0, h1, G, dt)
            ls = lse[b, h0 * G:h1 * G].to(dt).reshape(Hc, G, Sq, 1)
            delta = (doc * oc).sum(-1, keepdim=True)
            msk = _mask(Sq, Sk, causal, dev, allow, b, h0 * G, h1 * G, G)
            keep = None
            if drop and any(key[0] == b and h0 * G <= key[1] < h1 * G for key in drop):
                keep = torch.ones(Hc, G, Sq, Sk, dtype=dt, device=dev)
                for (bb, hq), mm in drop.items():
                    if bb == b and h0 * G <= hq < h1 * G:
                        keep[hq // G - h0, hq % G] = (~mm).to(dt).to(dev)
            dqc = torch.zeros(Hc, G, Sq, D, dtype=dt, device=dev)
            for j0 in range(0, Sk, block or Sk):
                j1 = min(Sk, j0 + (block or Sk))
                kt, vt = kc[:, :, j0:j1], vc[:, :, j0:j1]
                p = torch.exp((qc @ kt.transpose(-1, -2) * scale).masked_fill(~msk[..., j0:j1], -math.inf) - ls)
                ds = r(p * (doc @ vt.transpose(-1, -2) - delta))
                p = r(p)
                dqc += ds @ kt * scale
                if keep is not None:
                    ds, p = ds * keep[..., j0:j1], p * keep[..., j0:j1]
                dk[b, j0:j1, h0:h1] += ((ds.transpose(-1, -2) @ qc).sum(1) * scale).permute(1, 0, 2)
                dv[b, j0:j1, h0:h1] += (p.transpose(-1, -2) @ doc).sum(1).permute(1, 0, 2)
            dq[b, :, h0 * G:h1 * G] = dqc.reshape(-1, Sq, D).permute(1, 0, 2)
    if rope is not None:
        dq, dk = rope_inv(dq, *rope), rope_inv(dk, *rope)
    return dq, dk, dv


def reference_bwd(do, q, k, v, o, lse, scale, causal, rope=None, **mut):
    """fp64 dQ, dK, dV from the given o, lse and do; rope = (cos, sin): dQ and dK rotated by -theta."""
    return _bwd(do, q, k, v, o, lse, scale, causal, torch.float64, False, None, rope, **mut)


def emulate_bwd(do, q, k, v, o, lse, scale, causal, rope=None, block=None, dq_f32=False, **mut):
    """dQ, dK, dV at the kernels' precision (bf16; dQ stays fp32 with dq_f32, the accumulate mode)."""
    dq, dk, dv = _bwd(do, q, k, v, o, lse, scale, causal, torch.float32, True, block, rope, **mut)
    return (dq if dq_f32 else dq.to(BF)), dk.to(BF), dv.to(BF)


# ------------------------------------------------------------------------------------------ the per-tile check
def tile_rows(S):
    """(first row, one past the last) of every tile of S rows: the aligned 32-row tiles, and for a ragged tail the
    last 32 rows (overlapping the tile before), so that every tile is 32 consecutive rows whenever S >= 32. A stub of
    one or two tail rows would be a tile made of planted rows only (the edge set holds the last two rows), whose dQ is
    what is left after P (dO V^T - delta) cancels for the saturated key: fp32 summation noise over a signal of ~1e-3
    of a plain row, on which honest implementations differ by more than any margin (measured on the kernels: 7e-3
    and 2.6e-2 of such a one-row tile against the emulation's 1e-3 and 5e-3; on the CPU an emulation that only sums
    its dot products in two halves misses the bound on such a stub by up to 10x:
    test_attn_tiles_host.py::test_tail_tile_is_32_consecutive_rows)."""
    tiles = [(r0, r0 + TILE) for r0 in range(0, S - TILE + 1, TILE)]
    if S % TILE:
        tiles.append((max(0, S - TILE), S))
    return tiles


def tile_norms(x):
    """fp64 [B, H, tiles]: the norm of every (batch, head, 32 consecutive rows) tile (tile_rows) of x [B, S, H, D]."""
    sq = x.double().pow(2).sum(-1).permute(0, 2, 1)  # [B, H, S]
    cs = torch.nn.functional.pad(sq.cumsum(-1), (1, 0))
    rows = tile_rows(x.shape[1])
    lo = torch.tensor([r[0] for r in rows], device=x.device)
    hi = torch.tensor([r[1] for r in rows], device=x.device)
    return (cs[..., hi] - cs[..., lo]).clamp_min(0).sqrt()


def tile_check(name, kernel, emul, ref, bf16_term=True, m=M_TILE):
    """The per-tile bound of the module docstring. Returns {"ok", "ratio" (worst err / bound), "output", "batch",
    "head", "row_block", "err_rel", "emul_rel" (that tile's kernel and emulation error over ||ref tile||)} of the
    worst tile; the bound comes from the emulation and the reference only."""
    err = tile_norms(kernel.double() - ref.double())
    eerr, rn = tile_norms(emul.double() - ref.double()), tile_norms(ref)
    bound = m * eerr + (BF16_RN if bf16_term else 0.0) * rn
    ratio = torch.where((err == 0) & (bound == 0), torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    i = int(ratio.argmax())
    H, n = ratio.shape[1], ratio.shape[2]
    worst = float(ratio.flatten()[i])
    rn = float(rn.flatten()[i]) or 1.0
    return {"ok": worst <= 1.0, "ratio": worst, "output": name, "batch": i // (H * n), "head": i // n % H,
            "row_block": i % n, "err_rel": float(err.flatten()[i]) / rn, "emul_rel": float(eerr.flatten()[i]) / rn}


def lse_check(lse, lse_ref):
    """max-abs per row against fp64 (the project's existing bound)."""
    d = (lse.double() - lse_ref.double()).abs()
    i = int(d.argmax())
    return {"ok": float(d.max()) < LSE_TOL, "err": float(d.max()), "index": i}


def worst_of(results):
    return max(results, key=lambda r_: r_["ratio"])


# ------------------------------------------------------------------------------------------ input sets
def edge_rows(S):
    """Rows next to multiples of 32 (so of 64, 128 and 256 too) on both sides, row 0 and the last two rows."""
    rows = {0, S - 1, S - 2}
    for x in range(0, S + 1, 32):
        rows.update((x - 1, x))
    return sorted(r_ for r_ in rows if 0 <= r_ < S)


def make_inputs(kind, B, Sq, Sk, Hq, Hkv, D, causal, device="cpu", seed=0):
    """q, k, v, do (bf16). kind:
    randn  plain.
    diag   causal: for rows r of the edge set, k[r] is planted along q[r] (first query head of the GQA group), so the
           diagonal key carries nearly all of row r's mass and losing it is an O(1) error. Non-causal: the keys of
           the edge set of Sk are planted for rows of the edge set of Sq in turn.
    bait   causal: k[r + 1] is planted that way: the key just above the diagonal would dominate row r if it leaked
           (above the last row stands the NaN guard row of the launch helpers). Non-causal: the planted key is
           Sk - 1, for row Sq - 1.
    The planted key is BETA sqrt(D) q[r] / |q[r]|^2, so its scaled score is BETA whatever |q[r]| is. A row's other
    scores are ~ N(0, 1) (at most ~ 4.5 over these lengths) or other planted keys (BETA cos(q[r], q[r']), at most
    ~ 0.45 BETA at D = 64), so BETA = 16 leads every row by at least 8 nats
    (test_attn_tiles_host.py::test_planted_keys_lead_their_rows). An input choice, not a tolerance."""
    gen = torch.Generator().manual_seed(seed * 7919 + Sq * 31 + Sk * 17 + Hq * 5 + Hkv * 3 + D + (1 if causal else 0))
    q, do = [torch.randn(B, Sq, Hq, D, generator=gen) for _ in range(2)]
    k, v = [torch.randn(B, Sk, Hkv, D, generator=gen) for _ in range(2)]
    G = Hq // Hkv
    if kind != "randn":
        q = q.to(BF).float()
        qh = q[:, :, ::G]                                   # [B, Sq, Hkv, D]: the first query head of every group
        plant = BETA * math.sqrt(D) * qh / qh.pow(2).sum(-1, keepdim=True)  # scaled score q . k / sqrt(D) = BETA
        if kind == "diag":
            if causal:
                rows = edge_rows(Sq)
                k[:, rows] = plant[:, rows]
            else:
                keys, rows = edge_rows(Sk), edge_rows(Sq)
                k[:, keys] = plant[:, [rows[i % len(rows)] for i in range(len(keys))]]
        elif kind == "bait":
            if causal:
                rows = [r_ for r_ in edge_rows(Sq) if r_ + 1 < Sk]
                if rows:
                    k[:, [r_ + 1 for r_ in rows]] = plant[:, rows]
            else:
                k[:, Sk - 1] = plant[:, Sq - 1]
        else:
            raise ValueError(kind)
    return [t.to(BF).to(device) for t in (q, k, v, do)]


def rope_tables(S, D, device="cpu", base=10000.0):
    """bf16 cos / sin [S, D/2]."""
    inv = 1.0 / (base ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    ang = torch.arange(S, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().to(BF).to(device), ang.sin().to(BF).to(device)


# ------------------------------------------------------------------------------------------ guard bands
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8, torch.int64: torch.int64,
        torch.int32: torch.int32}
INT_GUARD = -0x5A5A5A5A  # guard value of integer buffers (token ids, targets): no valid index


class Guards:
    """Allocates every tensor of a launch as a view inside a larger buffer whose other elements (guards) hold NaN
    (0xFF bytes for the byte workspace), and checks after the launch that the guards are bit-identical (compared as
    integers) and that the interior of every output holds no NaN (every element written)."""

    def __init__(self, device, g=8):
        assert g % 8 == 0
        self.dev, self.g, self.items = device, g, []

    def _add(self, name, buf, view, inside, output):
        self.items.append({"name": name, "buf": buf, "view": view, "inside": inside, "output": output})
        return view

    def _new(self, shape, dtype):
        if dtype == torch.uint8:
            return torch.full(shape, 0xFF, dtype=dtype, device=self.dev)
        if not dtype.is_floating_point:
            return torch.full(shape, INT_GUARD, dtype=dtype, device=self.dev)
        return torch.full(shape, math.nan, dtype=dtype, device=self.dev)

    def bshd(self, name, B, S, H, D, dtype=BF, data=None, fill=None, pad_heads=1):
        """[B, S, H, D] view: g guard rows before and after every batch's sequence and pad_heads guard heads. data:
        an input (copied in); fill: an output interior starting at a constant; neither: an output full of NaN."""
        g = self.g
        buf = self._new((B, S + 2 * g, H + pad_heads, D), dtype)
        view = buf[:, g:g + S, :H]
        inside = torch.zeros(buf.shape, dtype=torch.bool, device=self.dev)
        inside[:, g:g + S, :H] = True
        if data is not None:
            view.copy_(data)
        elif fill is not None:
            view.fill_(fill)
        return self._add(name, buf, view, inside, data is None)

    def flat(self, name, n, dtype, data=None, shape=None):
        """Offset contiguous view of n elements (lse, the workspace), 256 guard bytes on either side."""
        pad = 256 // torch.empty((), dtype=dtype).element_size()
        buf = self._new((n + 2 * pad,), dtype)
        view = buf[pad:pad + n]
        inside = torch.zeros(buf.shape, dtype=torch.bool, device=self.dev)
        inside[pad:pad + n] = True
        if data is not None:
            view.copy_(data.reshape(-1))
        return self._add(name, buf, view.view(shape) if shape else view, inside, data is None)

    def mat(self, name, rows, cols, dtype=BF, data=None, ld=None, shift=0, inout=False):
        """[rows, cols] view with row stride ld (default cols: row-contiguous) inside a flat buffer, 256 guard bytes
        (+ shift elements: a deliberately unaligned base) before the first row and after the last; with ld > cols
        the ld - cols elements between rows are guards too. data: copied in (an input; with inout an output that
        starts at data); no data: an output full of NaN."""
        ld = cols if ld is None else ld
        pad = 256 // torch.empty((), dtype=dtype).element_size()
        n = (rows - 1) * ld + cols if rows else 0
        buf = self._new((pad + shift + n + pad,), dtype)
        view = buf.as_strided((rows, cols), (ld, 1), pad + shift)
        inside = torch.zeros(buf.shape, dtype=torch.bool, device=self.dev)
        inside.as_strided((rows, cols), (ld, 1), pad + shift).fill_(True)
        if data is not None:
            view.copy_(data.reshape(rows, cols))
        return self._add(name, buf, view, inside, data is None or inout)

    def o_t(self, name, rows, cols, dtype=BF):
        """[rows, cols] view of a [rows + 2, ld] buffer, ld = cols rounded up to 8, + 8."""
        ld = (cols + 7) // 8 * 8 + 8
        buf = self._new((rows + 2, ld), dtype)
        view = buf[1:1 + rows, :cols]
        inside = torch.zeros(buf.shape, dtype=torch.bool, device=self.dev)
        inside[1:1 + rows, :cols] = True
        return self._add(name, buf, view, inside, True)

    def table(self, name, data):
        """RoPE table [S, D/2] with a wider row stride (8 guard columns) and g guard rows after the last."""
        S, h = data.shape
        buf = self._new((S + self.g, h + 8), data.dtype)
        view = buf[:S, :h]
        inside = torch.zeros(buf.shape, dtype=torch.bool, device=self.dev)
        inside[:S, :h] = True
        view.copy_(data)
        return self._add(name, buf, view, inside, False)

    def arm(self):
        """Snapshot every buffer (as integers) just before the launch."""
        for it in self.items:
            it["before"] = it["buf"].view(_INT[it["buf"].dtype]).clone()

    def check(self, written=()):
        """After the launch. written: names of inputs the launch also writes (q under rope_q). The workspace's
        interior is scratch: only its guards are checked."""
        for it in self.items:
            after = it["buf"].view(_INT[it["buf"].dtype])
            out = ~it["inside"]
            same = after[out] == it["before"][out]
            assert bool(same.all()), f"{it['name']}: {int((~same).sum())} guard elements changed"
            if it["output"] or it["name"] in written:
                if it["buf"].dtype.is_floating_point:
                    bad = torch.isnan(it["view"])
                    assert not bool(bad.any()), f"{it['name']}: {int(bad.sum())} interior elements are NaN"
            else:
                assert torch.equal(after, it["before"]), f"{it['name']}: an input was written"


# ------------------------------------------------------------------------------------------ launches (HIP device)
def launch_fwd(q, k, v, scale, causal, rope_q=None, want_o_t=False, g=8):
    """pico_attn_fwd on guarded buffers. q, k, v: plain bf16 inputs on the device; rope_q = (cos, sin): q is rotated
    in the kernel and written back. Returns {"o", "lse", "q" (as left by the launch), "o_t"} after the guard check."""
    import ctypes
    from picotron_amd import _lib, ops
    B, Sq, Hq, D = q.shape
    G = Guards(q.device, g)
    qg = G.bshd("q", B, Sq, Hq, D, data=q)
    kg = G.bshd("k", B, k.shape[1], k.shape[2], D, data=k)
    vg = G.bshd("v", B, k.shape[1], k.shape[2], D, data=v)
    og = G.bshd("o", B, Sq, Hq, D)
    lse = G.flat("lse", B * Hq * Sq, torch.float32, shape=(B, Hq, Sq))
    a = ops._attn_args(qg, kg, vg, og, lse, scale, causal)
    ot = None
    if want_o_t:
        ot = G.o_t("o_t", Hq * D, B * Sq)
        a.o_t, a.o_t_ld = _lib.ptr(ot), ot.stride(0)
    if rope_q is not None:
        cos, sin = G.table("cos", rope_q[0]), G.table("sin", rope_q[1])
        a.flags |= _lib.ATTN_ROPE_Q_FWD
        a.rope_cos, a.rope_sin, a.rope_stride = _lib.ptr(cos), _lib.ptr(sin), cos.stride(0)
        a.dq, a.dq_strides = _lib.ptr(qg), _lib.i64x3(qg.stride()[:3])
    G.arm()
    _lib.check(_lib.load().pico_attn_fwd(ctypes.byref(a), _lib.stream_of(q)), "pico_attn_fwd")
    torch.cuda.synchronize()
    G.check(written=("q",) if rope_q is not None else ())
    return {"o": og, "lse": lse, "q": qg, "o_t": ot}


DQ_FILL = 0.25  # the fp32 accumulator's starting constant


def launch_bwd(do, q, k, v, o, lse, scale, causal, mode="bf16", rope=None, g=8):
    """pico_attn_bwd on guarded buffers; mode: bf16 | f32acc (dQ added into an fp32 buffer that starts at DQ_FILL;
    returned with the constant taken off) | rope (RoPE^-1 of dQ / dK in the kernels). The workspace is sized by
    pico_attn_bwd_workspace_bytes and guarded. Returns (dq, dk, dv) after the guard check."""
    import ctypes
    from picotron_amd import _lib, ops
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Guards(q.device, g)
    qg, og, dog = [G.bshd(n, B, Sq, Hq, D, data=t) for n, t in (("q", q), ("o", o), ("do", do))]
    kg, vg = [G.bshd(n, B, Sk, Hkv, D, data=t) for n, t in (("k", k), ("v", v))]
    lg = G.flat("lse", B * Hq * Sq, torch.float32, data=lse, shape=(B, Hq, Sq))
    if mode == "f32acc":
        dq = G.bshd("dq", B, Sq, Hq, D, dtype=torch.float32, fill=DQ_FILL)
    else:
        dq = G.bshd("dq", B, Sq, Hq, D)
    dk, dv = G.bshd("dk", B, Sk, Hkv, D), G.bshd("dv", B, Sk, Hkv, D)
    a = ops._attn_args(qg, kg, vg, og, lg, scale, causal)
    a.dout, a.do_strides = _lib.ptr(dog), _lib.i64x3(dog.stride()[:3])
    a.dq, a.dk, a.dv = _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv)
    a.dq_strides, a.dk_strides, a.dv_strides = [_lib.i64x3(t.stride()[:3]) for t in (dq, dk, dv)]
    if mode == "f32acc":
        a.flags |= _lib.ATTN_DQ_F32_ACCUM
    if mode == "rope":
        cos, sin = G.table("cos", rope[0]), G.table("sin", rope[1])
        a.flags |= _lib.ATTN_ROPE_BWD
        a.rope_cos, a.rope_sin, a.rope_stride = _lib.ptr(cos), _lib.ptr(sin), cos.stride(0)
    lib = _lib.load()
    ws = G.flat("workspace", max(16, lib.pico_attn_bwd_workspace_bytes(ctypes.byref(a))), torch.uint8)
    a.workspace = _lib.ptr(ws)
    G.arm()
    _lib.check(lib.pico_attn_bwd(ctypes.byref(a), _lib.stream_of(q)), "pico_attn_bwd")
    torch.cuda.synchronize()
    G.check()
    return (dq - DQ_FILL if mode == "f32acc" else dq), dk, dv
