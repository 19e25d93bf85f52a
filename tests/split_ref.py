"""References, restatements, checks, input sets and guarded launches for the kernels that combine partial softmax
results (tests/test_split_host.py, tests/test_split_gpu.py): pico_attn_merge (csrc/attn_merge.hip, the ring's block
merge) and pico_attn_decode (csrc/attn_decode.hip, split-KV decode and its combine kernel). A plain helper module: no
fixture, no conftest; plain torch on any device except the launch helpers, which need the library and a HIP device.

Merge layout ("ring" layout) everywhere in this module: out / block_out [B, S, H, D], lse / block_lse [B, H, S]; the
row index of the kernel's lane mapping is (b S + s) H + h. The reference's layout ([B, H, S, D], lse [B, H, S, 1]) is
the same memory addressed with other strides: merge_operands(layout="bhsd").

ref_merge      fp64, the max-shifted form. Returns {name: (reference, cond)} for rowwise_ref.elem_check (U = 0: fp32
               outputs; K = K_ELEM per merge):
                   cond_out = |out| + w |out - block_out|     cond_lse = |lse| + |lse' - lse|
               The kernel's form out - w (out - block_out) rounds the difference and the product at the magnitude of
               |out - block_out| whatever w is, so its error is of the order of ulp(|out - block_out|) even where the
               result (1 - w) out + w block_out is tiny; a condition term built from the convex form, w |block_out|,
               misses that (an honest fp32 restatement then needs K ~ 2e4).
restate_merge  the same at the kernel's precision, from the header comment of attn_merge.hip: fp32,
               w = 1 / (1 + exp(-(bl - l))), lse' = l - (min(x, 0) - log1p(exp(-|x|))), x = l - bl. mut= names a
               deliberate mistake (MERGE_MUTANTS).
Decode         reference: generate._decode_reference (the CPU path of attention_decode) on .double() inputs;
               emulation: the same function on the bf16 inputs with the case's split_keys (fp32 math, bf16 output).
               decode_check: per (batch row, query head)
                   ||o - ref|| <= 2 ||emul - ref|| + 2^-9 ||ref||
               (margin and bf16 term of attn_ref.tile_check), and for the LSE elem_check with U = 0, K = K_ELEM and
                   cond = 1 + |m*| + |lse - m*|,   m* the row's largest scaled score in nats:
               the score itself carries the fp32 rounding of scale log2(e) and of the dot product (relative to |m*|),
               log(l) that of l and of the log (relative to |lse - m*|); 1 is the floor for rows with lse ~ m* ~ 0.
restate_decode the decode kernels' arithmetic in plain torch, fp32: chunks of split_keys keys, lane groups that each
               own every NG-th key of a chunk, DEC_UNROLL keys per group and loop trip with one rescale (alpha) per
               trip, the groups merged against their common maximum, the chunks combined in chunk order in the log2
               domain. mut= names a deliberate mistake (DECODE_MUTANTS).
"""
import math

import torch

import attn_ref as A
import rowwise_ref as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
K_ELEM = R.K_ELEM
M_ROW = A.M_TILE
OLD_MERGE_TOL = 1e-5                 # tests/test_kernels_gpu.py, "ring merge": max_abs of out and of lse
OLD_O_REL, OLD_LSE_ABS = 4e-3, 2e-3  # tests/test_generate_gpu.py: rel_l2 per batch row, max_abs of the lse
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453

# ------------------------------------------------------------------------------------------ merge: the case table
MERGE_DIMS = (8, 24, 40, 64, 96, 128, 136, 256)
MERGE_SHAPE = (2, 257, 8)  # B, S, H: 4112 rows
GAPS = (0.0, 1e-3, 1.0, 12.0, 20.0, 60.0, 87.0, 89.0, 104.0, 1e4)  # block_lse - lse, both signs
SIGNED_GAPS = tuple(s * g for g in GAPS for s in (1.0, -1.0))
MERGE_KINDS = ("randn", "gaps", "empty")
MERGE_MUTANTS = ("race", "sign", "lse_stale", "first_ignored", "bl_strides")
WAVE = 64


def merge_cases():
    """(D, kind, block_out fp32, first, layout) of the single-merge GPU cases: every D with every kind in the ring
    layout and bf16 blocks, and both block types x first x both layouts at D = 96 and 64."""
    c = [(D, kind, False, False, "bshd") for D in MERGE_DIMS for kind in MERGE_KINDS]
    c += [(D, "gaps", f32, first, layout) for D in (96, 64) for f32 in (False, True) for first in (False, True)
          for layout in ("bshd", "bhsd") if (f32, first, layout) != (False, False, "bshd")]
    return c


def parent_lanes(rows, D):
    """(row, sub) of every global lane under the mapping before the lane groups were padded: D / 8 consecutive
    global lanes per row. Reachable only here, as a restatement."""
    lpr = D // 8
    gid = torch.arange(rows * lpr)
    return gid // lpr, gid % lpr


def plan_lanes(rows, D):
    """(row, sub, live) of every lane of the grid under csrc/attn_merge_plan.h (restated; the header itself is
    swept by tests/attn_merge_plan_check.cpp, which also checks this equality for the powers of two)."""
    lpr = D // 8
    shift = (lpr - 1).bit_length()
    per_wg = 256 >> shift
    grid = (rows + per_wg - 1) // per_wg
    tid = torch.arange(256).repeat(grid)
    blk = torch.arange(grid).repeat_interleave(256)
    row, sub = blk * per_wg + (tid >> shift), tid & ((1 << shift) - 1)
    return row, sub, (sub < lpr) & (row < rows)


def straddles(rows, D):
    """bool [rows, D / 8]: lanes that sat in a later wave than their row's first lane under parent_lanes."""
    lpr = D // 8
    first = torch.arange(rows)[:, None] * lpr
    return (first + torch.arange(lpr)[None, :]) // WAVE != first // WAVE


def gap_of_rows(rows):
    """Index into SIGNED_GAPS per row: rows with the same residue mod 64 (so the same position in every wave
    pattern of parent_lanes, whose period divides 64 rows) walk through all 20 gaps."""
    r = torch.arange(rows)
    return (r // WAVE + r % WAVE) % len(SIGNED_GAPS)


def make_merge(kind, B, S, H, D, f32_block=False, seed=0):
    """out [B, S, H, D] fp32, lse [B, H, S] fp32, block_out (bf16 or fp32), block_lse fp32, on the CPU.
    randn  gaps block_lse - lse = randn * 3.
    gaps   every gap of SIGNED_GAPS, laid out by gap_of_rows over the rows (b S + s) H + h: sigmoid saturation at
           both ends (exp(-x) overflows fp32 beyond 88.7, its reciprocal underflows beyond 104), equal lse, 1e4.
    empty  block_lse = -inf with block_out = 0 (a block with no visible key): the running row must come back
           bit-identical."""
    gen = torch.Generator().manual_seed(seed * 7919 + B * 131 + S * 31 + H * 17 + D)
    out = torch.randn(B, S, H, D, generator=gen)
    lse = (torch.randn(B, H, S, generator=gen) * 3).contiguous()
    return (out, lse) + make_block(kind, lse, D, f32_block, seed)


def make_block(kind, lse, D, f32_block=False, seed=0):
    """(block_out [B, S, H, D], block_lse [B, H, S]) of the given kind for a running lse [B, H, S] (which may be a
    slice of a larger one: the rows of gap_of_rows are then the slice's own)."""
    B, H, S = lse.shape
    gen = torch.Generator().manual_seed(seed * 7919 + 1 + B * 131 + S * 31 + H * 17 + D)
    bo = torch.randn(B, S, H, D, generator=gen)
    if kind == "randn":
        bl = lse + torch.randn(B, H, S, generator=gen) * 3
    elif kind == "gaps":
        gap = torch.tensor(SIGNED_GAPS)[gap_of_rows(B * S * H)].reshape(B, S, H).permute(0, 2, 1)
        bl = lse + gap
    elif kind == "empty":
        bl = torch.full((B, H, S), -math.inf)
        bo = torch.zeros(B, S, H, D)
    else:
        raise ValueError(kind)
    return (bo if f32_block else bo.to(BF)), bl.contiguous()


def _w4(w):
    return w.permute(0, 2, 1)[..., None]  # [B, H, S] -> [B, S, H, 1]


def ref_merge(out, lse, bo, bl):
    """fp64 merge of one block; cond_out = |out| + w |out - bo|, cond_lse = |lse| + |lse' - lse|."""
    out, lse, bo, bl = out.double(), lse.double(), bo.double(), bl.double()
    m = torch.maximum(lse, bl)
    a, b = torch.exp(lse - m), torch.exp(bl - m)
    w = _w4(b / (a + b))
    new = (1 - w) * out + w * bo
    nl = m + torch.log(a + b)
    return {"out": (new, out.abs() + w * (out - bo).abs()), "lse": (nl, lse.abs() + (nl - lse).abs())}


def restate_merge(out, lse, bo, bl, first=False, mut=None):
    """The kernel's arithmetic in fp32 (module docstring). Returns {"out", "lse"} as new tensors. Mutants:
    race           columns 8 j .. 8 j + 7 of a row whose lane j sat in a later wave than the row's first lane
                   (straddles) take their weight from the already merged lse: the race of the unpadded mapping
    sign           the sigmoid's argument negated
    lse_stale      the lse is not updated
    first_ignored  a first block is merged into whatever out / lse hold instead of replacing them
    bl_strides     block_lse [B, H, S] is read with the (b, s, h) strides of out"""
    out, lse, bo, bl = out.float(), lse.float(), bo.float(), bl.float()
    B, S, H, D = out.shape
    if mut == "bl_strides":
        bl = bl.contiguous().reshape(B, S, H).permute(0, 2, 1)
    if first and mut != "first_ignored":
        return {"out": bo.clone(), "lse": bl.clone()}
    x = lse - bl
    nl = lse - (torch.minimum(x, torch.zeros_like(x)) - torch.log1p(torch.exp(-x.abs())))
    arg = bl - lse
    w = _w4(1.0 / (1.0 + torch.exp(arg if mut == "sign" else -arg))).expand(B, S, H, D)
    if mut == "race":
        w2 = _w4(1.0 / (1.0 + torch.exp(-(bl - nl))))
        late = straddles(B * S * H, D).reshape(B, S, H, D // 8).repeat_interleave(8, -1)
        w = torch.where(late, w2.expand(B, S, H, D), w)
    new = out - w * (out - bo)
    return {"out": new, "lse": lse.clone() if mut == "lse_stale" else nl}


def check_merge(tag, got, ref, k=K_ELEM, worst_k=None):
    """elem_check of out and lse (U = 0) with budget k; prints one line per output and asserts."""
    R.check_all(tag, {n: got[n].cpu() for n in ref}, ref, k, worst_k)


def merge_results(got, ref, k=K_ELEM):
    return [R.elem_check(n, got[n].cpu(), r_, c_, F32, k) for n, (r_, c_) in ref.items()]


def ref_chain(blocks):
    """fp64 chain over [(block_out, block_lse), ...] on the given (already rounded) inputs: {name: (reference, cond)}
    with cond the maximum over the steps of the per-step cond; the budget of the check is K_ELEM (N - 1)."""
    out, lse = blocks[0][0].double(), blocks[0][1].double()
    co, cl = out.abs(), lse.abs()
    for bo, bl in blocks[1:]:
        r_ = ref_merge(out, lse, bo, bl)
        co, cl = torch.maximum(co, r_["out"][1]), torch.maximum(cl, r_["lse"][1])
        out, lse = r_["out"][0], r_["lse"][0]
    return {"out": (out, co), "lse": (lse, cl)}


def restate_chain(blocks):
    cur = restate_merge(blocks[0][0], blocks[0][1], blocks[0][0], blocks[0][1], first=True)
    for bo, bl in blocks[1:]:
        cur = restate_merge(cur["out"], cur["lse"], bo, bl)
    return cur


def make_chain(n, B, S, H, D, keys=16, seed=0):
    """n blocks of `keys` keys each of one softmax per (b, s, h) row: the blocks' partial results in fp64
    ([(out [B, S, H, D], lse [B, H, S])]) and the whole softmax's (out, lse). Block i's scores are shifted by
    3 (i - n / 2) so that the running maximum moves along the chain."""
    gen = torch.Generator().manual_seed(seed * 7919 + n * 977 + B * 131 + S * 31 + H * 17 + D)
    s = torch.randn(B, S, H, n, keys, generator=gen, dtype=F64) * 2
    s = s + 3.0 * (torch.arange(n, dtype=F64) - n / 2)[:, None]
    v = torch.randn(B, S, H, n, keys, D, generator=gen, dtype=F64)
    blocks = []
    for i in range(n):
        p = torch.softmax(s[..., i, :], -1)
        blocks.append((torch.einsum("bshk,bshkd->bshd", p, v[..., i, :, :]),
                       torch.logsumexp(s[..., i, :], -1).permute(0, 2, 1).contiguous()))
    p = torch.softmax(s.reshape(B, S, H, n * keys), -1)
    whole = (torch.einsum("bshk,bshkd->bshd", p, v.reshape(B, S, H, n * keys, D)),
             torch.logsumexp(s.reshape(B, S, H, n * keys), -1).permute(0, 2, 1).contiguous())
    return blocks, whole


# ------------------------------------------------------------------------------------------ decode: the case table
DEC_DIMS = (64, 128)
DEC_GROUPS = tuple(range(1, 9))
DEC_HKV = 2
DEC_KINDS = ("randn", "large", "ascending", "descending")
DECODE_MUTANTS = ("drop_chunk_start", "drop_trip", "drop_group", "leak_len", "no_alpha", "kv_neighbour", "combine8",
                  "empty_o")
DEC_UNROLL = 4  # csrc/attn_decode_plan.h (asserted against the header by test_split_host.py)
DEC_DEFAULT = 256  # DEC_MIN_SPLIT


def dec_trip(D):
    return 256 // (D // 8) * DEC_UNROLL


def dec_ng(D):
    return 256 // (D // 8)


def dec_smax(D):
    return 2 * dec_trip(D) + 37


def dec_splits(D):
    """split_keys of the case table; None: the library's default rule (DEC_MIN_SPLIT = 256 keys at these cache
    lengths on any chip of 15 CUs or more: two chunks at D = 64, one at D = 128). The emulation and the restatement
    take the chunk length itself: generate.default_split_keys on the GPU, DEC_DEFAULT on the host."""
    t = dec_trip(D)
    return (1, 7, 32, t - 1, t, t + 1, 2 * t + 5, None, dec_split8(D))


def dec_split8(D):
    """The chunk length that gives exactly 8 chunks: one whole trip of the combine kernel's loops, unrolled by 8."""
    return (dec_smax(D) + 7) // 8


def dec_lens(D, split):
    """One batch row per length: the edges of the kernel's loops, and of the chunk where they differ."""
    t, ng, s = dec_trip(D), dec_ng(D), dec_smax(D)
    lens = [-3, 0, 1, ng - 1, ng, ng + 1, t - 1, t, t + 1, s - 1, s, s + 5]
    for x in (() if split is None else (split - 1, split, split + 1)):
        if x not in lens:
            lens.append(x)
    return tuple(lens)


def dec_cases():
    """(D, G, split_keys, kind) of the GPU grid: per <D, G> instance `ascending` at every multi-trip split (trip + 1
    and 2 trip + 5: two and three loop trips in a chunk, so every unroll slot and the rescale see live keys), `randn`
    at split 7 (43 or 24 chunks: the combine's unrolled trips and its tail), and one further (split, kind) pair
    that walks through the other splits and kinds as G goes up, so that every split and every kind runs at both D."""
    cases = []
    for D in DEC_DIMS:
        t = dec_trip(D)
        rest = [(1, "large"), (32, "descending"), (t - 1, "large"), (t, "descending"), (None, "randn"),
                (dec_split8(D), "large"), (None, "large"), (dec_split8(D), "descending")]
        for G in DEC_GROUPS:
            cases += [(D, G, t + 1, "ascending"), (D, G, 2 * t + 5, "ascending"), (D, G, 7, "randn"),
                      (D, G) + rest[G - 1]]
    return cases


def make_decode(kind, G, D, lens, S=None, Hkv=DEC_HKV, seed=0, stale_nan=True):
    """q [B, Hq, D], k / v [B, Hkv, S, D] bf16 and seqlens int32 [B] on the CPU, one batch row per length.
    randn       plain.
    large       q x 20: scores of standard deviation 20.
    ascending   the score of key j for the first query head of each group rises linearly from -30 to +30 over the
                cache (k[j] = t_j sqrt(D) q / |q|^2 plus a part orthogonal to q): every loop trip and every chunk
                raises the maximum.
    descending  the same from +30 down to -30.
    stale_nan: the cache rows at and beyond seqlens[b] hold NaN."""
    S = dec_smax(D) if S is None else S
    B, Hq = len(lens), G * Hkv
    kid = DEC_KINDS.index(kind)
    gen = torch.Generator().manual_seed(seed * 7919 + kid * 101 + G * 1009 + D * 13 + S + B)
    q = torch.randn(B, Hq, D, generator=gen)
    k = torch.randn(B, Hkv, S, D, generator=gen)
    v = torch.randn(B, Hkv, S, D, generator=gen)
    if kind == "large":
        q = q * 20
    elif kind in ("ascending", "descending"):
        q = q.to(BF).float()
        qh = q[:, ::G]                                                # [B, Hkv, D]
        n2 = qh.pow(2).sum(-1, keepdim=True)
        t = torch.linspace(-30.0, 30.0, S)
        t = t.flip(0) if kind == "descending" else t
        k = k - (k * qh[:, :, None]).sum(-1, keepdim=True) * qh[:, :, None] / n2[:, :, None]
        k = k + t[None, None, :, None] * math.sqrt(D) * (qh / n2)[:, :, None]
    elif kind != "randn":
        raise ValueError(kind)
    q, k, v = q.to(BF), k.to(BF), v.to(BF)
    if stale_nan:
        for b, n in enumerate(lens):
            n = min(max(n, 0), S)
            k[b, :, n:] = math.nan
            v[b, :, n:] = math.nan
    return q, k, v, torch.tensor(lens, dtype=torch.int32)


def decode_ref(q, k, v, lens, scale, split):
    """{"o_ref", "lse_ref" (fp64), "o_emul" (bf16), "lse_emul", "mstar" (fp64 [B, Hq]: the largest scaled score of
    the row, 0 for an empty row)}. Every case of the tables has inputs of its own, so nothing is shared."""
    from picotron_amd import generate as GEN
    B, Hq, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    o_ref, lse_ref = GEN.attention_decode(q.double(), k.double(), v.double(), lens, scale, None, True)
    o_emul, lse_emul = GEN.attention_decode(q, k, v, lens, scale, split, True)
    live = torch.arange(S)[None, :] < lens.to(torch.int64).clamp(0, S)[:, None]
    kd = torch.where(live[:, None, :, None], k.double(), torch.zeros((), dtype=F64))
    s = torch.einsum("bhgd,bhsd->bhgs", q.double().view(B, Hkv, Hq // Hkv, D), kd) * scale
    s = s.masked_fill(~live[:, None, None, :], -math.inf).amax(-1).reshape(B, Hq)
    out = {"o_ref": o_ref, "lse_ref": lse_ref, "o_emul": o_emul, "lse_emul": lse_emul,
           "mstar": torch.where(torch.isinf(s), torch.zeros_like(s), s)}
    return out


def decode_check(tag, o, lse, ref, m=M_ROW, k=K_ELEM, worst=None, quiet=False):
    """The two bounds of the module docstring; every value finite except the lse of an empty row, which must be
    -inf with o = 0. Returns {"ok", "ratio" (worst O row over its bound), "k" (LSE K needed), "row"}; prints the
    figures before anything is asserted by the caller. worst: optional dict collecting the largest of each."""
    o, lse = o.cpu(), lse.cpu()
    O, L = ref["o_ref"], ref["lse_ref"]
    empty = torch.isinf(L) & (L < 0)
    finite = bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse[~empty]).all())
    empty_ok = bool((lse[empty] == -math.inf).all()) and bool((o[empty] == 0).all())
    err = (o.double() - O).norm(dim=-1)
    bound = m * (ref["o_emul"].double() - O).norm(dim=-1) + A.BF16_RN * O.norm(dim=-1)
    ratio = torch.where((err == 0) & (bound == 0), torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    i = int(ratio.argmax())
    z = torch.zeros_like(L)
    got_l = torch.where(empty, z.float(), lse)
    ref_l = torch.where(empty, z, L)
    r_ = R.elem_check("lse", got_l, ref_l, 1 + ref["mstar"].abs() + (ref_l - ref["mstar"]).abs(), F32, k)
    res = {"ok": finite and empty_ok and float(ratio.max()) <= 1.0 and r_["ok"], "ratio": float(ratio.max()),
           "k": r_["k"], "row": (i // o.shape[1], i % o.shape[1]), "finite": finite, "empty_ok": empty_ok,
           "lse_index": r_["index"]}
    if not quiet:
        print(f"DECODE {tag} O ratio {res['ratio']:.3g} at (b, h) {res['row']}; LSE K {res['k']:.2f} at "
              f"{res['lse_index']}; finite {finite}, empty rows {empty_ok}")
    if worst is not None:
        worst["decode.o_ratio"] = max(worst.get("decode.o_ratio", 0.0), res["ratio"])
        worst["decode.lse_k"] = max(worst.get("decode.lse_k", 0.0), res["k"])
    return res


def decode_old_ok(o, lse, ref):
    """The criterion of tests/test_generate_gpu.py: rel_l2 < 4e-3 over the tensor and per batch row, LSE max_abs
    < 2e-3 (rows of length 0 left out, as there)."""
    o, lse, O, L = o.cpu().double(), lse.cpu().double(), ref["o_ref"], ref["lse_ref"]
    live = ~(torch.isinf(L) & (L < 0))
    if not (bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse[live]).all())):
        return False
    rows = [b for b in range(o.shape[0]) if bool(live[b].any())]
    per_row = all(A.rel_l2(o[b], O[b]) < OLD_O_REL for b in rows)
    return per_row and A.rel_l2(o, O) < OLD_O_REL and float((lse[live] - L[live]).abs().max()) < OLD_LSE_ABS


def _ex2(x):
    return torch.exp2(x)


def restate_decode(q, k, v, lens, scale, split, mut=None, ws_fill=1.0):
    """The decode kernels' arithmetic (module docstring) in fp32 on the CPU: (o bf16 [B, Hq, D], lse fp32 [B, Hq]).
    ws_fill: what the never-written workspace o of an empty chunk holds (only the empty_o mutant reads it). Mutants:
    drop_chunk_start  the first key of every chunk after the first is lost
    drop_trip         the first key of every loop trip after a chunk's first is lost
    drop_group        the first key of every chunk's second row of lane groups (chunk start + NG) is lost
    leak_len          the key at index len is treated as live (the cache holds finite stale rows in that test)
    no_alpha          the running sums are not rescaled when a trip raises the maximum
    kv_neighbour      the last query head of every group reads the next kv head
    combine8          the combine stops at the last multiple of 8 chunks
    empty_o           an empty chunk's workspace o is added with weight 1"""
    B, Hq, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    G = Hq // Hkv
    ng, trip = dec_ng(D), dec_trip(D)
    sk = S if split is None else int(split)
    nsplit = (S + sk - 1) // sk
    n = lens.to(torch.int64).clamp(0, S)
    if mut == "leak_len":
        n = (n + 1).clamp(max=S)
    qf = q.float().view(B, Hkv, G, D)
    kf, vf = k.float(), v.float()
    if mut == "kv_neighbour":
        kx = torch.stack([kf] * G, 2)                       # [B, Hkv, G, S, D]
        vx = torch.stack([vf] * G, 2)
        kx[:, :, G - 1], vx[:, :, G - 1] = kf.roll(-1, 1), vf.roll(-1, 1)
    else:
        kx, vx = kf[:, :, None].expand(B, Hkv, G, S, D), vf[:, :, None].expand(B, Hkv, G, S, D)
    sl2 = torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    ninf = torch.tensor(-math.inf)
    pm = torch.full((B, Hkv, G, nsplit), -math.inf)
    pl = torch.zeros(B, Hkv, G, nsplit)
    po = torch.full((B, Hkv, G, nsplit, D), float(ws_fill))
    keys = torch.arange(S)
    for c in range(nsplit):
        c0 = c * sk
        end = torch.minimum(torch.tensor(c0 + sk), n)        # [B]
        if not bool((end > c0).any()):
            continue
        m = torch.full((B, Hkv, G, ng), -math.inf)
        l = torch.zeros(B, Hkv, G, ng)
        acc = torch.zeros(B, Hkv, G, ng, D)
        for base in range(c0, min(c0 + sk, S), trip):
            idx = base + torch.arange(DEC_UNROLL)[:, None] * ng + torch.arange(ng)[None, :]  # [U, ng]
            live = idx[None] < end[:, None, None]                                             # [B, U, ng]
            if mut == "drop_chunk_start" and c > 0:
                live = live & (idx != c0)[None]
            if mut == "drop_trip" and base > c0:
                live = live & (idx != base)[None]
            if mut == "drop_group":
                live = live & (idx != c0 + ng)[None]
            row = idx.clamp(max=S - 1)
            kk = torch.nan_to_num(kx[:, :, :, row])                                           # [B, Hkv, G, U, ng, D]
            vv = torch.nan_to_num(vx[:, :, :, row])
            s = torch.einsum("bhgd,bhgund->bhgun", qf, kk) * sl2
            lv = live[:, None, None]
            s = torch.where(lv, s, ninf)
            mn = torch.maximum(m, s.amax(3))
            ms = torch.where(mn == -math.inf, torch.zeros_like(mn), mn)
            alpha = torch.ones_like(m) if mut == "no_alpha" else _ex2(m - ms)
            p = _ex2(s - ms[:, :, :, None])
            l = l * alpha + p.sum(3)
            acc = acc * alpha[..., None] + torch.einsum("bhgun,bhgund->bhgnd", p, vv)
            m = mn
        mt = m.amax(-1)
        ms = torch.where(mt == -math.inf, torch.zeros_like(mt), mt)
        sc = _ex2(m - ms[..., None])
        wrote = (end > c0)[:, None, None].expand(B, Hkv, G)
        pm[..., c] = torch.where(wrote, mt, ninf)
        pl[..., c] = torch.where(wrote, (l * sc).sum(-1), torch.zeros(()))
        po[..., c, :] = torch.where(wrote[..., None], (acc * sc[..., None]).sum(-2), po[..., c, :])
    upto = nsplit // 8 * 8 if mut == "combine8" and nsplit >= 8 else nsplit
    mt = pm[..., :upto].amax(-1)
    acc, lt = torch.zeros(B, Hkv, G, D), torch.zeros(B, Hkv, G)
    for c in range(upto):
        mc = pm[..., c]
        empty = mc == -math.inf
        sc = torch.where(empty, torch.zeros(()), _ex2(mc - mt))
        oc = po[..., c, :]
        if mut == "empty_o":
            sc_o = torch.where(empty, torch.ones(()), sc)
        else:
            sc_o, oc = sc, torch.where(empty[..., None], torch.zeros(()), oc)
        lt = lt + pl[..., c] * sc
        acc = acc + oc * sc_o[..., None]
    any_ = lt > 0
    o = torch.where(any_[..., None], acc / lt.clamp_min(1e-38)[..., None], torch.zeros(()))
    lse = torch.where(any_, mt * torch.tensor(LN2, dtype=F32) + torch.log(lt.clamp_min(1e-38)), ninf)
    return o.reshape(B, Hq, D).to(BF), lse.reshape(B, Hq)


# ------------------------------------------------------------------------------------------ launches (HIP device)
def _lib():
    from picotron_amd import _lib as L
    return L, L.load()


def merge_operands(G, out0, lse0, bo, bl, layout="bshd", first=False, sl=None):
    """The four operands of one merge as views inside NaN-filled guard buffers of G (attn_ref.Guards), on G's
    device. Inputs in the ring layout on any device; bo / bl have the shape of the slice sl = (seq slice, head
    slice) of out / lse when it is given. layout bshd: views out [B, S, H, D], lse [B, H, S]; bhsd: the
    reference's, out [B, H, S, D], lse [B, H, S, 1], block_out [B, H, S, D], block_lse [B, H, S]. first: out and lse
    start as NaN (every element must be written). Returns {"out", "lse", "bo", "bl"}."""
    B, S, H, D = out0.shape
    Sb, Hb = bo.shape[1], bo.shape[2]
    if layout == "bshd":
        out = G.bshd("out", B, S, H, D, dtype=F32, data=None if first else out0)
        bov = G.bshd("block_out", B, Sb, Hb, D, dtype=bo.dtype, data=bo)
        lse = G.flat("lse", B * H * S, F32, data=None if first else lse0, shape=(B, H, S))
    else:
        out = G.bshd("out", B, H, S, D, dtype=F32, data=None if first else out0.permute(0, 2, 1, 3))
        bov = G.bshd("block_out", B, Hb, Sb, D, dtype=bo.dtype, data=bo.permute(0, 2, 1, 3))
        lse = G.flat("lse", B * H * S, F32, data=None if first else lse0, shape=(B, H, S, 1))
    blv = G.flat("block_lse", B * Hb * Sb, F32, data=bl, shape=(B, Hb, Sb))
    return {"out": out, "lse": lse, "bo": bov, "bl": blv}


def ring_view(ops, layout):
    """(out [B, S, H, D], lse [B, H, S]) views of merge_operands' out / lse."""
    if layout == "bshd":
        return ops["out"], ops["lse"]
    return ops["out"].permute(0, 2, 1, 3), ops["lse"][..., 0]


def run_guarded_merge(G, ops, layout, fn, sl=None):
    """Arms the guards, runs fn(), checks the guards and that everything of out / lse outside the slice sl is
    bit-identical. Returns (out [B, S, H, D], lse [B, H, S]) views."""
    out, lse = ring_view(ops, layout)
    before = (out.clone(), lse.clone())
    G.arm()
    fn()
    torch.cuda.synchronize()
    G.check(written=("out", "lse"))
    if sl is not None:
        ss, hs = sl
        for name, now, was, idx in (("out", out, before[0], (slice(None), ss, hs)),
                                    ("lse", lse, before[1], (slice(None), hs, ss))):
            keep = now.clone()
            keep[idx] = was[idx]
            assert torch.equal(keep.view(torch.int32), was.view(torch.int32)), f"{name}: written outside the slice"
    return out, lse


def launch_merge(out0, lse0, bo, bl, first=False, layout="bshd", sl=None, device="cuda"):
    """pico_attn_merge through the C ABI on guarded buffers (merge_operands): merges the block into the slice sl of
    the running out / lse (everything when None). Returns {"out" [B, S, H, D], "lse" [B, H, S]} after the guard
    and outside-the-slice checks."""
    L, lib = _lib()
    G = A.Guards(device)
    ops = merge_operands(G, out0, lse0, bo, bl, layout, first, sl)
    out, lse = ring_view(ops, layout)
    bov = ops["bo"] if layout == "bshd" else ops["bo"].permute(0, 2, 1, 3)
    ss, hs = sl if sl is not None else (slice(None), slice(None))
    ov, lv = out[:, ss, hs], lse[:, hs, ss]
    B, S, H, D = bov.shape
    assert ov.shape == bov.shape and lv.shape == ops["bl"].shape

    def fn():
        L.check(lib.pico_attn_merge(L.ptr(ov), L.i64x3(ov.stride()[:3]), L.ptr(lv), L.i64x3(lv.stride()), L.ptr(bov),
                                    L.i64x3(bov.stride()[:3]), 1 if bov.dtype == F32 else 0, L.ptr(ops["bl"]),
                                    L.i64x3(ops["bl"].stride()), B, S, H, D, 1 if first else 0, L.stream_of(ov)),
                "pico_attn_merge")

    out, lse = run_guarded_merge(G, ops, layout, fn, sl)
    return {"out": out, "lse": lse}


def launch_decode(q, k, v, lens, scale, split, device="cuda"):
    """pico_attn_decode through the C ABI on guarded buffers: q rows strided (a guard head after every row's
    heads), the caches windows of larger allocations (guard kv heads before and after, a guard key row after every
    head's S_max rows), o and lse inside NaN, the workspace 0xFF inside and outside (an empty chunk's never-written
    o is NaN bits). Returns {"o" [B, Hq, D] bf16, "lse" [B, Hq]} after the guard check."""
    L, lib = _lib()
    B, Hq, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    G = A.Guards(device)
    qg = G.bshd("q", B, 1, Hq, D, data=q[:, None])[:, 0]
    kg, vg = G.bshd("k", B, Hkv, S, D, data=k), G.bshd("v", B, Hkv, S, D, data=v)
    lg = G.flat("seqlens", B, torch.int32, data=lens)
    o = G.mat("o", B * Hq, D)
    lse = G.flat("lse", B * Hq, F32, shape=(B, Hq))
    sk = 0 if split is None else int(split)
    nbytes = int(lib.pico_attn_decode_workspace_bytes(B, Hq, Hkv, S, D, sk))
    assert nbytes > 0, lib.pico_last_error()
    ws = G.flat("workspace", nbytes, torch.uint8)
    qs = (L.c_i64 * 2)(qg.stride(0), qg.stride(1))
    G.arm()
    L.check(lib.pico_attn_decode(L.ptr(qg), qs, L.ptr(kg), L.i64x3(kg.stride()[:3]), L.ptr(vg), L.i64x3(vg.stride()[:3]),
                                 L.ptr(lg), L.ptr(o), L.ptr(lse), L.ptr(ws), B, Hq, Hkv, S, D, scale, sk,
                                 L.stream_of(qg)), "pico_attn_decode")
    torch.cuda.synchronize()
    G.check()
    return {"o": o.view(B, Hq, D), "lse": lse}
