"""pico_attn_merge, pico_attn_decode (both kernels) and the ring forward on the GPU under the bounds, guard bands and
case tables of tests/split_ref.py (tried on the CPU by tests/test_split_host.py):

merge   every head dim of the table (the multiples of 8 whose rows the unpadded lane mapping split over two waves
        among them) x randn / every lse gap / an empty block, bf16 and fp32 blocks, first and later merges, the
        ring's layout and the reference's, through the C ABI and through _merge_bshd / update_out_and_lse, slices of
        query rows and of heads (everything outside bit-identical), an 8-block chain against the fp64 chain;
decode  all 16 <D, G> instances x the split / kind grid of split_ref.dec_cases, one batch row per edge length, NaN
        in the cache beyond every length, a workspace of 0xFF bytes, strided q and cache windows;
ring    RingAttentionFunc.forward for every rank of a 2- and 4-rank ring in one process (a stub ContextCommunicate
        hands each rank the K / V shards it would receive), contiguous and zig-zag, GQA and D = 128, per-tile bound
        against the fp64 whole-sequence attention.
The worst K and ratio per output are printed by the last test of the file."""
import math

import pytest
import torch

import attn_ref as A
import split_ref as SR

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
WORST = {}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _check_one_merge(tag, got, out0, lse0, bo, bl, first, kind, k=SR.K_ELEM):
    if first:  # a copy: block_out as fp32, block_lse
        assert torch.equal(_bits(got["out"].cpu()), _bits(bo.float())) and torch.equal(_bits(got["lse"].cpu()), _bits(bl))
        return
    assert torch.isfinite(got["out"]).all() and torch.isfinite(got["lse"]).all()
    SR.check_merge(tag, got, SR.ref_merge(out0, lse0, bo, bl), k, WORST)
    if kind == "empty":
        assert torch.equal(_bits(got["out"].cpu()), _bits(out0)) and torch.equal(_bits(got["lse"].cpu()), _bits(lse0))


# ------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("D,kind,f32,first,layout", SR.merge_cases())
def test_merge(D, kind, f32, first, layout):
    out0, lse0, bo, bl = SR.make_merge(kind, *SR.MERGE_SHAPE, D, f32)
    got = SR.launch_merge(out0, lse0, bo, bl, first=first, layout=layout)
    _check_one_merge(f"merge D={D} {kind} f32={int(f32)} {layout}", got, out0, lse0, bo, bl, first, kind)


@pytest.mark.parametrize("D", [64, 128])
def test_merge_pow2_dims_keep_their_lanes_and_bits(D):
    """At D = 64 and 128 every lane serves the row and the columns it served before the lane groups were padded
    (the old mapping exists only as split_ref.parent_lanes), and an element's result does not depend on the mapping:
    the same rows as the first D columns of a wider, padded-group problem (D + 8: 9 or 17 lanes in groups of 16 or
    32) come out bit-identical. So the results at D = 64 and 128 are the bits they were."""
    rows = math.prod(SR.MERGE_SHAPE)
    row, sub, live = SR.plan_lanes(rows, D)
    prow, psub = SR.parent_lanes(rows, D)
    n = prow.numel()
    assert bool(live[:n].all()) and not bool(live[n:].any())
    assert torch.equal(row[:n], prow) and torch.equal(sub[:n], psub)
    out0, lse0, bo, bl = SR.make_merge("gaps", *SR.MERGE_SHAPE, D)
    got = SR.launch_merge(out0, lse0, bo, bl)
    wide = [torch.cat([t, t[..., :8]], -1) for t in (out0, bo)]
    got_w = SR.launch_merge(wide[0], lse0, wide[1], bl)
    assert torch.equal(_bits(got["out"]), _bits(got_w["out"][..., :D])) and torch.equal(_bits(got["lse"]), _bits(got_w["lse"]))


@pytest.mark.parametrize("D", [96, 64])
@pytest.mark.parametrize("which", ["rows", "heads"])
@pytest.mark.parametrize("layout", ["bshd", "bhsd"])
def test_merge_into_a_slice(layout, which, D):
    """A merge into a slice of query rows (the zig-zag second half) or of heads leaves everything outside it
    bit-identical (checked in run_guarded_merge) and the slice within the bound."""
    B, S, H = SR.MERGE_SHAPE
    sl = (slice(129, None), slice(None)) if which == "rows" else (slice(None), slice(3, 6))
    out0, lse0, _, _ = SR.make_merge("gaps", B, S, H, D)
    bo, bl = SR.make_block("gaps", lse0[:, sl[1], sl[0]], D, which == "heads", seed=1)
    got = SR.launch_merge(out0, lse0, bo, bl, layout=layout, sl=sl)
    part = {"out": got["out"][:, sl[0], sl[1]], "lse": got["lse"][:, sl[1], sl[0]]}
    SR.check_merge(f"merge slice {which} D={D} {layout}", part,
                   SR.ref_merge(out0[:, sl[0], sl[1]], lse0[:, sl[1], sl[0]], bo, bl), SR.K_ELEM, WORST)


@pytest.mark.parametrize("D,f32", [(96, False), (40, True), (128, False)])
def test_merge_bshd_api(D, f32):
    """The ring's own entry: _merge_bshd allocates on the first block and merges in place afterwards."""
    from picotron_amd.context_parallel import context_parallel as CP
    out0, lse0, bo, bl = SR.make_merge("gaps", *SR.MERGE_SHAPE, D, f32)
    o1, l1 = CP._merge_bshd(None, None, bo.to(DEV), bl.to(DEV))
    assert o1.dtype == F32 and torch.equal(_bits(o1.cpu()), _bits(bo.float())) and torch.equal(_bits(l1.cpu()), _bits(bl))
    G = A.Guards(DEV)
    ops = SR.merge_operands(G, out0, lse0, bo, bl)
    out, lse = SR.run_guarded_merge(G, ops, "bshd", lambda: CP._merge_bshd(ops["out"], ops["lse"], ops["bo"], ops["bl"]))
    SR.check_merge(f"merge _merge_bshd D={D}", {"out": out, "lse": lse}, SR.ref_merge(out0, lse0, bo, bl), SR.K_ELEM, WORST)


@pytest.mark.parametrize("D,f32,which", [(96, False, "all"), (136, True, "rows"), (24, False, "heads"),
                                         (64, False, "rows")])
def test_update_out_and_lse_api(D, f32, which):
    """The reference's entry and layout ([B, H, S, D], lse [B, H, S, 1]): an in-place slice_ merge (the whole
    tensor, query rows, heads) on guarded buffers, and the rebinding non-slice merge."""
    from picotron_amd.context_parallel import context_parallel as CP
    B, S, H = SR.MERGE_SHAPE
    sl = {"all": (slice(None), slice(None)), "rows": (slice(129, None), slice(None)),
          "heads": (slice(None), slice(3, 6))}[which]
    out0, lse0, _, _ = SR.make_merge("randn", B, S, H, D)
    bo, bl = SR.make_block("randn", lse0[:, sl[1], sl[0]], D, f32, seed=2)
    G = A.Guards(DEV)
    ops = SR.merge_operands(G, out0, lse0, bo, bl, layout="bhsd")
    slice_ = (slice(None), sl[1], sl[0])
    out, lse = SR.run_guarded_merge(
        G, ops, "bhsd", lambda: CP.update_out_and_lse(ops["out"], ops["lse"], ops["bo"], ops["bl"], slice_=slice_), sl)
    ref = SR.ref_merge(out0[:, sl[0], sl[1]], lse0[:, sl[1], sl[0]], bo, bl)
    SR.check_merge(f"merge update_out_and_lse {which} D={D}",
                   {"out": out[:, sl[0], sl[1]], "lse": lse[:, sl[1], sl[0]]}, ref, SR.K_ELEM, WORST)
    if which == "all":  # without slice_: new tensors, the caller's untouched
        o0, l0 = out0.permute(0, 2, 1, 3).contiguous().to(DEV), lse0[..., None].to(DEV)
        keep = (o0.clone(), l0.clone())
        o2, l2 = CP.update_out_and_lse(o0, l0, bo.permute(0, 2, 1, 3).to(DEV), bl.to(DEV))
        assert torch.equal(o0, keep[0]) and torch.equal(l0, keep[1])
        SR.check_merge(f"merge update_out_and_lse rebinding D={D}", {"out": o2.permute(0, 2, 1, 3), "lse": l2[..., 0]},
                       ref, SR.K_ELEM, WORST)


@pytest.mark.parametrize("D", [96, 128])
def test_merge_chain_of_8(D):
    """Eight partial softmax results of one row (rounded to the kernel's input types) merged in turn, against the
    fp64 chain on the same rounded inputs: cond the largest per-step cond, budget K_ELEM (N - 1)."""
    n = 8
    blocks, _ = SR.make_chain(n, 1, 129, 4, D, keys=4)
    blocks = [(bo.to(BF), bl.float()) for bo, bl in blocks]
    out0, lse0 = torch.zeros(blocks[0][0].shape), torch.zeros(blocks[0][1].shape)
    cur = SR.launch_merge(out0, lse0, *blocks[0], first=True)
    for bo, bl in blocks[1:]:
        cur = SR.launch_merge(cur["out"], cur["lse"], bo, bl)
    key = {}
    SR.check_merge(f"chain N={n} D={D}", cur, SR.ref_chain(blocks), SR.K_ELEM * (n - 1), key)
    for name, kk in key.items():
        WORST[name + ".per_merge"] = max(WORST.get(name + ".per_merge", 0.0), kk / (n - 1))


# ------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("D,G,split,kind", SR.dec_cases())
def test_decode(D, G, split, kind):
    from picotron_amd import generate as GEN
    lens = SR.dec_lens(D, split)
    q, k, v, lt = SR.make_decode(kind, G, D, lens)
    B, Hkv, S = len(lens), k.shape[1], k.shape[2]
    assert S == SR.dec_smax(D)
    eff = GEN.default_split_keys(B, Hkv, S, D) if split is None else split
    scale = 1.0 / math.sqrt(D)
    ref = SR.decode_ref(q, k, v, lt, scale, eff)
    got = SR.launch_decode(q, k, v, lt, scale, split)
    assert got["o"].dtype == BF and got["lse"].dtype == F32
    res = SR.decode_check(f"D={D} G={G} split={split} ({eff}) {kind}", got["o"], got["lse"], ref, worst=WORST)
    assert res["ok"], res


def test_decode_public_entry_matches_the_guarded_launch():
    """generate.attention_decode (its own grow-only workspace, contiguous operands) gives the bits of the guarded,
    strided launch."""
    from picotron_amd import generate as GEN
    D, G, split = 64, 4, 129
    lens = SR.dec_lens(D, split)
    q, k, v, lt = SR.make_decode("ascending", G, D, lens)
    got = SR.launch_decode(q, k, v, lt, 0.125, split)
    o, lse = GEN.attention_decode(q.to(DEV), k.to(DEV), v.to(DEV), lt.to(DEV), 0.125, split, True)
    assert torch.equal(_bits(o), _bits(got["o"])) and torch.equal(_bits(lse), _bits(got["lse"]))


# ------------------------------------------------------------------------------------------ ring forward, one process
class _Ctx:
    def save_for_backward(self, *t):
        self.saved = t


def _ring_rows(S, rank, world, zigzag):
    from picotron_amd.context_parallel import context_parallel as CP
    if zigzag:
        return CP.zigzag_positions(S, rank, world)
    n = S // world
    return torch.arange(rank * n, (rank + 1) * n)


_RING_REF = {}


def _ring_ref(kind, B, S, Hq, Hkv, D):
    key = (kind, B, S, Hq, Hkv, D)
    if key not in _RING_REF:
        q, k, v, _ = A.make_inputs(kind, B, S, S, Hq, Hkv, D, True)
        scale = D ** -0.5
        _RING_REF[key] = (q, k, v, A.reference_fwd(q, k, v, scale, True), A.emulate_fwd(q, k, v, scale, True))
    return _RING_REF[key]


@pytest.mark.parametrize("kind", ["randn", "diag"])
@pytest.mark.parametrize("Hq,Hkv,D", [(4, 4, 64), (4, 2, 64), (2, 1, 128)])
@pytest.mark.parametrize("zigzag", [False, True])
@pytest.mark.parametrize("world", [2, 4])
def test_ring_forward_one_process(monkeypatch, world, zigzag, Hq, Hkv, D, kind):
    """The forward's traffic depends on the inputs only, so the ranks run one after another: at ring step s rank r
    holds the K / V shard of rank r - s. S = 96 world: a zig-zag chunk is 48 rows, not a multiple of a tile."""
    from picotron_amd.context_parallel import context_parallel as CP
    B, S = 2, 96 * world
    q, k, v, (o_ref, l_ref), (o_emul, _) = _ring_ref(kind, B, S, Hq, Hkv, D)
    rows = [_ring_rows(S, r, world, zigzag) for r in range(world)]
    shard = [[t[:, rows[r]].contiguous().to(DEV) for t in (q, k, v)] for r in range(world)]
    monkeypatch.setenv("PICO_CP_ZIGZAG", "1" if zigzag else "0")
    state = {}

    class Stub:
        def __init__(self, msg=""):
            self.rank, self.world_size, self.step, self.calls = state["rank"], world, 0, 0

        def send_recv(self, tensor_to_send, recv_tensor=None):
            src = (self.rank - self.step - 1) % world
            held = shard[(self.rank - self.step) % world][1 + self.calls % 2]
            assert tensor_to_send.data_ptr() == held.data_ptr()  # the rank passes on what it holds
            self.calls += 1
            return shard[src][1 + (self.calls - 1) % 2]

        def commit(self):
            pass

        def wait(self):
            self.step += 1

    monkeypatch.setattr(CP, "ContextCommunicate", Stub)
    o = torch.empty(B, S, Hq, D, dtype=BF)
    lse = torch.empty(B, Hq, S)
    for r in range(world):
        state["rank"] = r
        ctx = _Ctx()
        with torch.no_grad():
            out = CP.RingAttentionFunc.forward(ctx, *shard[r], D ** -0.5, True)
        assert out.dtype == BF and out.shape == shard[r][0].shape
        o[:, rows[r]] = out.cpu()
        lse[:, :, rows[r]] = ctx.saved[4].cpu()
    res = A.tile_check("o", o, o_emul, o_ref)
    lres = A.lse_check(lse, l_ref)
    print(f"RING world={world} zigzag={zigzag} Hq={Hq} Hkv={Hkv} D={D} {kind}: O ratio {res['ratio']:.3f} at "
          f"(b {res['batch']}, h {res['head']}, tile {res['row_block']}), LSE max-abs {lres['err']:.2e}")
    WORST["ring.o_ratio"] = max(WORST.get("ring.o_ratio", 0.0), res["ratio"])
    assert res["ok"], res
    assert lres["ok"], lres


def test_report_worst():
    """Prints what the tests above measured (run the whole file): the worst K per merge output, the worst decode O
    ratio and LSE K, the worst ring tile ratio."""
    for name in sorted(WORST):
        print(f"WORST {name} {WORST[name]:.3f}")
