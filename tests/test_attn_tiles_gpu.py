"""Every attention kernel path on the GPU under the per-tile error bound and guard bands of tests/attn_ref.py.

Each case launches through ops._attn_args / the C ABI on guarded buffers (NaN around every tensor, NaN-filled outputs,
a guarded workspace), checks that the guards are bit-identical afterwards and every output element was written, and
holds every (batch, head, 32-row) tile of O / dQ / dK / dV to
    ||X_kernel - X_ref|| <= 2 ||X_emul - X_ref|| + 2^-9 ||X_ref||
against an fp64 reference and a dense emulation at the kernels' precision, both plain torch on the GPU. The backward's
o and lse come from the emulation, not from the forward kernel. Which plan path a backward case takes at 256 CUs is
asserted on the CPU by tests/test_attn_tiles_host.py::test_case_table_reaches_every_plan_path; on another device the
cases still run and must pass. At import this file only defines its tables."""
import math

import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AUTO = -1

# ---------------------------------------------------------------------------------------------------------- tables
# forward, 32-row kernel: (D, causal, Sq, Sk); every case runs GQA 1, 2 and 8 at B 2 on all three input sets
FWD_CASES = ([(D, True, S, S) for D in (64, 128) for S in (1, 31, 33, 65, 129, 257)]
             + [(D, False, Sq, Sk) for D in (64, 128) for Sq, Sk in ((96, 200), (300, 77), (33, 1))])

# forward, persistent kernel (PICO_SEL_ATTN_FWD = 1, D 64): (B, Sq, Sk, Hq, Hkv, causal)
FWDP_CASES = [
    (1, 128, 128, 2, 2, True),      # one item
    (2, 1344, 1344, 4, 4, True),    # odd block count, partial last block
    (4, 1024, 1024, 32, 32, True),  # paired items (nbh * ceil(nJ / 2) >= CUs)
    (4, 1024, 1024, 32, 8, True),   # paired items, GQA 4
    (2, 512, 512, 4, 4, False),     # non-causal
    # cross lengths, non-causal: attn_fwdp_kernel takes its K/V tile count, ring and DMA stream from Sk alone
    # (nkt = Sk / 64, item_tiles = nkt, gtot) and its items, row clamps and stores from Sq alone
    (2, 256, 512, 4, 4, False),
    (2, 512, 256, 4, 4, False),
]
# with the knob at 1 these fall back to the 32-row kernel: bit-identical to knob 0. (D, B, Sq, Sk, H, causal)
FWDP_FALLBACK = [(128, 1, 128, 128, 2, True), (64, 1, 200, 200, 2, True), (64, 1, 96, 200, 2, False)]

# dK/dV kernels: name -> (D, PICO_SEL_ATTN_KVP, PICO_SEL_KVP_WAVES)
KV_KERNELS = {
    "kvp64w4": (64, 1, 4),      # attn_bwd_kvp_kernel, 4 waves
    "kvp64w8": (64, 1, 8),      # attn_bwd_kvp_kernel, 8 waves (256-key blocks)
    "kv32d64": (64, 0, AUTO),   # 32-row attn_bwd_kv_kernel: 3 per CU causal, 2 non-causal
    "kvp128": (128, 1, AUTO),   # attn_bwd_kvp128_kernel
    "kv32d128": (128, 0, AUTO),  # 32-row attn_bwd_kv_kernel<128>
}
# shapes every dK/dV kernel runs: (causal, B, Sq, Sk, Hq, Hkv, groups, mode, input sets)
# groups "pair": the causal block groups and the same shape with PICO_SEL_ATTN_GROUPS = 0, compared bit for bit
_EVERY = [
    (True, 1, 31, 31, 1, 1, AUTO, "rope", ("randn", "bait")),      # one tile: hsplit 1, RoPE^-1 on the direct path
    (True, 2, 33, 33, 2, 2, AUTO, "bf16", ("randn", "bait")),      # hsplit 2
    (True, 2, 129, 129, 2, 2, AUTO, "rope", ("randn", "bait")),    # hsplit 4, RoPE^-1 in attn_bwd_dkv_kernel
    (True, 2, 257, 257, 4, 2, AUTO, "f32acc", ("randn", "bait", "diag")),  # hsplit 8, GQA 2
    (False, 2, 96, 200, 4, 4, AUTO, "bf16", ("randn", "bait")),    # cross lengths
    (False, 1, 300, 77, 2, 1, AUTO, "rope", ("randn", "bait")),
    (False, 2, 129, 257, 8, 1, AUTO, "f32acc", ("randn", "bait")),  # GQA 8
]
# the smallest causal shape whose dK/dV grid is cut into block groups at 256 CUs, per kernel (B, S, Hq, Hkv)
_GROUPED = {"kvp64w4": (4, 384, 64, 64), "kvp64w8": (2, 768, 64, 64), "kv32d64": (4, 512, 64, 64),
            "kvp128": (2, 384, 128, 64), "kv32d128": (2, 384, 128, 64)}
BWD_CASES = [(kern,) + shape for kern in KV_KERNELS for shape in _EVERY]
BWD_CASES += [(kern, True, B, S, S, Hq, Hkv, "pair", "bf16", ("randn", "bait"))
              for kern, (B, S, Hq, Hkv) in _GROUPED.items()]
# dQ kernel with a lightest-first front (q_front > 0) in its other two output forms, the library's own dK/dV choice
BWD_CASES += [("auto64", True, 4, 512, 512, 64, 64, AUTO, mode, ("randn",)) for mode in ("f32acc", "rope")]
BWD_CASES += [("auto128", True, 2, 384, 384, 128, 64, AUTO, mode, ("randn",)) for mode in ("f32acc", "rope")]
KV_KERNELS_ALL = dict(KV_KERNELS, auto64=(64, AUTO, AUTO), auto128=(128, AUTO, AUTO))


# ---------------------------------------------------------------------------------------------------------- helpers
def _knobs(**kw):
    from picotron_amd import _lib as L
    for name, val in kw.items():
        L.select(getattr(L, name), val)


def _reset_knobs():
    _knobs(SEL_ATTN_KVP=AUTO, SEL_KVP_WAVES=AUTO, SEL_ATTN_GROUPS=AUTO, SEL_ATTN_FWD=AUTO)


def _report(tag, results):
    for r_ in results:
        print(f"TILE {tag} {r_['output']} ratio {r_['ratio']:.3f} at (batch {r_['batch']}, head {r_['head']}, "
              f"row block {r_['row_block']}): kernel {r_['err_rel']:.2e}, emulation {r_['emul_rel']:.2e} of the tile")
    bad = [r_ for r_ in results if not r_["ok"]]
    assert not bad, (tag, bad)


def _rope_rotated(q, cos, sin):
    from picotron_amd import ops
    qc = q.contiguous()
    out = torch.empty_like(qc)
    ops._rope_launch(qc, out, cos, sin, False)
    return out


def _check_fwd(tag, q, k, v, D, causal, rope):
    """One forward launch (plain, or rope_q + o_t) under the guards, the per-tile bound and the LSE bound."""
    sc = 1.0 / math.sqrt(D)
    B, Sq, Hq, _ = q.shape
    qr = q
    tables = None
    if rope:
        tables = R.rope_tables(Sq, D, DEV)
        qr = _rope_rotated(q, *tables)
    out = R.launch_fwd(q, k, v, sc, causal, rope_q=tables, want_o_t=rope)
    if rope:
        assert torch.equal(out["q"], qr), f"{tag}: the rotated q written back differs from pico_rope"
        assert torch.equal(out["o_t"], out["o"].permute(2, 3, 0, 1).reshape(Hq * D, B * Sq)), f"{tag}: o_t != O^T"
    O, L = R.reference_fwd(qr, k, v, sc, causal)
    oe, _ = R.emulate_fwd(qr, k, v, sc, causal)
    lse = R.lse_check(out["lse"], L)
    assert lse["ok"], (tag, lse)
    assert R.rel_l2(out["o"], O) < R.FWD_TOL
    _report(tag, [R.tile_check("O", out["o"], oe, O)])
    return out


# ---------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("D,causal,Sq,Sk", FWD_CASES)
def test_fwd_32row(D, causal, Sq, Sk):
    try:
        _knobs(SEL_ATTN_FWD=0)
        for gqa, Hkv in ((1, 2), (2, 2), (8, 1)):
            for kind in ("randn", "diag", "bait"):
                q, k, v, _ = R.make_inputs(kind, 2, Sq, Sk, Hkv * gqa, Hkv, D, causal, DEV)
                tag = f"fwd32 D{D} {'causal' if causal else 'full'} {Sq}x{Sk} gqa{gqa} {kind}"
                _check_fwd(tag, q, k, v, D, causal, rope=False)
                if gqa == 2 and kind == "randn":
                    _check_fwd(tag + " rope_q+o_t", q, k, v, D, causal, rope=True)
    finally:
        _reset_knobs()


@pytest.mark.parametrize("B,Sq,Sk,Hq,Hkv,causal", FWDP_CASES)
def test_fwd_persistent(B, Sq, Sk, Hq, Hkv, causal):
    try:
        _knobs(SEL_ATTN_FWD=1)
        for kind, rope in (("randn", False), ("bait", False), ("randn", True)):
            q, k, v, _ = R.make_inputs(kind, B, Sq, Sk, Hq, Hkv, 64, causal, DEV)
            tag = (f"fwdp {'causal' if causal else 'full'} B{B} {Sq}x{Sk} H{Hq}/{Hkv} {kind}"
                   f"{' rope_q+o_t' if rope else ''}")
            out = _check_fwd(tag, q, k, v, 64, causal, rope)
            if kind == "randn" and not rope:  # the 32-row kernel on the same inputs
                _knobs(SEL_ATTN_FWD=0)
                o32 = R.launch_fwd(q, k, v, 0.125, causal)["o"]
                _knobs(SEL_ATTN_FWD=1)
                print(f"FWDP {tag}: {int((o32 != out['o']).sum())} of {o32.numel()} elements differ from the "
                      f"32-row kernel's")
    finally:
        _reset_knobs()


@pytest.mark.parametrize("D,B,Sq,Sk,H,causal", FWDP_FALLBACK)
def test_fwd_persistent_falls_back(D, B, Sq, Sk, H, causal):
    """D = 128 and lengths that are no multiple of 64 are the 32-row kernel's with the knob at 1: bit-identical."""
    try:
        q, k, v, _ = R.make_inputs("randn", B, Sq, Sk, H, H, D, causal, DEV)
        outs = []
        for sel in (0, 1):
            _knobs(SEL_ATTN_FWD=sel)
            outs.append(R.launch_fwd(q, k, v, 1.0 / math.sqrt(D), causal))
        assert torch.equal(outs[0]["o"], outs[1]["o"]) and torch.equal(outs[0]["lse"], outs[1]["lse"])
    finally:
        _reset_knobs()


def test_fwd_causal_cross_lengths_are_refused():
    """Causal Sq != Sk never reaches either forward kernel: the ABI refuses it, whatever the knob says."""
    try:
        q, _, _, _ = R.make_inputs("randn", 1, 128, 128, 2, 2, 64, True, DEV)
        _, k, v, _ = R.make_inputs("randn", 1, 192, 192, 2, 2, 64, True, DEV)
        for sel in (0, 1):
            _knobs(SEL_ATTN_FWD=sel)
            with pytest.raises(RuntimeError, match="causal"):
                R.launch_fwd(q, k, v, 0.125, True)
    finally:
        _reset_knobs()


# ---------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("kern,causal,B,Sq,Sk,Hq,Hkv,groups,mode,kinds", BWD_CASES)
def test_bwd(kern, causal, B, Sq, Sk, Hq, Hkv, groups, mode, kinds):
    D, kvp, waves = KV_KERNELS_ALL[kern]
    sc = 1.0 / math.sqrt(D)
    try:
        for kind in kinds:
            q, k, v, do = R.make_inputs(kind, B, Sq, Sk, Hq, Hkv, D, causal, DEV)
            o, lse = R.emulate_fwd(q, k, v, sc, causal)  # the backward's inputs: independent of the forward kernel
            rope = R.rope_tables(max(Sq, Sk), D, DEV) if mode == "rope" else None
            ref = R.reference_bwd(do, q, k, v, o, lse, sc, causal, rope=rope)
            emu = R.emulate_bwd(do, q, k, v, o, lse, sc, causal, rope=rope, dq_f32=mode == "f32acc")
            got = {}
            for grp in ((AUTO, 0) if groups == "pair" else (groups,)):
                _knobs(SEL_ATTN_KVP=kvp, SEL_KVP_WAVES=waves, SEL_ATTN_GROUPS=grp)
                got[grp] = R.launch_bwd(do, q, k, v, o, lse, sc, causal, mode=mode, rope=rope)
                tag = (f"bwd {kern} {'causal' if causal else 'full'} B{B} {Sq}x{Sk} H{Hq}/{Hkv} {mode} "
                       f"groups{grp} {kind}")
                res = []
                for n, x, e, r_ in zip(("dQ", "dK", "dV"), got[grp], emu, ref):
                    assert R.rel_l2(x, r_) < R.BWD_TOL, (tag, n)
                    res.append(R.tile_check(n, x, e, r_, bf16_term=not (n == "dQ" and mode == "f32acc")))
                _report(tag, res)
            if groups == "pair":  # the same work in another order per workgroup, every output with one owner
                for n, a, b in zip(("dQ", "dK", "dV"), got[AUTO], got[0]):
                    assert torch.equal(a, b), f"{kern} {kind}: {n} differs between the grouped and the plain grid"
    finally:
        _reset_knobs()
