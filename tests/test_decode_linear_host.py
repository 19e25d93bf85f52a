"""ops.decode_linear / pico_decode_linear without a device: the plain-torch restatement against the fp64 reference
and bound of tests/decode_linear_ref.py, the refusals, and the workspace size against the split rule."""
import ctypes

import pytest
import torch

import decode_linear_ref as D

BF = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    from picotron_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("form", ["bf16", "f32", "norm", "norm_res", "swiglu", "norm_res_swiglu"])
@pytest.mark.parametrize("M,N,K", [(1, 32, 32), (3, 176, 160), (16, 272, 1024)])
def test_restatement_matches_fp64(form, M, N, K):
    from picotron_amd import ops
    x, w, nw, res = D.inputs(M, N, K)
    kw = dict(norm_weight=nw, eps=1e-5, residual=res if "res" in form else None) if "norm" in form else {}
    out = ops.decode_linear(x, w, out_dtype=torch.float32 if form == "f32" else None, **kw)
    y, ro = out if "norm" in form else (out, None)
    if form == "norm":
        assert ro is x
    D.check(f"host {form} {M}x{N}x{K}", {"y": y, "residual_out": ro}, D.reference(x, w, **kw))
    if "swiglu" in form:  # the epilogue on the projection's own bf16 output, against fp64
        act = ops.decode_linear(x, w, swiglu=True, **kw)
        act = act[0] if "norm" in form else act
        ref, cond = D.swiglu_of(y)
        D.R.report(f"host {form} act", [D.R.elem_check("act", act, ref, cond, BF)])


def test_ops_refusals():
    from picotron_amd import ops
    x, w, nw, res = D.inputs(4, 32, 64)
    with pytest.raises(ValueError, match="1..16"):
        ops.decode_linear(torch.zeros(17, 64, dtype=BF), w)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.decode_linear(x[:, :48], w[:, :48])
    with pytest.raises(ValueError, match="row stride"):
        ops.decode_linear(torch.zeros(4, 68, dtype=BF)[:, :64], w)
    with pytest.raises(ValueError, match="norm prologue"):
        ops.decode_linear(x, w, residual=res)
    with pytest.raises(ValueError, match="out_dtype"):
        ops.decode_linear(x, w, swiglu=True, out_dtype=torch.float32)


def test_abi_refusals(lib):
    from picotron_amd import _lib
    assert lib.pico_decode_linear_args_size() == ctypes.sizeof(_lib.DecodeLinearArgs)

    def call(**kw):
        a = _lib.DecodeLinearArgs()
        a.x, a.weight, a.y = 0x1000, 0x100000, 0x200000
        a.ldx = a.ldw = a.k = 64
        a.m, a.n, a.ldy = 4, 32, 32
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.pico_decode_linear(ctypes.byref(a), None)
        return rc, lib.pico_last_error()

    for kw, msg in ((dict(x=None), b"null"), (dict(m=17), b"m=17"), (dict(k=48, ldx=48, ldw=48), b"multiple of 32"),
                    (dict(n=36), b"multiple of 8"), (dict(epilogue=2, n=40, ldy=24), b"multiple of 16"),
                    (dict(ldx=68), b"strides"), (dict(x=0x1008), b"16-byte"), (dict(residual=0x3000), b"norm"),
                    (dict(k=4096, ldx=4096, ldw=4096, split_k=1), b"LDS"),
                    (dict(norm_weight=0x4000, residual_out=0x1040, ldro=64), b"alias"),
                    (dict(norm_weight=0x4000, residual=0x3000, ldr=64, residual_out=0x3000 + 2 * 200, ldro=64),
                     b"alias")):
        rc, err = call(**kw)
        assert rc == 1000 and msg in err, (kw, rc, err)


@pytest.mark.parametrize("M,N,K,epi", [(8, 2048, 8192, 0), (16, 16384, 2048, 2)])
def test_workspace_follows_the_split_rule(lib, M, N, K, epi):
    """The down projection splits (64 column blocks for the CUs of the device, or 256 without one), gate|up does
    not; an explicit split sizes the partials for its slices."""
    sk = lib.pico_decode_linear_split_k(N, K, epi)
    assert sk >= -(-K // 2048) and (sk > 1) == (epi == 0)
    assert lib.pico_decode_linear_workspace_bytes(M, N, K, epi, 0) == (sk * M * N * 4 if sk > 1 else 0)
    assert lib.pico_decode_linear_workspace_bytes(M, N, K, epi, 8) == 8 * M * N * 4
    assert lib.pico_decode_linear_workspace_bytes(M, N, 8192, epi, 3) == -1  # slices of 2752 columns do not fit
