"""Gradient-norm / clip entry points without a GPU: argument checks of the C ABI (status 1000 + message), the
workspace size, the Python interface's argument errors, and the rule that picks which parameters a tensor-parallel
rank adds to its local sum of squares (no compute calls: CPU only)."""
import ctypes
import os

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from picotron_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from picotron_amd.build import build
        build()
    return _lib.load()


def test_entry_points_reject_bad_arguments(lib):
    p = ctypes.c_void_p(64)
    # pico_grad_sqnorm: null tables / workspace / result, chunk count out of range
    assert lib.pico_grad_sqnorm(None, None, None, 4, p, p, None) == 1000
    assert b"null table" in lib.pico_last_error()
    assert lib.pico_grad_sqnorm(p, p, p, 4, None, p, None) == 1000
    assert b"workspace" in lib.pico_last_error()
    assert lib.pico_grad_sqnorm(p, p, p, 4, p, None, None) == 1000
    assert b"sumsq" in lib.pico_last_error()
    for n in (-1, 1 << 31):
        assert lib.pico_grad_sqnorm(p, p, p, n, p, p, None) == 1000
        assert b"chunk count" in lib.pico_last_error()
    # pico_grad_clip_coef: max_norm negative or NaN, null pointers
    for bad in (-1.0, float("nan")):
        assert lib.pico_grad_clip_coef(p, bad, p, None) == 1000
        assert b"max_norm" in lib.pico_last_error()
    assert lib.pico_grad_clip_coef(None, 1.0, p, None) == 1000
    assert lib.pico_grad_clip_coef(p, 1.0, None, None) == 1000
    assert b"null" in lib.pico_last_error()
    # pico_grad_scale
    assert lib.pico_grad_scale(None, p, p, 4, p, None) == 1000
    assert b"null table" in lib.pico_last_error()
    assert lib.pico_grad_scale(p, p, p, 4, None, None) == 1000
    assert b"norm_coef" in lib.pico_last_error()
    assert lib.pico_grad_scale(p, p, p, -2, p, None) == 1000
    assert b"chunk count" in lib.pico_last_error()
    # pico_adamw_bf16_clip: pico_adamw_bf16's checks plus the norm_coef pointer
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.01)
    assert lib.pico_adamw_bf16_clip(None, p, p, 4, *hp, 1, p, None) == 1000
    assert b"null table" in lib.pico_last_error()
    assert lib.pico_adamw_bf16_clip(p, p, p, 4, *hp, 1, None, None) == 1000
    assert b"norm_coef" in lib.pico_last_error()
    assert lib.pico_adamw_bf16_clip(p, p, p, 1 << 31, *hp, 1, p, None) == 1000
    assert b"chunk count" in lib.pico_last_error()
    assert lib.pico_adamw_bf16_clip(p, p, p, 4, *hp, 0, p, None) == 1000
    assert b"step" in lib.pico_last_error()
    assert lib.pico_adamw_bf16_clip(p, p, p, 4, 1e-3, 1.0, 0.999, 1e-8, 0.01, 1, p, None) == 1000
    assert b"hyper-parameters" in lib.pico_last_error()


def test_workspace_bytes(lib):
    # one fp32 partial per chunk
    assert lib.pico_grad_sqnorm_workspace_bytes(1) == 4
    assert lib.pico_grad_sqnorm_workspace_bytes(26113) == 26113 * 4
    assert lib.pico_grad_sqnorm_workspace_bytes(0) == 0


def test_kernel_ids():
    from picotron_amd import _lib
    assert (_lib.K_GRAD_SQNORM, _lib.K_GRAD_SCALE) == (24, 25)
    assert _lib.KERNEL_NAMES[24] == "grad_sqnorm" and _lib.KERNEL_NAMES[25] == "grad_scale"


def test_python_argument_errors():
    from picotron_amd.optim import AdamW, clip_grad_norm_
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))
    for bad in (-1, -1.0, float("nan")):
        with pytest.raises(ValueError):
            AdamW([p], max_grad_norm=bad)
    opt = AdamW([p], max_grad_norm=0.5)
    assert opt.max_grad_norm == 0.5 and opt.grad_norm is None
    assert AdamW([p]).max_grad_norm is None
    p.grad = torch.zeros(8, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        clip_grad_norm_([p], 1.0, norm_type=1)
    with pytest.raises(NotImplementedError):
        clip_grad_norm_([p], 1.0, norm_type=float("inf"))
    with pytest.raises(ValueError):
        clip_grad_norm_([p], -1.0)
    with pytest.raises(TypeError):  # a CPU gradient: no fallback
        clip_grad_norm_([p], 1.0)


def test_select_norm_params():
    """Sharded (tagged) parameters count on every tensor-parallel rank, replicated ones on tp rank 0 only."""
    from picotron_amd.optim import select_norm_params
    params = [torch.nn.Parameter(torch.zeros(2)) for _ in range(5)]
    for i in (0, 2, 3):
        params[i]._pico_tp_sharded = True
    assert select_norm_params(params, 0, 2) == [True] * 5
    assert select_norm_params(params, 1, 2) == [True, False, True, True, False]
    assert select_norm_params(params, 3, 4) == [True, False, True, True, False]
    for rank in range(2):
        assert select_norm_params(params, rank, 1) == [True] * 5
    assert select_norm_params([], 1, 2) == []


def test_tensor_parallel_layers_tag_their_shards():
    """ColumnParallelLinear weight + bias, RowParallelLinear weight and VocabParallelEmbedding weight are tagged;
    the row-parallel bias is replicated and is not."""
    from types import SimpleNamespace
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.tensor_parallel import tensor_parallel as TP
    old = pgm.process_group_manager
    pgm.process_group_manager = SimpleNamespace(tp_world_size=2, tp_rank=1)
    try:
        col = TP.ColumnParallelLinear(8, 4, bias=True)
        row = TP.RowParallelLinear(8, 4, bias=True)
        emb = TP.VocabParallelEmbedding(16, 4)
    finally:
        pgm.process_group_manager = old
    tagged = [getattr(p, "_pico_tp_sharded", False) for p in (col.weight, col.bias, row.weight, row.bias, emb.weight)]
    assert tagged == [True, True, True, False, True]
