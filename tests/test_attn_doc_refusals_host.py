"""What the document-masked attention refuses, and the plan its workspace follows (no compute calls: CPU only)."""
import ctypes

import pytest
import torch

from picotron_amd import _lib, ops


def _args(**kw):
    a = _lib.AttnArgs()
    a.q = a.k = a.v = ctypes.c_void_p(64)
    a.batch, a.seqlen_q, a.seqlen_k, a.heads_q, a.heads_kv, a.head_dim, a.causal = 1, 256, 256, 2, 2, 64, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,bounds,msg", [({}, None, b"null doc_bounds"), ({"causal": 0}, 64, b"causal"),
                                            ({"causal": 0, "seqlen_k": 128}, 64, b"causal"),
                                            ({"head_dim": 96}, 64, b"head_dim"), ({"heads_kv": 3}, 64, b"multiple")])
def test_entry_points_refuse(kw, bounds, msg):
    lib = _lib.load()
    for fn in (lib.pico_attn_doc_fwd, lib.pico_attn_doc_bwd):
        assert fn(ctypes.byref(_args(**kw)), ctypes.c_void_p(bounds) if bounds else None, None) == 1000
        assert msg in lib.pico_last_error() and b"pico_attn_doc_" in lib.pico_last_error()


def test_workspace_follows_the_doc_plan():
    lib, a = _lib.load(), _args(batch=4, seqlen_q=2048, seqlen_k=2048, heads_q=32, heads_kv=8)
    lsd, part = 2 * 4 * 32 * 2048 * 4, 2 * 2 * 4 * 2048 * 8 * 64 * 4
    old = _lib.select(_lib.SEL_ATTN_KVP, 1)  # ignored: the 32-row kernel's 2-way split (sizes of tests/test_abi.py)
    try:
        assert lib.pico_attn_doc_bwd_workspace_bytes(ctypes.byref(a)) == lsd + part
        assert lib.pico_attn_bwd_workspace_bytes(ctypes.byref(a)) == lsd
    finally:
        _lib.select(_lib.SEL_ATTN_KVP, old)


def test_python_refusals(monkeypatch):
    from picotron_amd.model import Llama, LlamaConfig
    q, good = torch.zeros(2, 64, 2, 64, dtype=torch.bfloat16), torch.zeros(2, 2, 64, dtype=torch.int32)
    for bad in (good.long(), good[:, :1], good.transpose(1, 2).contiguous().transpose(1, 2), good.to("meta"), None):
        with pytest.raises(ValueError, match="doc_bounds"):
            ops.flash_attn_doc_func(q, q, q, bad)
    with pytest.raises(ValueError, match="Sq == Sk"):
        ops.flash_attn_doc_func(q, q[:, :32], q[:, :32], good)
    with pytest.raises(RuntimeError, match="HIP"):  # HIP bf16 only, like flash_attn_func
        ops.flash_attn_doc_func(q, q, q, good)
    monkeypatch.setenv("DEVICE", "cpu")
    with torch.device("meta"):
        model = Llama(LlamaConfig(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_key_value_heads=2,
                                  num_hidden_layers=1, vocab_size=64, max_position_embeddings=64))
    monkeypatch.setenv("CONTEXT_PARALLEL", "1")
    with pytest.raises(NotImplementedError, match="context parallelism"):
        model(torch.zeros(2, 64, dtype=torch.long), doc_start=good[0])
