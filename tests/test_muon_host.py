"""Muon without a GPU: the C ABI's argument checks (status 1000 + message), the constructor against torch.optim.Muon
(param_groups keys and defaults, refusals, state_dict interchange), muon_param_split on a meta-device Llama, and the
host half of the tables (chunk_start, shape buckets, _adjust_lr ratios). No kernel runs: CPU only."""
import ctypes
import os

import pytest
import torch

BF = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    from picotron_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from picotron_amd.build import build
        build()
    return _lib.load()


def test_symbols_exported_with_signatures(lib):
    from picotron_amd import _lib
    for name in ("pico_muon_momentum", "pico_muon_normalize", "pico_muon_update"):
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes == _lib._SIGNATURES[name][1]
    assert lib.pico_abi_version() == 2  # added functions only


def test_entry_points_reject_bad_arguments(lib):
    p = ctypes.c_void_p(64)
    # pico_muon_momentum
    assert lib.pico_muon_momentum(None, p, p, 4, 0.95, 1, p, None) == 1000
    assert b"null table" in lib.pico_last_error()
    assert lib.pico_muon_momentum(p, p, p, 4, 0.95, 1, None, None) == 1000
    assert b"partials" in lib.pico_last_error()
    for bad in (-0.1, float("nan")):
        assert lib.pico_muon_momentum(p, p, p, 4, bad, 1, p, None) == 1000
        assert b"momentum" in lib.pico_last_error()
    for n in (-1, 1 << 31):
        assert lib.pico_muon_momentum(p, p, p, n, 0.95, 1, p, None) == 1000
        assert b"chunk count" in lib.pico_last_error()
    assert lib.pico_muon_momentum(None, None, None, 0, 0.95, 1, None, None) == 0
    # pico_muon_normalize
    assert lib.pico_muon_normalize(p, None, p, 4, p, 2, p, 1e-7, p, None) == 1000
    assert b"null table" in lib.pico_last_error()
    assert lib.pico_muon_normalize(p, p, p, 4, None, 2, p, 1e-7, p, None) == 1000
    assert b"null table" in lib.pico_last_error()
    assert lib.pico_muon_normalize(p, p, p, 4, p, 2, p, 1e-7, None, None) == 1000
    assert b"norms" in lib.pico_last_error()
    assert lib.pico_muon_normalize(p, p, p, 4, p, 2, p, -1e-7, p, None) == 1000
    assert b"eps" in lib.pico_last_error()
    assert lib.pico_muon_normalize(p, p, p, 4, p, 0, p, 1e-7, p, None) == 1000
    assert b"tensor count" in lib.pico_last_error()
    for n in (-1, 1 << 31):
        assert lib.pico_muon_normalize(p, p, p, n, p, 2, p, 1e-7, p, None) == 1000
        assert b"chunk count" in lib.pico_last_error()
    assert lib.pico_muon_normalize(None, None, None, 0, None, 0, None, 1e-7, None, None) == 0
    # pico_muon_update
    assert lib.pico_muon_update(p, p, None, p, 4, 0.02, 0.1, p, None) == 1000
    assert b"null table" in lib.pico_last_error()
    assert lib.pico_muon_update(p, None, p, p, 4, 0.02, 0.1, p, None) == 1000
    assert b"out_ptrs" in lib.pico_last_error()
    assert lib.pico_muon_update(p, p, p, p, 4, 0.02, 0.1, None, None) == 1000
    assert b"ratios" in lib.pico_last_error()
    for lr, wd in ((-0.02, 0.1), (0.02, -0.1), (float("nan"), 0.1)):
        assert lib.pico_muon_update(p, p, p, p, 4, lr, wd, p, None) == 1000
        assert b"lr and weight_decay" in lib.pico_last_error()
    for n in (-1, 1 << 31):
        assert lib.pico_muon_update(p, p, p, p, n, 0.02, 0.1, p, None) == 1000
        assert b"chunk count" in lib.pico_last_error()
    assert lib.pico_muon_update(None, None, None, None, 0, 0.02, 0.1, None, None) == 0


def test_constructor_matches_torch():
    from picotron_amd.optim import Muon
    p = torch.nn.Parameter(torch.randn(8, 12).to(BF))
    ours, ref = Muon([p]), torch.optim.Muon([p])
    assert list(ours.param_groups[0]) == list(ref.param_groups[0])
    for k, v in ref.param_groups[0].items():
        if k != "params":
            assert ours.param_groups[0][k] == v, k
    assert Muon.reads_deferred_grads is True
    # torch's positional order
    o = Muon([p], 0.02, 0.0, 0.9, False, (1.0, 2.0, 3.0), 1e-6, 3, "match_rms_adamw")
    g = o.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["momentum"], g["nesterov"], g["ns_coefficients"], g["eps"], g["ns_steps"],
            g["adjust_lr_fn"]) == (0.02, 0.0, 0.9, False, (1.0, 2.0, 3.0), 1e-6, 3, "match_rms_adamw")
    import inspect
    assert list(inspect.signature(Muon.__init__).parameters) == list(inspect.signature(
        torch.optim.Muon.__init__).parameters)


def test_constructor_refusals():
    from picotron_amd.optim import Muon
    p = torch.nn.Parameter(torch.randn(8, 12).to(BF))
    for kw in ({"lr": -1e-3}, {"momentum": -0.1}, {"weight_decay": -0.1}, {"adjust_lr_fn": "spectral"}):
        with pytest.raises(ValueError):
            Muon([p], **kw)
    for shape in ((8,), (2, 3, 4)):
        with pytest.raises(ValueError, match="2D"):
            Muon([torch.nn.Parameter(torch.randn(shape).to(BF))])
    with pytest.raises(TypeError, match="float lr"):
        Muon([p], lr=torch.tensor(1e-3))
    q = torch.nn.Parameter(torch.randn(8, 12).to(BF))
    q._pico_tp_sharded = True
    with pytest.raises(NotImplementedError, match="shard"):
        Muon([p, q])


def test_step_refuses_cpu_tensors_before_touching_state():
    from picotron_amd.optim import Muon
    p = torch.nn.Parameter(torch.randn(8, 12).to(BF))
    p.grad = torch.randn(8, 12).to(BF)
    o = Muon([p])
    with pytest.raises(TypeError, match="bf16 HIP tensors"):
        o.step()
    assert len(o.state) == 0


def test_state_dict_interchanges_with_torch():
    from picotron_amd.optim import Muon
    torch.manual_seed(3)
    base = [torch.randn(8, 12).to(BF), torch.randn(16, 4).to(BF)]
    ref_p = [torch.nn.Parameter(t.clone()) for t in base]
    for q in ref_p:
        q.grad = torch.randn(q.shape).to(BF)
    ref = torch.optim.Muon(ref_p, lr=0.02)
    ref.step()  # one CPU step of torch's
    sd = ref.state_dict()
    ours = Muon([torch.nn.Parameter(t.clone()) for t in base], lr=0.5)
    ours.load_state_dict(sd)
    assert ours.param_groups[0]["lr"] == 0.02
    for q, r in zip(ours.param_groups[0]["params"], ref_p):
        assert set(ours.state[q]) == {"momentum_buffer"}
        assert ours.state[q]["momentum_buffer"].dtype == BF
        assert torch.equal(ours.state[q]["momentum_buffer"], ref.state[r]["momentum_buffer"])
    back = torch.optim.Muon([torch.nn.Parameter(t.clone()) for t in base])
    back.load_state_dict(ours.state_dict())
    for q, r in zip(back.param_groups[0]["params"], ref_p):
        assert torch.equal(back.state[q]["momentum_buffer"], ref.state[r]["momentum_buffer"])
    assert {k: v for k, v in back.param_groups[0].items() if k != "params"} == \
        {k: v for k, v in ref.param_groups[0].items() if k != "params"}


def test_muon_param_split():
    from picotron_amd import model as M
    from picotron_amd.optim import muon_param_split
    cfg = M.LlamaConfig(hidden_size=64, intermediate_size=128, num_attention_heads=2, num_key_value_heads=2,
                        num_hidden_layers=2, vocab_size=96, max_position_embeddings=16)
    with torch.device("meta"):
        model = M.Llama(cfg)
    muon, other = muon_param_split(model)
    named = list(model.named_parameters())
    name_of = {id(p): n for n, p in named}
    assert len(muon) + len(other) == len(named)
    assert {id(p) for p in muon}.isdisjoint({id(p) for p in other})
    assert {id(p) for p in muon} | {id(p) for p in other} == {id(p) for _, p in named}
    order = {id(p): i for i, (_, p) in enumerate(named)}
    for lst in (muon, other):
        assert [order[id(p)] for p in lst] == sorted(order[id(p)] for p in lst)
    assert len(muon) == 2 * 7  # q, k, v, out, up, gate, down per layer
    for p in muon:
        assert p.ndim == 2 and name_of[id(p)].startswith("decoder_layers.")
        assert "norm" not in name_of[id(p)]
    other_names = {name_of[id(p)] for p in other}
    assert {"embedding.weight", "final_proj.weight", "final_norm.weight"} <= other_names
    assert all(p.ndim == 1 for p in other if name_of[id(p)].startswith("decoder_layers."))  # the layers' norms


def test_table_building(lib):
    from torch.optim._muon import _adjust_lr
    from picotron_amd.optim import _muon_layout, _muon_work
    assert lib.pico_adamw_chunk_elems() == 65536
    shapes = [(8, 8), (40, 72), (40, 72), (2, 32772)]
    lay = _muon_layout(shapes)
    assert lay["chunk_start"] == [0, 1, 2, 3, 5]
    assert lay["buckets"] == {(8, 8): [0], (40, 72): [1, 2], (2, 32772): [3]}
    assert lay["slot"] == [((8, 8), 0), ((40, 72), 0), ((40, 72), 1), ((2, 32772), 0)]
    bufs, slices = _muon_work(lay, "cpu")
    assert bufs[(40, 72)].shape == (2, 40, 72) and bufs[(40, 72)].is_contiguous() and bufs[(40, 72)].dtype == BF
    assert slices[1].data_ptr() == bufs[(40, 72)].data_ptr()
    assert slices[2].data_ptr() == slices[1].data_ptr() + 2 * 40 * 72  # contiguous, in list order
    assert [tuple(s.shape) for s in slices] == shapes and all(s.is_contiguous() for s in slices)
    assert sum(b.numel() for b in bufs.values()) == sum(a * b for a, b in shapes)  # 2 B per Muon parameter
    # ratios: torch's _adjust_lr for both functions (and None), a tall shape included
    shapes.append((1000, 3))
    for fn in (None, "original", "match_rms_adamw"):
        lay = _muon_layout(shapes, fn)
        for s, r in zip(shapes, lay["ratios"]):
            assert r == _adjust_lr(1.0, fn, torch.Size(s)), (fn, s)
            assert 0.02 * r == _adjust_lr(0.02, fn, torch.Size(s))
    assert _muon_layout([(1000, 3)])["ratios"][0] == (1000 / 3) ** 0.5


def test_newton_schulz_plan_matches_torch_on_cpu():
    """The GEMM schedule (the tall matrices iterated without a transposed copy, the shared ping-pong and Gram
    buffers, the result landing in the matrix's slice of its shape's work buffer) against torch's own _zeropower_via_newtonschulz on the CPU, fed
    the same normalised bf16 input. Both run the same bf16 sums, at most in another order; the bound is the low end
    of torch's own bf16 error against fp64 on these iterations (1e-2); a wrong transpose, coefficient or slice
    gives O(1)."""
    from torch.optim._muon import _zeropower_via_newtonschulz
    from picotron_amd.optim import _muon_layout, _muon_ns_plan, _muon_work, _newton_schulz
    torch.manual_seed(0)
    shapes = [(8, 8), (40, 72), (40, 72), (128, 64), (128, 64), (100, 3)]
    co = (3.4445, -4.7750, 2.0315)
    us = [torch.randn(s).to(BF) for s in shapes]
    for steps in (5, 2, 1, 0):
        lay = _muon_layout(shapes)
        bufs, slices = _muon_work(lay, "cpu")
        flat, plan = _muon_ns_plan(lay, slices, "cpu")
        assert [f.numel() for f in flat] == [128 * 64, 128 * 64, 64 * 64, 64 * 64]  # the largest matrix's
        for u, w in zip(us, slices):
            w.copy_(u / u.norm().clamp(min=1e-7))
        _newton_schulz(plan, co, steps)
        for u, w in zip(us, slices):
            ref = _zeropower_via_newtonschulz(u.clone(), co, steps, 1e-7).float()
            assert float((w.float() - ref).norm() / ref.norm()) <= 1e-2, (steps, tuple(u.shape))
