"""Vocab-parallel cross-entropy without a GPU: the C ABI's argument checks (status 1000 + message, no device),
the plain-torch path of picotron_amd.tensor_parallel.vocab_parallel_loss over gloo (world 2 and 4) against
F.cross_entropy on the whole logits, and the apply_tensor_parallel(vocab_parallel_loss=True) switch on a small
CPU model: local logits, both loss functions and every gradient against the unsharded model."""
import ctypes
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from picotron_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from picotron_amd.build import build
        build()
    return _lib.load()


def test_symbols_exported_with_signatures(lib):
    from picotron_amd import _lib
    for name in ("pico_ce_vp_partial", "pico_ce_vp_combine", "pico_ce_vp_grad"):
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes == _lib._SIGNATURES[name][1]
    assert lib.pico_abi_version() == 2  # added functions only


def test_entry_points_reject_bad_arguments(lib):
    p = ctypes.c_void_p(64)
    R, VL, V = 4, 16, 64

    def partial(logits=p, ld=V, target=p, part=p, rows=R, vl=VL, start=16, total=V):
        return lib.pico_ce_vp_partial(logits, ld, target, part, rows, vl, start, total, -100, None)

    def grad(logits=p, ld=V, target=p, lse=p, gs=p, dl=p, ldd=V, rows=R, vl=VL, start=16, total=V):
        return lib.pico_ce_vp_grad(logits, ld, target, lse, gs, dl, ldd, rows, vl, start, total, -100, None)

    for fn, ptrs in ((partial, ("logits", "target", "part")), (grad, ("logits", "target", "lse", "gs", "dl"))):
        for name in ptrs:
            assert fn(**{name: None}) == 1000
            assert b"null pointer" in lib.pico_last_error()
        assert fn(vl=12) == 1000
        assert b"vocab_local" in lib.pico_last_error()
        assert fn(start=4) == 1000
        assert b"vocab_start" in lib.pico_last_error()
        assert fn(start=56) == 1000  # 56 + 16 > 64
        assert b"exceeds" in lib.pico_last_error()
        assert fn(ld=V + 4) == 1000 and fn(ld=8) == 1000
        assert b"row stride" in lib.pico_last_error()
        assert fn(logits=ctypes.c_void_p(72)) == 1000
        assert b"16-byte" in lib.pico_last_error()
        assert fn(rows=-1) == 1000
        assert fn(**{k: None for k in ptrs}, rows=0) == 0
    assert grad(ldd=8) == 1000
    assert b"dlogits row stride" in lib.pico_last_error()
    assert grad(ldd=32) == 1000  # logits == dlogits with another stride
    assert b"in place" in lib.pico_last_error()

    def combine(parts=p, tp=2, target=p, rows=R, total=V, lse=p, loss=p):
        return lib.pico_ce_vp_combine(parts, tp, target, rows, total, -100, lse, loss, None)

    for name in ("parts", "target", "lse", "loss"):
        assert combine(**{name: None}) == 1000
        assert b"null pointer" in lib.pico_last_error()
    assert combine(tp=0) == 1000
    assert b"tp size" in lib.pico_last_error()
    assert combine(total=0) == 1000
    assert combine(rows=-1) == 1000
    assert combine(parts=None, target=None, lse=None, loss=None, rows=0) == 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.pop("PICO_UNFUSED", None)
    import torch.distributed as dist
    import torch.nn as nn
    import torch.nn.functional as F
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from picotron_amd import process_group_manager as pgm
    from picotron_amd import train
    from picotron_amd.tensor_parallel import tensor_parallel as TP
    from picotron_amd.tensor_parallel import vocab_parallel_loss as VPL
    pgm.setup_process_group_manager(tp_size=world, cp_size=1, pp_size=1, dp_size=1)
    bad = {}

    def everywhere_equal(name, loss):
        got = [torch.empty_like(loss) for _ in range(world)]
        dist.all_gather(got, loss.detach())
        if not all(torch.equal(g, got[0]) for g in got):
            bad[name + " differs between ranks"] = [float(g) for g in got]

    # ---- the torch path against F.cross_entropy on the whole logits ----
    N, V = 37, 64
    vl = V // world
    g = torch.Generator().manual_seed(5)
    full = (torch.randn(N, V, generator=g) * 3).requires_grad_(True)
    t = torch.randint(0, V, (N,), generator=g)
    t[::7] = -100
    for r in range(world):  # the first and the last index of every shard (these rows override the ignored ones)
        t[1 + 2 * r], t[2 + 2 * r] = r * vl, (r + 1) * vl - 1
    assert int((t == -100).sum()) >= 3
    ref = F.cross_entropy(full, t, ignore_index=-100)
    ref.backward()
    local = full.detach()[:, rank * vl:(rank + 1) * vl].clone().requires_grad_(True)
    loss = VPL.vocab_parallel_cross_entropy(local, t)
    loss.backward()
    try:
        torch.testing.assert_close(loss.detach(), ref.detach(), rtol=1e-5, atol=0)
        torch.testing.assert_close(local.grad, full.grad[:, rank * vl:(rank + 1) * vl], rtol=1e-5, atol=1e-8)
        assert bool((local.grad[t == -100] == 0).all())
    except AssertionError as e:
        bad["torch path"] = str(e)
    everywhere_equal("loss", loss)

    # ---- the fused torch form: x W^T sharded by rows of W, non-unit upstream ----
    H = 16
    xf = torch.randn(N, H, generator=g).requires_grad_(True)
    wf = (torch.randn(V, H, generator=g) * 0.5).requires_grad_(True)
    (F.cross_entropy(xf @ wf.t(), t, ignore_index=-100) * 0.25).backward()
    xl = xf.detach().clone().requires_grad_(True)
    wl = wf.detach()[rank * vl:(rank + 1) * vl].clone().requires_grad_(True)
    lh = VPL.vocab_parallel_lm_head_cross_entropy(xl, wl, t)
    (lh * 0.25).backward()
    try:
        torch.testing.assert_close(lh.detach(), F.cross_entropy(xf @ wf.t(), t, ignore_index=-100).detach(),
                                   rtol=1e-5, atol=0)
        torch.testing.assert_close(xl.grad, xf.grad, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(wl.grad, wf.grad[rank * vl:(rank + 1) * vl], rtol=1e-4, atol=1e-6)
    except AssertionError as e:
        bad["fused torch path"] = str(e)
    everywhere_equal("fused loss", lh)

    # ---- the switch on a small CPU model ----
    I = 32

    class Attn(nn.Module):
        def __init__(self):
            super().__init__()
            self.q_proj, self.k_proj, self.v_proj = (nn.Linear(H, H, bias=False) for _ in range(3))
            self.out_proj = nn.Linear(H, H, bias=False)

    class Mlp(nn.Module):
        def __init__(self):
            super().__init__()
            self.up_proj, self.gate_proj = nn.Linear(H, I, bias=False), nn.Linear(H, I, bias=False)
            self.down_proj = nn.Linear(I, H, bias=False)

    class Layer(nn.Module):
        def __init__(self):
            super().__init__()
            self.attention, self.mlp = Attn(), Mlp()

        def forward(self, x):
            x = x + self.attention.out_proj(torch.tanh(self.attention.q_proj(x)))
            return x + self.mlp.down_proj(self.mlp.up_proj(x) * torch.sigmoid(self.mlp.gate_proj(x)))

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.embedding = nn.Embedding(V, H)
            self.decoder_layers = nn.ModuleList([Layer()])
            self.final_proj = nn.Linear(H, V, bias=False)

        def forward(self, input_ids, return_hidden=False):
            x = self.embedding(input_ids)
            for layer in self.decoder_layers:
                x = layer(x)
            return x if return_hidden else self.final_proj(x)

    torch.manual_seed(0)
    plain = Tiny()
    default, marked = Tiny(), Tiny()
    default.load_state_dict(plain.state_dict())
    marked.load_state_dict(plain.state_dict())
    TP.apply_tensor_parallel(default, shard_weights=True)
    TP.apply_tensor_parallel(marked, shard_weights=True, vocab_parallel_loss=True)
    # everything that communicates runs first, on every rank alike; the assertions follow
    ids = torch.randint(0, V, (2, 9), generator=g)
    inp, tgt = ids[:, :-1], ids[:, 1:].clone()
    tgt[0, 3] = -100
    shapes = (tuple(marked(inp).shape), tuple(default(inp).shape), tuple(marked(inp, return_hidden=True).shape))
    want = F.cross_entropy(plain(inp).reshape(-1, V), tgt.reshape(-1)) / 2
    want.backward()
    # the model's own forward on the sharded head, then the loss on this rank's logits ...
    local = marked(inp)
    got = VPL.vocab_parallel_cross_entropy(local.reshape(-1, vl), tgt.reshape(-1)) / 2
    got.backward()
    # ... and the LM head fused with the loss, on a second copy
    fused_m = Tiny()
    fused_m.load_state_dict(plain.state_dict())
    TP.apply_tensor_parallel(fused_m, shard_weights=True, vocab_parallel_loss=True)
    fused = VPL.vocab_parallel_lm_head_cross_entropy(fused_m(inp, return_hidden=True), fused_m.final_proj.weight,
                                                     tgt.reshape(-1)) / 2
    fused.backward()
    same, _ = train._forward_loss(default, inp, tgt, 2)  # the default head: the gathered logits, as before
    everywhere_equal("model loss", got)
    everywhere_equal("fused model loss", fused)
    try:
        assert default.final_proj.gather_output and not hasattr(default.final_proj, "vocab_parallel_loss")
        assert marked.final_proj.gather_output is False and marked.final_proj.vocab_parallel_loss is True
        assert shapes == ((2, 8, vl), (2, 8, V), (2, 8, H)), shapes
        for loss in (got, fused, same):
            torch.testing.assert_close(loss.detach(), want.detach(), rtol=1e-5, atol=0)
        for m in (marked, fused_m):
            torch.testing.assert_close(m.final_proj.weight.grad,
                                       plain.final_proj.weight.grad[rank * vl:(rank + 1) * vl], rtol=1e-4, atol=1e-7)
            torch.testing.assert_close(m.embedding.weight.grad, plain.embedding.weight.grad[rank * vl:(rank + 1) * vl],
                                       rtol=1e-4, atol=1e-7)
    except AssertionError as e:
        bad["switch"] = repr(e)
    dist.barrier()
    dist.destroy_process_group()
    if bad:
        raise AssertionError(f"rank {rank}: {bad}")


@pytest.mark.parametrize("world", [2, 4])
def test_vocab_parallel_loss_torch_path(world):
    mp.start_processes(_worker, args=(world, _free_port()), nprocs=world, join=True, start_method="spawn")
