"""The vocab-parallel loss under tensor parallelism: tp = 2 ranks sharing this GPU (gloo, as tests/test_tp_gpu.py)
run forward + loss + backward on a model converted with apply_tensor_parallel(shard_weights=True,
vocab_parallel_loss=True) — vocab_parallel_lm_head_cross_entropy on model(..., return_hidden=True), and with
PICO_UNFUSED=1 the ungathered ColumnParallelLinear head followed by vocab_parallel_cross_entropy — against the
unsharded model on the same weights (its loss through train._forward_loss): the loss, every parameter gradient
against the matching shard, the loss bit-equal on the two ranks, and model(tokens) returning this rank's
[B, S, V / tp] logits (the gathered [T, V] logits are never built)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, unfused):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ["PICO_UNFUSED"] = "1" if unfused else "0"
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from picotron_amd import process_group_manager as pgm
    from picotron_amd import train
    from picotron_amd.model import LlamaConfig, build_llama
    pgm.setup_process_group_manager(tp_size=world, cp_size=1, pp_size=1, dp_size=1)
    bf = torch.bfloat16
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2,
                      num_hidden_layers=2, vocab_size=512, max_position_embeddings=128)
    # unsharded model (built as at tp = 1) and the tp model (built under tp = world: local head counts)
    tp_size = pgm.tp_world_size
    pgm.tp_world_size = lambda: 1
    torch.manual_seed(42)
    full = build_llama(cfg, device="cuda", dtype=bf)
    pgm.tp_world_size = tp_size
    torch.manual_seed(42)
    tpm = build_llama(cfg, device="cuda", dtype=bf)
    g = torch.Generator(device="cpu").manual_seed(3)
    with torch.no_grad():
        full.final_proj.weight.copy_((torch.randn(full.final_proj.weight.shape, generator=g) * 0.02).to(bf))
        for pf, pt in zip(full.parameters(), tpm.parameters()):
            pt.copy_(pf)
    from picotron_amd.tensor_parallel.tensor_parallel import apply_tensor_parallel
    apply_tensor_parallel(tpm, shard_weights=True, vocab_parallel_loss=True)
    from picotron_amd.tensor_parallel import vocab_parallel_loss as VPL
    assert tpm.final_proj.vocab_parallel_loss is True and tpm.final_proj.gather_output is False
    toks = torch.randint(0, cfg.vocab_size, (2, 129), generator=g).to("cuda")
    inp, tgt = toks[:, :-1].contiguous(), toks[:, 1:].contiguous()

    loss_f, _ = train._forward_loss(full, inp, tgt, 1)  # the unsharded model's own path (fused LM head + CE, or not)
    loss_f.backward()
    loss_f = loss_f.detach().float()
    if unfused:  # the ungathered ColumnParallelLinear head, then the loss on this rank's logits
        local = tpm(input_ids=inp)
        loss_t = VPL.vocab_parallel_cross_entropy(local.reshape(-1, local.shape[-1]), tgt.reshape(-1))
    else:  # the LM head fused with the loss
        h = tpm(input_ids=inp, return_hidden=True)
        loss_t = VPL.vocab_parallel_lm_head_cross_entropy(h, tpm.final_proj.weight, tgt.reshape(-1))
    loss_t.backward()
    loss_t = loss_t.detach().float()
    with torch.no_grad():
        local_shape = tuple(tpm(inp).shape)
    both = [torch.empty_like(loss_t) for _ in range(world)]
    dist.all_gather(both, loss_t)
    torch.cuda.synchronize()

    def rel(a, b):
        a, b = a.double(), b.double()
        return float((a - b).norm() / b.norm().clamp_min(1e-30))

    errs = {"loss": abs(float(loss_t) - float(loss_f))}
    for (nf, pf), (nt, pt) in zip(full.named_parameters(), tpm.named_parameters()):
        gf = pf.grad
        shape = tuple(pt.shape)
        if shape != tuple(pf.shape):  # sharded: column (rows) or row (columns) parallel
            if shape[0] != pf.shape[0]:
                n = shape[0]
                gf = gf[rank * n:(rank + 1) * n]
            else:
                n = shape[1]
                gf = gf[:, rank * n:(rank + 1) * n]
        errs["grad:" + nt] = rel(pt.grad, gf)
    bad = {k: v for k, v in errs.items() if not v < (2e-2 if k != "loss" else 5e-3)}
    if not all(torch.equal(b, both[0]) for b in both):
        bad["loss differs between ranks"] = [float(b) for b in both]
    if local_shape != (2, 128, cfg.vocab_size // world):  # this rank's logits: nothing [T, V]-shaped is returned
        bad["model(tokens) shape"] = local_shape
    dist.barrier()
    dist.destroy_process_group()
    if bad:
        raise AssertionError(f"rank {rank}: {bad}")


@pytest.mark.parametrize("unfused", [False, True])
def test_vocab_parallel_loss_matches_unsharded(unfused):
    mp.start_processes(_worker, args=(2, _free_port(), unfused), nprocs=2, join=True, start_method="spawn")
