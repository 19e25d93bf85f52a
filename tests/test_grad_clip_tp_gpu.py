"""One global gradient norm under tensor parallelism: tp = 2 ranks sharing this GPU (gloo, as test_tp_gpu.py) hold
the shards apply_tensor_parallel(shard_weights=True) leaves; picotron_amd.optim.clip_grad_norm_ must return, on
both ranks, the norm of the FULL model's gradients (every shard once, the replicated RMSNorm weights once, not tp
times) and scale every shard by that one coefficient. Tolerance 2**-16 relative on the norm (derived in
test_grad_clip_gpu.py; the cross-rank sum runs in double)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu
TOL = 2.0 ** -16


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
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.model import LlamaConfig, build_llama
    from picotron_amd.optim import clip_grad_norm_, get_grad_norm
    from picotron_amd.tensor_parallel.tensor_parallel import apply_tensor_parallel
    pgm.setup_process_group_manager(tp_size=world, cp_size=1, pp_size=1, dp_size=1)
    bf = torch.bfloat16
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2,
                      num_hidden_layers=2, vocab_size=512, max_position_embeddings=128)
    tp_size = pgm.tp_world_size
    pgm.tp_world_size = lambda: 1
    torch.manual_seed(42)
    full = build_llama(cfg, device="cuda", dtype=bf)  # the unsharded shapes
    pgm.tp_world_size = tp_size
    torch.manual_seed(42)
    tpm = build_llama(cfg, device="cuda", dtype=bf)
    apply_tensor_parallel(tpm, shard_weights=True)

    # synthetic full-model gradients, identical on both ranks; each rank takes its slice (test_tp_gpu.py's rule)
    g = torch.Generator(device="cpu").manual_seed(11)
    sumsq = 0.0
    n_repl = 0
    for (nf, pf), (nt, pt) in zip(full.named_parameters(), tpm.named_parameters()):
        gf = torch.randn(pf.shape, generator=g)
        shape = tuple(pt.shape)
        sharded = shape != tuple(pf.shape)
        assert bool(getattr(pt, "_pico_tp_sharded", False)) == sharded, nt
        if not sharded:  # replicated (RMSNorm weights): x10, so counting them twice moves the norm by percents
            gf = gf * 10.0
            n_repl += 1
        gf = gf.to(bf)
        sumsq += float(gf.double().square().sum())
        if sharded:
            if shape[0] != pf.shape[0]:
                n = shape[0]
                gf = gf[rank * n:(rank + 1) * n]
            else:
                n = shape[1]
                gf = gf[:, rank * n:(rank + 1) * n]
        pt.grad = gf.contiguous().to("cuda")
    assert n_repl == 2 * cfg.num_hidden_layers + 1
    ref = sumsq ** 0.5
    m = 1.0
    assert ref > 2 * m
    params = list(tpm.parameters())
    before = [p.grad.clone() for p in params]
    errors = []
    local = float(get_grad_norm(params, groups=()))
    ret = clip_grad_norm_(params, m)
    norm, coef = float(ret), ret._base[1]
    both = [torch.zeros(2, dtype=torch.float32) for _ in range(world)]
    dist.all_gather(both, ret._base.cpu())
    if not all(torch.equal(b.view(torch.int32), both[0].view(torch.int32)) for b in both):
        errors.append(f"ranks disagree: {both}")
    if not abs(norm - ref) / ref <= TOL:
        errors.append(f"norm {norm} vs fp64 {ref}: rel {abs(norm - ref) / ref:.3g}")
    if not abs(local - norm) / norm > 0.01:
        errors.append(f"groups=() local norm {local} should differ from the global norm {norm}")
    local_ref = float(sum(b.double().square().sum() for b in before)) ** 0.5
    if not abs(local - local_ref) / local_ref <= TOL:
        errors.append(f"local norm {local} vs fp64 {local_ref}")
    for p, g0 in zip(params, before):
        want = (g0.float() * coef).to(bf)
        if not torch.equal(p.grad.view(torch.int16), want.view(torch.int16)):
            errors.append(f"shard {tuple(p.shape)} not scaled by the global coefficient")
    dist.barrier()
    dist.destroy_process_group()
    if errors:
        raise AssertionError(f"rank {rank}: {errors}")


def test_clip_grad_norm_under_tensor_parallelism():
    mp.start_processes(_worker, args=(2, _free_port()), nprocs=2, join=True, start_method="spawn")
