"""AdamW on the gfx950 pico_adamw_bf16 kernel: one launch updates every parameter.

Drop-in for the reference's optimizer, `torch.optim.AdamW(model.parameters(), lr=..., fused=...)`
(ref train.py:13,204-209; stepped at :235, zeroed at :221): same constructor arguments and defaults,
same `param_groups` / `state` layout (`step`, `exp_avg`, `exp_avg_sq` per parameter, states in the
parameter dtype), so checkpoints and LR schedules see a torch AdamW. The update has ATen's fused
AdamW expression order and types (decoupled weight decay; see csrc/adamw.hip). Parameters and
gradients must be bf16 HIP tensors (the training dtype of the hot path); anything else raises —
there is no CPU or eager fallback.

Global-norm gradient clipping (csrc/grad_clip.hip) on the same device tables: `clip_grad_norm_` /
`get_grad_norm` replace `torch.nn.utils.clip_grad_norm_` / `get_total_norm` (one launch over the whole list, the
norm and the coefficient stay on the device, fixed summation order, fp32 main_grads of
DataParallelBucket(defer_grad_cast=True) read in place, one norm under tensor / pipeline parallelism), and
`AdamW(max_grad_norm=...)` folds the clip into the optimizer's gradient load.

`AdamW(master_weights=True)` (pico_adamw_master): fp32 master weights and fp32 moments under the bf16 parameters, the
mixed-precision recipes' arrangement, on the same tables and in the same one launch.

`AdamW(stochastic_rounding=True)` (pico_adamw_bf16_sr): the bf16 step with the parameter and both moments rounded
stochastically from a counter-based generator: small updates and slow decays survive on average at the bf16 step's
state size and traffic.

`Muon` (csrc/muon.hip): torch.optim.Muon for the 2-D hidden matrices on the same tables: three whole-list HIP kernels
(momentum, normalise, update) around the Newton-Schulz GEMMs; `muon_param_split` picks the
matrices Muon takes from a Llama and leaves the rest to AdamW.
"""
import math

import torch

from . import _lib


def _deferred_grad(p):
    """The fp32 main_grad the step reads instead of .grad when DataParallelBucket(defer_grad_cast=True) left
    the bf16 .grad cast to the optimizer (the kernel rounds it to bf16 in register, as the cast would)."""
    g32 = getattr(p, "_pico_grad_f32", None)
    if g32 is None or not getattr(p, "_pico_grad_deferred", False):
        return None
    if g32.dtype != torch.float32 or not g32.is_contiguous() or g32.shape != p.shape:
        raise ValueError("picotron_amd.optim.AdamW: deferred-cast gradient must be a contiguous fp32 main_grad")
    return g32


def _new_tables(numels, dev, sixth=None):
    """Device tables of one parameter set: sizes / 64 Ki-element chunks (fixed for the set) and the [n][5] pointer
    table with its two pinned staging buffers (see _sync_ptrs). sixth: the pointer tuples carry a sixth entry, which
    goes to a second device table [n] of that name behind the first in the same buffer: "masters", the fp32 master
    parameter address (AdamW(master_weights=True)), "ids", the generator's tensor id
    (AdamW(stochastic_rounding=True)), or "out", the address of the orthogonalised update (Muon)."""
    chunk = int(_lib.load().pico_adamw_chunk_elems())
    sizes = torch.tensor(numels, dtype=torch.int64)
    chunks = torch.tensor([(i, c) for i, n in enumerate(numels) for c in range(0, n, chunk)],
                          dtype=torch.int64).reshape(-1, 2)
    n = len(numels)
    buf = torch.empty(n * (6 if sixth else 5), dtype=torch.int64, device=dev)  # one upload: [n][5], then [n]
    return {"buf": buf, "tens": buf[:5 * n].view(n, 5), "masters": buf[5 * n:] if sixth == "masters" else None,
            "ids": buf[5 * n:] if sixth == "ids" else None, "out": buf[5 * n:] if sixth == "out" else None,
            "sizes": sizes.to(dev), "chunks": chunks.to(dev), "chunks_host": chunks, "n_chunks": chunks.shape[0],
            "ptrs": None, "turn": 0, "host": [torch.empty_like(buf, device="cpu").pin_memory() for _ in range(2)],
            "done": [None, None], "norm": None}


def _sync_ptrs(ent, ptrs, dev):
    """Re-upload the pointer table only when a pointer changed (persistent gradients: never after the first
    step); two pinned staging buffers used in turn."""
    if ptrs != ent["ptrs"]:
        i = ent["turn"]
        if ent["done"][i] is not None:  # this staging buffer may still be feeding its previous copy
            ent["done"][i].synchronize()
        n, host = len(ptrs), ent["host"][i].numpy()
        host[:5 * n].reshape(n, 5)[:] = [t[:5] for t in ptrs]
        if host.size > 5 * n:  # the sixth entries: masters, ids or out
            host[5 * n:] = [t[5] for t in ptrs]
        ent["buf"].copy_(ent["host"][i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        ent["done"][i] = ev
        ent["turn"] = 1 - i
        ent["ptrs"] = ptrs


def select_norm_params(params, tp_rank, tp_world_size):
    """Which of `params` this rank adds to its local sum of squares, one bool each, so that the sum over a
    tensor-parallel group counts every element of the model once: a parameter tagged `_pico_tp_sharded` (a
    ColumnParallelLinear / RowParallelLinear / VocabParallelEmbedding shard) is this rank's alone and always
    counts; an untagged one (RMSNorm weights, the row-parallel bias) is replicated on every tp rank and counts
    on tp rank 0 only. tp_world_size 1: everything counts."""
    if tp_world_size <= 1 or tp_rank == 0:
        return [True] * len(params)
    return [bool(getattr(p, "_pico_tp_sharded", False)) for p in params]


def _norm_groups(groups):
    """(process groups the sum of squares is all-reduced over, tp_rank, tp_world_size for select_norm_params).
    groups None: tp_group if tp > 1 and pp_group if pp > 1 of the process_group_manager, when it is set up (DP and
    CP ranks hold identical synced gradients: nothing to reduce); groups=(): local only, every parameter counts."""
    from . import process_group_manager as pgm
    m = pgm.process_group_manager
    if groups is None:
        groups = []
        if m is not None:
            if m.tp_world_size > 1:
                groups.append(m.tp_group)
            if m.pp_world_size > 1:
                groups.append(m.pp_group)
    groups = tuple(groups)
    if not groups or m is None:
        return groups, 0, 1
    return groups, m.tp_rank, m.tp_world_size


def _sqnorm(lib, ent, keep, stream):
    """Launch pico_grad_sqnorm over the chunks of the kept tensors of a table set; returns its 1-element device
    double. The chunk list, the partial-sum workspace and the result live next to the tables (allocated once)."""
    keep = tuple(keep)
    nrm = ent["norm"]
    if nrm is None or nrm["keep"] != keep:
        dev = ent["tens"].device
        if all(keep):
            chunks, n = ent["chunks"], ent["n_chunks"]
        else:
            host = ent["chunks_host"]
            host = host[torch.tensor(keep, dtype=torch.bool)[host[:, 0]]] if host.shape[0] else host
            chunks, n = host.to(dev), host.shape[0]
        ws = int(lib.pico_grad_sqnorm_workspace_bytes(n))
        nrm = ent["norm"] = {"keep": keep, "chunks": chunks, "n_chunks": n,
                             "ws": torch.empty(max(ws // 4, 1), dtype=torch.float32, device=dev),
                             "sumsq": torch.empty(1, dtype=torch.float64, device=dev)}
    _lib.check(lib.pico_grad_sqnorm(_lib.ptr(ent["tens"]), _lib.ptr(ent["sizes"]), _lib.ptr(nrm["chunks"]),
                                    nrm["n_chunks"], _lib.ptr(nrm["ws"]), _lib.ptr(nrm["sumsq"]), stream),
               "pico_grad_sqnorm")
    return nrm["sumsq"]


def _norm_coef(lib, sums, groups, max_norm, stream):
    """The device (total norm, clip coefficient) pair from the table sets' sums of squares: added in list order,
    all-reduced (SUM, double) over each group, then pico_grad_clip_coef. Nothing is read on the host."""
    total = sums[0]
    for s in sums[1:]:
        total = total + s
    if groups:
        import torch.distributed as dist
        for g in groups:
            dist.all_reduce(total, op=dist.ReduceOp.SUM, group=g)
    out = torch.empty(2, dtype=torch.float32, device=total.device)
    _lib.check(lib.pico_grad_clip_coef(_lib.ptr(total), float(max_norm), _lib.ptr(out), stream), "pico_grad_clip_coef")
    return out


_STANDALONE = {}  # clip_grad_norm_ / get_grad_norm: tables per parameter list, as AdamW._tables


def _grad_tables(parameters):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return params, None
    ptrs = []
    for p in params:
        g32 = _deferred_grad(p)
        g = g32 if g32 is not None else p.grad
        if not g.is_cuda or (g32 is None and g.dtype != torch.bfloat16):
            raise TypeError(f"picotron_amd.optim: gradients must be bf16 HIP tensors, got {g.dtype} on {g.device}")
        if g.is_sparse or not g.is_contiguous():
            raise ValueError("picotron_amd.optim: dense contiguous gradients only")
        ptrs.append((0, g.data_ptr(), 0, 0, 0 if g32 is None else 1))
    dev = params[0].grad.device
    key = (dev, tuple((p.data_ptr(), p.numel()) for p in params))
    ent = _STANDALONE.get(key)
    if ent is None:
        ent = _new_tables([p.numel() for p in params], dev)
        if len(_STANDALONE) > 16:
            _STANDALONE.clear()
        _STANDALONE[key] = ent
    _sync_ptrs(ent, ptrs, dev)
    return params, ent


def _total_norm(parameters, max_norm, groups):
    params, ent = _grad_tables(parameters)
    if ent is None:
        return None, None, None
    lib = _lib.load()
    stream = _lib.stream_of(params[0].grad)
    groups, tp_rank, tp_world = _norm_groups(groups)
    s = _sqnorm(lib, ent, select_norm_params(params, tp_rank, tp_world), stream)
    return _norm_coef(lib, [s], groups, max_norm, stream), ent, stream


@torch.no_grad()
def get_grad_norm(parameters, *, groups=None):
    """The global L2 norm of the gradients of `parameters`, a 0-dim fp32 device tensor (no host read). bf16
    gradients, or the fp32 main_grad DataParallelBucket(defer_grad_cast=True) left (read as bf16(g), the value the
    deferred cast would store: no materialize_grads() needed). `groups`: see clip_grad_norm_."""
    nc, _, _ = _total_norm(parameters, math.inf, groups)
    return torch.zeros((), dtype=torch.float32) if nc is None else nc[0]


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None, *, groups=None):
    """torch.nn.utils.clip_grad_norm_ on the gfx950 kernels: scales the gradients in place by
    min(1, max_norm / (total_norm + 1e-6)) and returns the total pre-clip norm (0-dim fp32 device tensor). Three
    launches over the whole list; the norm and the coefficient stay on the device, so the host does not wait
    (error_if_nonfinite=True is the one path that reads the norm: RuntimeError, as torch). A non-finite norm
    leaves the gradients as they are. A deferred fp32 main_grad is read and scaled in place (to the value its
    bf16 form would hold), without materialize_grads().

    Model parallelism: one norm for the whole model. Each tensor-parallel rank sums its own shards (parameters
    tagged `_pico_tp_sharded` by tensor_parallel.py) and tp rank 0 the replicated parameters, then the sum of
    squares is all-reduced over every process group in `groups` (None: the process_group_manager's tp and pp
    groups where > 1; (): none — the local norm of everything this rank holds)."""
    if float(norm_type) != 2.0:
        raise NotImplementedError("picotron_amd.optim.clip_grad_norm_: norm_type 2 only")
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError(f"clip_grad_norm_: max_norm must be >= 0, got {max_norm}")
    nc, ent, stream = _total_norm(parameters, max_norm, groups)
    if nc is None:
        return torch.zeros((), dtype=torch.float32)
    if error_if_nonfinite and not bool(torch.isfinite(nc[0])):
        raise RuntimeError("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot "
                           "be clipped. To disable this error and scale the gradients by the non-finite norm "
                           "anyway, set `error_if_nonfinite=False`")
    _lib.check(_lib.load().pico_grad_scale(_lib.ptr(ent["tens"]), _lib.ptr(ent["sizes"]), _lib.ptr(ent["chunks"]),
                                           ent["n_chunks"], _lib.ptr(nc), stream), "pico_grad_scale")
    return nc[0]


class AdamW(torch.optim.Optimizer):
    # reads DataParallelBucket(defer_grad_cast=True)'s fp32 main_grad itself: the bucket's step pre-hook leaves
    # the deferred cast to this optimizer (see data_parallel.py)
    reads_deferred_grads = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                 max_grad_norm=None, grad_norm_groups=None, master_weights=False, stochastic_rounding=False,
                 sr_seed=None):
        """max_grad_norm (an extension; None: off, the step runs exactly as without it): clip the global L2
        gradient norm inside the step. One norm over every parameter that has a gradient (all param groups and
        step counts; `grad_norm_groups`: the `groups` of clip_grad_norm_), then pico_adamw_bf16_clip scales each
        gradient as it loads it — bit-identical to clip_grad_norm_ followed by the plain step, without the
        gradient write and re-read. `self.grad_norm` is the pre-clip norm (0-dim device tensor) after each step.
        The host never reads the norm: when it is not finite the kernel writes nothing (parameters and moments
        stay as they were) but the per-parameter `step` counters have already advanced; watch `grad_norm`.

        master_weights (an extension; False: the bf16 step above, untouched): fp32 master weights and fp32 Adam
        moments under the bf16 model, the Megatron / DeepSpeed / torch-AMP arrangement, still one launch
        (pico_adamw_master; with max_grad_norm, the clip folded in). `state[p]` holds `master_param` (created at the
        parameter's first step as `p.float()`, exact), `exp_avg` and `exp_avg_sq`, all fp32: 12 bytes of state per
        parameter instead of 4. The update is ATen's fused AdamW on the fp32 tensors with the bf16 gradient values;
        the bf16 parameter is overwritten in place with bf16(master) and never read, so a parameter written from
        outside (model.load_state_dict after the first step) is overridden by its master at the next step unless
        sync_master_params() is called. state_dict() / load_state_dict() keep the fp32 state fp32; a checkpoint of
        the bf16 form loads too (moments upcast exactly, masters created from the parameters at the next step).

        stochastic_rounding (an extension; False: the bf16 step above, untouched): the bf16 step, state and traffic
        (pico_adamw_bf16_sr; with max_grad_norm, the clip folded in), but the parameter, exp_avg and exp_avg_sq are
        rounded from their fp32 results to one of the two bf16 neighbours with probability proportional to distance
        instead of to the nearest: unbiased, so updates below half a bf16 ulp and the beta2 = 0.999 decay survive on
        average, where the plain bf16 step loses them. Not together with master_weights (which needs no such cure).
        The random bits are Philox4x32-10 of (sr_seed, the parameter's step count, the parameter's running index
        over param_groups, the element), evaluated in registers: no generator state, the same bits on every run, under
        graph replay and after a checkpoint resume. sr_seed None: torch.initial_seed() at construction; kept as
        `self.sr_seed` (64 bits). state_dict() then carries a top-level "sr_seed", which load_state_dict adopts."""
        if amsgrad or maximize or capturable or differentiable:
            raise NotImplementedError("picotron_amd.optim.AdamW: amsgrad / maximize / capturable / differentiable")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid AdamW hyper-parameters lr={lr} betas={betas} eps={eps}")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:  # negative or NaN
            raise ValueError(f"invalid AdamW max_grad_norm={max_grad_norm}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=fused)
        if stochastic_rounding and master_weights:
            raise ValueError("picotron_amd.optim.AdamW: stochastic_rounding rounds bf16 state; master_weights keeps "
                             "fp32 state and needs none: choose one")
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm_groups = grad_norm_groups
        self.grad_norm = None
        self.master_weights = bool(master_weights)  # not a param-group default: state_dict() reports torch's keys
        self.stochastic_rounding = bool(stochastic_rounding)  # an attribute too, for the same reason
        self.sr_seed = (torch.initial_seed() if sr_seed is None else int(sr_seed)) & 0xFFFFFFFFFFFFFFFF
        self._sr_ids = {}
        # per (group, parameter set): device tables of sizes / 64 Ki-element chunks (fixed for the set) and of
        # the (param, grad, exp_avg, exp_avg_sq) pointers, re-uploaded only when a pointer changed (persistent
        # gradients: never after the first step); two pinned staging buffers used in turn
        self._tables = {}

    def _group_tables(self, gi, params):
        # keyed by pointer AND size: a parameter re-pointed at a different-sized tensor that the caching
        # allocator placed at the same address gets new size / chunk tables
        key = (gi, tuple((p.data_ptr(), p.numel()) for p in params))
        ent = self._tables.get(key)
        if ent is None:
            sixth = "masters" if self.master_weights else "ids" if self.stochastic_rounding else None
            ent = _new_tables([p.numel() for p in params], params[0].device, sixth)
            if len(self._tables) > 64:  # parameter sets keep changing (step counts diverging): keep the map small
                self._tables.clear()
            self._tables[key] = ent
        ptrs = []
        ids = self._param_ids() if self.stochastic_rounding else None
        for p in params:
            g32 = _deferred_grad(p)
            st = self.state[p]
            ptrs.append((p.data_ptr(), (g32 if g32 is not None else p.grad).data_ptr(),
                         st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), 0 if g32 is None else 1)
                        + ((st["master_param"].data_ptr(),) if self.master_weights else ())
                        + ((ids[p],) if ids is not None else ()))
        _sync_ptrs(ent, ptrs, params[0].device)
        return ent

    def _param_ids(self):
        """The generator's tensor ids: a parameter's running index over param_groups in order, over all parameters
        (not only those with a gradient), so an id does not shift when another parameter skips a step."""
        n = sum(len(g["params"]) for g in self.param_groups)
        if len(self._sr_ids) != n:  # first use, or add_param_group since
            self._sr_ids = {p: i for i, p in enumerate(q for g in self.param_groups for q in g["params"])}
        return self._sr_ids

    def zero_grad(self, set_to_none=True):
        """torch.optim.Optimizer.zero_grad; zeroing in place (set_to_none=False: persistent gradient buffers,
        as HIP-graph replay needs) runs as multi-tensor launches instead of one launch per parameter."""
        if set_to_none:
            return super().zero_grad(set_to_none=True)
        grads = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    if p.grad.grad_fn is not None:
                        p.grad.detach_()
                    else:
                        p.grad.requires_grad_(False)
                    grads.append(p.grad)
        if grads:
            torch._foreach_zero_(grads)

    def _advance(self, group):
        """Validate a group's parameters that have a gradient, create / advance their states, and return
        [(step count, parameters)] sorted by step count (empty: no gradient in the group)."""
        params = [p for p in group["params"] if p.grad is not None]
        if not params:
            return []
        # validate everything before touching any state (a failed step leaves the state as it was)
        for p in params:
            if not (p.is_cuda and p.dtype == torch.bfloat16 and p.grad.dtype == torch.bfloat16):
                raise TypeError("picotron_amd.optim.AdamW: parameters and gradients must be bf16 HIP tensors, "
                                f"got {p.dtype} / {p.grad.dtype} on {p.device}")
            if p.grad.is_sparse or not p.grad.is_contiguous() or not p.is_contiguous():
                raise ValueError("picotron_amd.optim.AdamW: dense contiguous parameters and gradients only")
        if self.master_weights:  # fp32 state only: a state of another dtype was not loaded through load_state_dict
            for p in params:
                for key in ("exp_avg", "exp_avg_sq", "master_param"):
                    t = self.state[p].get(key)
                    if t is not None and (t.dtype != torch.float32 or t.device != p.device or t.shape != p.shape
                                          or not t.is_contiguous()):
                        raise TypeError(f"picotron_amd.optim.AdamW(master_weights=True): state '{key}' must be a "
                                        f"contiguous fp32 tensor of the parameter's shape and device, got {t.dtype} "
                                        f"{tuple(t.shape)} on {t.device}")
        if self.stochastic_rounding:
            for p in params:
                if p.numel() >= 1 << 35:  # the generator's counter word holds (element index >> 3)
                    raise ValueError("picotron_amd.optim.AdamW(stochastic_rounding=True): parameters of fewer than "
                                     f"2**35 elements only, got {p.numel()}")
        state_dtype = torch.float32 if self.master_weights else None
        # per-parameter step counts, as torch.optim.AdamW keeps them: a parameter that had no gradient on
        # some steps (frozen for a while, an idle pipeline stage) advances only when it has one; one
        # launch per distinct step count. `step` stays a CPU scalar (a loaded state may carry it on the
        # device: moved back once, so reading it costs no host sync per step).
        by_step = {}
        for p in params:
            st = self.state[p]
            if not st:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, dtype=state_dtype, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, dtype=state_dtype, memory_format=torch.preserve_format)
            elif st["step"].device.type != "cpu":
                st["step"] = st["step"].detach().to("cpu", torch.float32)
            if self.master_weights and "master_param" not in st:  # first step, or a loaded bf16-form checkpoint
                st["master_param"] = p.detach().float()
            st["step"] += 1
            by_step.setdefault(int(st["step"].item()), []).append(p)
        return sorted(by_step.items())

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        if self.max_grad_norm is None:  # group by group, each table set on its own stream
            for gi, group in enumerate(self.param_groups):
                for step, ps in self._advance(group):
                    self._launch(lib, self._group_tables(gi, ps), group, step, None, _lib.stream_of(ps[0]))
            return loss
        # with max_grad_norm: every (group, step count) table set first, one global norm over all of them, then
        # one launch per set with the same device (norm, coefficient) pair, all on the first set's stream
        work = []
        for gi, group in enumerate(self.param_groups):
            for step, ps in self._advance(group):
                work.append((group, step, ps, self._group_tables(gi, ps)))
        if not work:
            return loss
        stream = _lib.stream_of(work[0][2][0])
        groups, tp_rank, tp_world = _norm_groups(self.grad_norm_groups)
        sums = [_sqnorm(lib, ent, select_norm_params(ps, tp_rank, tp_world), stream) for _, _, ps, ent in work]
        nc = _norm_coef(lib, sums, groups, self.max_grad_norm, stream)
        for group, step, _, ent in work:
            self._launch(lib, ent, group, step, nc, stream)
        self.grad_norm = nc[0]
        return loss

    def _launch(self, lib, ent, group, step, norm_coef, stream):
        """One launch over a table set: the master, stochastic-rounding or plain bf16 step, with the clip folded in
        when norm_coef (the device (norm, coefficient) pair) is given."""
        nc = _lib.ptr(norm_coef)
        if self.master_weights:
            fn, sixth, tail = lib.pico_adamw_master, (_lib.ptr(ent["masters"]),), (nc, stream)
        elif self.stochastic_rounding:
            fn, sixth, tail = lib.pico_adamw_bf16_sr, (_lib.ptr(ent["ids"]),), (nc, self.sr_seed, stream)
        elif norm_coef is not None:
            fn, sixth, tail = lib.pico_adamw_bf16_clip, (), (nc, stream)
        else:
            fn, sixth, tail = lib.pico_adamw_bf16, (), (stream,)
        beta1, beta2 = group["betas"]
        _lib.check(fn(_lib.ptr(ent["tens"]), *sixth, _lib.ptr(ent["sizes"]), _lib.ptr(ent["chunks"]), ent["n_chunks"],
                      float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]),
                      step, *tail), fn.__name__)

    def state_dict(self):
        """torch.optim.Optimizer.state_dict; with stochastic_rounding=True it also carries "sr_seed" at the top
        level, so a resumed run draws the bits the uninterrupted run would have."""
        sd = super().state_dict()
        if self.stochastic_rounding:
            sd["sr_seed"] = self.sr_seed
        return sd

    @torch.no_grad()
    def sync_master_params(self):
        """Re-read every existing fp32 master from its bf16 parameter (in place: the device tables stay valid).
        Call it after writing model weights into an already-stepped optimizer (model.load_state_dict, a manual
        `p.copy_`): the kernel never reads the bf16 parameter, so without it the master silently wins and the next
        step overwrites the new weights. Nothing to do before the first step or with master_weights=False."""
        for p, st in self.state.items():
            master = st.get("master_param")
            if master is not None:
                master.copy_(p.detach())

    def load_state_dict(self, state_dict):
        """torch.optim.Optimizer.load_state_dict casts every floating-point state tensor but `step` to the
        parameter's dtype, which would round fp32 masters and moments to bf16. With master_weights=True they are
        taken from `state_dict` again afterwards as fp32 (fp32 input: bit for bit, own copies; the bf16 moments of
        a bf16-form checkpoint: upcast exactly; `step` its own copy too, so an optimizer loaded from another live
        optimizer's state_dict() shares nothing with it). master_weights=False: torch's loading, unchanged, and with
        stochastic_rounding=True the checkpoint's "sr_seed", when it has one, becomes this optimizer's."""
        super().load_state_dict(state_dict)
        if self.stochastic_rounding and state_dict.get("sr_seed") is not None:
            self.sr_seed = int(state_dict["sr_seed"]) & 0xFFFFFFFFFFFFFFFF
        if not self.master_weights:
            return
        from itertools import chain
        saved = chain.from_iterable(g["params"] for g in state_dict["param_groups"])
        mine = chain.from_iterable(g["params"] for g in self.param_groups)
        id_map = dict(zip(saved, mine))
        for k, sv in state_dict["state"].items():
            p = id_map.get(k)
            if p is None or not isinstance(sv, dict):
                continue
            if isinstance(sv.get("step"), torch.Tensor):  # torch hands the very tensor over; _advance adds in place
                self.state[p]["step"] = sv["step"].detach().clone()
            for key in ("exp_avg", "exp_avg_sq", "master_param"):
                v = sv.get(key)
                if isinstance(v, torch.Tensor) and v.is_floating_point():
                    t = v.detach().to(device=p.device, dtype=torch.float32)
                    self.state[p][key] = t.clone() if t.data_ptr() == v.data_ptr() else t


# ---- Muon ----

def muon_param_split(model):
    """(muon_params, other_params) of a Llama (picotron_amd.model): Muon takes the 2-D hidden matrices, i.e. the
    parameters with ndim == 2 whose name starts with `decoder_layers.`; everything else (the embedding, final_proj
    and all norms) is AdamW's. Every parameter lands in exactly one list, in named_parameters() order."""
    muon, other = [], []
    for name, p in model.named_parameters():
        (muon if p.ndim == 2 and name.startswith("decoder_layers.") else other).append(p)
    return muon, other


def _muon_ratio(adjust_lr_fn, shape):
    """torch.optim._muon._adjust_lr's ratio (double): adjusted_lr = lr * ratio."""
    A, B = shape
    if adjust_lr_fn is None or adjust_lr_fn == "original":
        return math.sqrt(max(1, A / B))
    if adjust_lr_fn == "match_rms_adamw":
        return 0.2 * math.sqrt(max(A, B))
    raise ValueError(f"Adjust learning rate function {adjust_lr_fn} is not supported")


def _muon_layout(shapes, adjust_lr_fn=None):
    """The host half of Muon's tables for matrices of `shapes`, in list order: `chunk_start` ([n + 1], the first
    64 Ki-element chunk of each tensor), `ratios` (torch's _adjust_lr ratio of each), `buckets` ({shape: tensor
    indices}, shapes in order of first appearance: a bucket's Newton-Schulz inputs are one [L, A, B] buffer) and
    `slot` (each tensor's (shape, position in its bucket))."""
    chunk = int(_lib.load().pico_adamw_chunk_elems())
    shapes = [tuple(int(d) for d in s) for s in shapes]
    chunk_start = [0]
    for a, b in shapes:
        chunk_start.append(chunk_start[-1] + (a * b + chunk - 1) // chunk)
    buckets, slot = {}, []
    for i, s in enumerate(shapes):
        idx = buckets.setdefault(s, [])
        slot.append((s, len(idx)))
        idx.append(i)
    return {"shapes": shapes, "chunk_start": chunk_start, "ratios": [_muon_ratio(adjust_lr_fn, s) for s in shapes],
            "buckets": buckets, "slot": slot}


def _muon_work(layout, dev):
    """The Newton-Schulz input buffers of a layout: ({shape: [L, A, B] bf16 buffer}, each tensor's slice of its
    bucket's buffer, in list order): 2 bytes per Muon parameter."""
    bufs = {s: torch.empty((len(idx),) + s, dtype=torch.bfloat16, device=dev) for s, idx in layout["buckets"].items()}
    return bufs, [bufs[s][k] for s, k in layout["slot"]]


def _muon_ns_plan(layout, slices, dev):
    """The persistent Newton-Schulz workspace, sized for the largest matrix and shared by all: two ping-pong
    buffers and the two Gram buffers (G, G2); and per matrix the views the GEMMs take (X: the matrix's slice of the
    work buffer, where the result lands again)."""
    pp = max(s[0] * s[1] for s in layout["shapes"])
    gg = max(min(s) ** 2 for s in layout["shapes"])
    flat = [torch.empty(n, dtype=torch.bfloat16, device=dev) for n in (pp, pp, gg, gg)]
    plan = []
    for s, x in zip(layout["shapes"], slices):
        m = min(s)
        plan.append({"X": x, "P": [flat[0][:s[0] * s[1]].view(s), flat[1][:s[0] * s[1]].view(s)],
                     "G": flat[2][:m * m].view(m, m), "G2": flat[3][:m * m].view(m, m), "tall": s[0] > s[1]})
    return flat, plan


def _newton_schulz(plan, coefficients, ns_steps):
    """ns_steps times G = X X^T, G2 = b G + c G G, X = a X + G2 X per matrix, as bf16 GEMMs (torch.mm /
    torch.addmm, the calls torch's Muon makes) into the plan's buffers. A tall matrix [A, B] (A > B) is iterated as
    it lies, without a transposed copy: with Y = X^T the same sums read G = Y^T Y, Y = a Y + Y G2^T, the GEMM
    taking the transposes. The result is left in X, contiguous in the parameter's layout."""
    a, b, c = coefficients
    for sb in plan:
        X, (P0, P1), G, G2 = sb["X"], sb["P"], sb["G"], sb["G2"]
        cur = X
        for k in range(ns_steps):
            nxt = X if (k == ns_steps - 1 and cur is not X) else (P1 if cur is P0 else P0)
            if sb["tall"]:
                torch.mm(cur.T, cur, out=G)
                torch.addmm(G, G, G, beta=b, alpha=c, out=G2)
                torch.addmm(cur, cur, G2.T, beta=a, out=nxt)
            else:
                torch.mm(cur, cur.T, out=G)
                torch.addmm(G, G, G, beta=b, alpha=c, out=G2)
                torch.addmm(cur, G2, cur, beta=a, out=nxt)
            cur = nxt
        if cur is not X:  # ns_steps == 1: a GEMM cannot write over its own input
            X.copy_(cur)


class Muon(torch.optim.Optimizer):
    """torch.optim.Muon on the gfx950 kernels of csrc/muon.hip, for bf16 matrices on a HIP device: torch's positional
    signature and defaults, the same `param_groups` keys and the same `state[p]` layout (`momentum_buffer` only, in
    the parameter dtype, no step counter), so state_dict() / load_state_dict() interchange with torch.optim.Muon.

    Per matrix p [A, B], with g the bf16 gradient (or bf16(main_grad) of DataParallelBucket(defer_grad_cast=True),
    read in place) and m the momentum buffer, fp32 arithmetic and one bf16 rounding (nearest even) per named result,
    torch's rounding points:
      m' = bf16(lerp(m, g, 1 - momentum));  u = bf16(lerp(g, m', momentum)) if nesterov else m'
      X0 = bf16(u / max(float(bf16(||u||)), eps))                  (a true division)
      O  = ns_steps Newton-Schulz iterations on X0 (its transposed view when A > B), bf16 GEMMs
      p  = bf16(p * (1 - lr weight_decay));  p = bf16(p - lr ratio O),  ratio = torch's _adjust_lr(shape)
    One deliberate difference from torch 2.10: with nesterov=False and a bf16 gradient, torch's `.bfloat16()` is a
    no-op, so its in-place `div_` normalises the momentum buffer itself (after a step the stored buffer has norm 1).
    Here the buffer keeps m', as the documented algorithm has it.

    step(): per parameter group, over the parameters that have a gradient, pico_muon_momentum and pico_muon_normalize
    (whole list), the Newton-Schulz GEMMs per matrix (torch.mm / torch.addmm on hipBLASLt, the calls torch's Muon
    makes, into persistent buffers), then one pico_muon_update: 4 HIP launches plus 3 * ns_steps GEMM calls per
    matrix. Nothing is read on the host and nothing is allocated after the first step of a parameter set. Workspace:
    2 bytes per Muon parameter (the Newton-Schulz inputs, one [L, A, B] buffer per matrix shape, where the results
    land too) plus two ping-pong and two Gram buffers of the largest matrix. (Batching a shape's matrices into
    bmm / baddbmm calls is not in: DESIGN.md §4j.)

    Refused: parameters that are not 2-D (ValueError, at construction); a parameter tagged `_pico_tp_sharded`
    (NotImplementedError: orthogonalising a shard is not Muon); a tensor lr; at step(), before any state is touched,
    parameters or gradients that are not contiguous bf16 HIP tensors (TypeError / ValueError). Gradient clipping:
    the standalone clip_grad_norm_ in front of the step."""
    reads_deferred_grads = True  # as AdamW: the fp32 main_grad of DataParallelBucket(defer_grad_cast=True) is read in place

    def __init__(self, params, lr=1e-3, weight_decay=0.1, momentum=0.95, nesterov=True,
                 ns_coefficients=(3.4445, -4.7750, 2.0315), eps=1e-7, ns_steps=5, adjust_lr_fn=None):
        if isinstance(lr, torch.Tensor):
            raise TypeError("picotron_amd.optim.Muon: a float lr only")
        if not 0.0 <= lr:
            raise ValueError(f"Learning rate should be >= 0 but is: {lr}")
        if not 0.0 <= momentum:
            raise ValueError(f"momentum should be >= 0 but is: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"weight decay should be >= 0 but is: {weight_decay}")
        if not 0.0 <= eps:
            raise ValueError(f"eps should be >= 0 but is: {eps}")
        if adjust_lr_fn is not None and adjust_lr_fn not in ("original", "match_rms_adamw"):
            raise ValueError(f"Adjust learning rate function {adjust_lr_fn} is not supported")
        defaults = {"lr": lr, "weight_decay": weight_decay, "momentum": momentum, "nesterov": nesterov,
                    "ns_coefficients": ns_coefficients, "eps": eps, "ns_steps": ns_steps, "adjust_lr_fn": adjust_lr_fn}
        super().__init__(params, defaults)
        for group in self.param_groups:
            for p in group["params"]:
                if p.ndim != 2:
                    raise ValueError(f"Muon only supports 2D parameters whereas we found a parameter with size: "
                                     f"{p.size()}")
                if getattr(p, "_pico_tp_sharded", False):
                    raise NotImplementedError("picotron_amd.optim.Muon: a tensor-parallel shard is not a matrix to "
                                              "orthogonalise (Newton-Schulz sharded across ranks is not implemented)")
        self._tables = {}  # per (group, parameter set): the device tables and the Newton-Schulz workspace

    def _validate(self, group):
        """The group's parameters that have a gradient, everything checked before any state is touched."""
        params = [p for p in group["params"] if p.grad is not None]
        if not params:
            return params
        if isinstance(group["lr"], torch.Tensor):
            raise TypeError("picotron_amd.optim.Muon: a float lr only")
        if not 0 <= int(group["ns_steps"]) < 100:
            raise ValueError("Number of steps must be less than 100 for computational efficiency")
        if len(group["ns_coefficients"]) != 3:
            raise ValueError("Coefficients must be a tuple of exactly 3 values")
        _muon_ratio(group["adjust_lr_fn"], (1, 1))
        for p in params:
            if not (p.is_cuda and p.dtype == torch.bfloat16 and p.grad.dtype == torch.bfloat16 and p.grad.is_cuda):
                raise TypeError("picotron_amd.optim.Muon: parameters and gradients must be bf16 HIP tensors, "
                                f"got {p.dtype} / {p.grad.dtype} on {p.device}")
            if p.grad.is_sparse or not p.grad.is_contiguous() or not p.is_contiguous():
                raise ValueError("picotron_amd.optim.Muon: dense contiguous parameters and gradients only")
            if p.ndim != 2 or p.grad.shape != p.shape:
                raise ValueError("picotron_amd.optim.Muon: 2-D parameters with gradients of their shape only")
            _deferred_grad(p)
            m = self.state[p].get("momentum_buffer") if p in self.state else None
            if m is not None and (m.dtype != torch.bfloat16 or m.device != p.device or m.shape != p.shape
                                  or not m.is_contiguous()):
                raise TypeError("picotron_amd.optim.Muon: state 'momentum_buffer' must be a contiguous bf16 tensor of "
                                f"the parameter's shape and device, got {m.dtype} {tuple(m.shape)} on {m.device}")
        return params

    def _group_tables(self, gi, group, params):
        dev = params[0].device
        key = (gi, tuple((p.data_ptr(), tuple(p.shape)) for p in params), group["adjust_lr_fn"])
        ent = self._tables.get(key)
        if ent is None:
            layout = _muon_layout([p.shape for p in params], group["adjust_lr_fn"])
            ent = _new_tables([p.numel() for p in params], dev, "out")
            bufs, slices = _muon_work(layout, dev)
            flat, plan = _muon_ns_plan(layout, slices, dev)
            ent.update(layout=layout, work=bufs, slices=slices, ns_flat=flat, ns_plan=plan,
                       chunk_start=torch.tensor(layout["chunk_start"], dtype=torch.int64).to(dev),
                       ratios=torch.tensor(layout["ratios"], dtype=torch.float64).to(dev),
                       partials=torch.empty(max(ent["n_chunks"], 1), dtype=torch.float32, device=dev),
                       norms=torch.empty(len(params), dtype=torch.float32, device=dev))
            if len(self._tables) > 16:  # parameter sets keep changing: keep the map (and its workspaces) small
                self._tables.clear()
            self._tables[key] = ent
        ptrs = []
        for p, w in zip(params, ent["slices"]):
            g32 = _deferred_grad(p)
            # the orthogonalised update lands where its input was: the tensor's slice of the work buffer
            ptrs.append((p.data_ptr(), (g32 if g32 is not None else p.grad).data_ptr(),
                         self.state[p]["momentum_buffer"].data_ptr(), w.data_ptr(), 0 if g32 is None else 1,
                         w.data_ptr()))
        _sync_ptrs(ent, ptrs, dev)
        return ent

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        work = [(gi, group, self._validate(group)) for gi, group in enumerate(self.param_groups)]
        for gi, group, params in work:
            if not params:
                continue
            for p in params:
                st = self.state[p]
                if "momentum_buffer" not in st:
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            ent = self._group_tables(gi, group, params)
            stream = _lib.stream_of(params[0])
            tens, sizes, chunks, n_chunks = (_lib.ptr(ent["tens"]), _lib.ptr(ent["sizes"]), _lib.ptr(ent["chunks"]),
                                             ent["n_chunks"])
            _lib.check(lib.pico_muon_momentum(tens, sizes, chunks, n_chunks, float(group["momentum"]),
                                              1 if group["nesterov"] else 0, _lib.ptr(ent["partials"]), stream),
                       "pico_muon_momentum")
            _lib.check(lib.pico_muon_normalize(tens, sizes, chunks, n_chunks, _lib.ptr(ent["chunk_start"]),
                                               len(params), _lib.ptr(ent["partials"]), float(group["eps"]),
                                               _lib.ptr(ent["norms"]), stream), "pico_muon_normalize")
            _newton_schulz(ent["ns_plan"], group["ns_coefficients"], int(group["ns_steps"]))
            _lib.check(lib.pico_muon_update(tens, _lib.ptr(ent["out"]), sizes, chunks, n_chunks, float(group["lr"]),
                                            float(group["weight_decay"]), _lib.ptr(ent["ratios"]), stream),
                       "pico_muon_update")
        return loss
