"""AdamW(master_weights=True) without a GPU: pico_adamw_master's argument checks (status 1000 + message) and the
optimizer's state_dict / load_state_dict dtypes on CPU tensors (no compute calls: CPU only)."""
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


def test_master_entry_point_rejects_bad_arguments(lib):
    p = ctypes.c_void_p(64)
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.01)
    assert lib.pico_adamw_master(p, None, p, p, 4, *hp, 1, None, None) == 1000
    assert b"masters" in lib.pico_last_error()
    assert lib.pico_adamw_master(p, None, p, p, 4, *hp, 1, p, None) == 1000  # with a clip coefficient too
    assert b"masters" in lib.pico_last_error()
    assert lib.pico_adamw_master(None, p, p, p, 4, *hp, 1, None, None) == 1000
    assert b"null table" in lib.pico_last_error()
    assert lib.pico_adamw_master(p, p, p, p, 4, *hp, 0, None, None) == 1000
    assert b"step" in lib.pico_last_error()
    assert lib.pico_adamw_master(p, p, p, p, 4, 1e-3, 1.0, 0.999, 1e-8, 0.01, 1, None, None) == 1000
    assert b"hyper-parameters" in lib.pico_last_error()
    for n in (-1, 1 << 31):
        assert lib.pico_adamw_master(p, p, p, p, n, *hp, 1, None, None) == 1000
        assert b"chunk count" in lib.pico_last_error()
    # nothing to do: no table is looked at
    assert lib.pico_adamw_master(None, None, None, None, 0, *hp, 1, None, None) == 0


def _state_dict(opt, state):
    return {"state": {0: state}, "param_groups": opt.state_dict()["param_groups"]}


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def test_load_state_dict_keeps_fp32_state():
    from picotron_amd.optim import AdamW
    p = torch.nn.Parameter(torch.ones(8, dtype=BF))
    opt = AdamW([p], master_weights=True)
    assert opt.master_weights is True
    vals = {"exp_avg": torch.full((8,), 1.00001), "exp_avg_sq": torch.full((8,), 3.00001e-7),
            "master_param": torch.linspace(1.00001, 1.00002, 8)}
    for v in vals.values():  # not representable in bf16: a cast to the parameter's dtype would show
        assert v.dtype == torch.float32 and not torch.equal(v.to(BF).float(), v)
    opt.load_state_dict(_state_dict(opt, {"step": torch.tensor(3.0), **{k: v.clone() for k, v in vals.items()}}))
    st = opt.state[p]
    for k, v in vals.items():
        assert st[k].dtype == torch.float32, k
        assert torch.equal(_bits(st[k]), _bits(v)), k
    assert float(st["step"]) == 3.0
    # own copies: stepping the loaded optimizer must not write into the dict it was loaded from
    src = {"step": torch.tensor(3.0), **{k: v.clone() for k, v in vals.items()}}
    opt.load_state_dict(_state_dict(opt, src))
    assert all(opt.state[p][k].data_ptr() != src[k].data_ptr() for k in vals)
    assert opt.state[p]["step"] is not src["step"] and float(opt.state[p]["step"]) == 3.0
    # and out again as fp32
    out = opt.state_dict()["state"][0]
    assert all(out[k].dtype == torch.float32 and torch.equal(_bits(out[k]), _bits(vals[k])) for k in vals)


def test_load_bf16_form_checkpoint_into_master_mode():
    from picotron_amd.optim import AdamW
    p = torch.nn.Parameter(torch.ones(8, dtype=BF))
    opt = AdamW([p], master_weights=True)
    m = torch.linspace(-1.0, 1.0, 8).to(BF)
    v = torch.linspace(1e-8, 1e-2, 8).to(BF)
    opt.load_state_dict(_state_dict(opt, {"step": torch.tensor(5.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}))
    st = opt.state[p]
    assert st["exp_avg"].dtype == torch.float32 and torch.equal(st["exp_avg"], m.float())
    assert st["exp_avg_sq"].dtype == torch.float32 and torch.equal(st["exp_avg_sq"], v.float())
    assert "master_param" not in st  # created from the parameter at the next step
    assert float(st["step"]) == 5.0


def test_bf16_mode_is_unchanged():
    """Without master_weights: the defaults state_dict() reports are torch.optim.AdamW's keys (no new one), and
    load_state_dict casts to the parameter's dtype as torch does."""
    from picotron_amd.optim import AdamW
    p = torch.nn.Parameter(torch.ones(8, dtype=BF))
    opt = AdamW([p])
    assert opt.master_weights is False
    ref = torch.optim.AdamW([torch.nn.Parameter(torch.ones(8, dtype=BF))])
    (g,), (gr,) = opt.state_dict()["param_groups"], ref.state_dict()["param_groups"]
    assert set(g) <= set(gr) and "master_weights" not in g
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-8, 1e-2)
    assert AdamW([p], master_weights=True).state_dict()["param_groups"] == opt.state_dict()["param_groups"]
    opt.load_state_dict(_state_dict(opt, {"step": torch.tensor(1.0), "exp_avg": torch.full((8,), 1.00001),
                                          "exp_avg_sq": torch.full((8,), 1.00001)}))
    assert opt.state[p]["exp_avg"].dtype == BF and opt.state[p]["exp_avg_sq"].dtype == BF


def test_sync_master_params_on_cpu_state():
    """sync_master_params re-reads existing masters in place (same storage: the device tables stay valid) and is a
    no-op where there is none."""
    from picotron_amd.optim import AdamW
    p = torch.nn.Parameter(torch.ones(8, dtype=BF))
    opt = AdamW([p], master_weights=True)
    opt.sync_master_params()  # no state yet
    assert not opt.state[p]
    opt.load_state_dict(_state_dict(opt, {"step": torch.tensor(1.0), "exp_avg": torch.zeros(8),
                                          "exp_avg_sq": torch.zeros(8), "master_param": torch.full((8,), 1.00001)}))
    master = opt.state[p]["master_param"]
    with torch.no_grad():
        p.fill_(0.5)
    opt.sync_master_params()
    assert opt.state[p]["master_param"] is master and torch.equal(master, torch.full((8,), 0.5))
    AdamW([p]).sync_master_params()  # bf16 mode: nothing to do
