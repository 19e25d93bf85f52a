"""bench.py's host-side arithmetic (CPU): the all-reduce exposure model the N > 1 line reports."""
import importlib.util
import os

import pytest

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_fixed_sample(tmp_path):
    """--dump-outputs' writer on a CPU module: small tensors whole, large ones at the same seeded indices in every
    call, float32 weights and gradients beside the float64 losses, a missing gradient left out."""
    import numpy as np
    import torch
    b = _bench()
    m = torch.nn.Module()
    m.small = torch.nn.Parameter(torch.arange(12.0).reshape(3, 4).bfloat16())
    m.big = torch.nn.Parameter(torch.arange(float(4 * b.DUMP_ELEMS)).reshape(4, -1))
    m.nograd = torch.nn.Parameter(torch.ones(5))
    m.small.grad = torch.full_like(m.small, 0.5)
    m.big.grad = -m.big.detach()
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), [2.5, 1.25], m)
    got = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["grad.big.npy", "grad.small.npy", "loss.npy", "param.big.npy", "param.nograd.npy",
                           "param.small.npy"]
    assert got["loss.npy"].dtype == np.float64 and got["loss.npy"].tolist() == [2.5, 1.25]
    assert all(a.dtype == np.float32 for f, a in got.items() if f != "loss.npy")
    assert got["param.small.npy"].tolist() == list(range(12)) and (got["grad.small.npy"] == 0.5).all()
    big = got["param.big.npy"]
    assert big.shape == (b.DUMP_ELEMS,) and len(np.unique(big)) > b.DUMP_ELEMS // 2  # a spread sample, not a prefix
    assert big.max() > 3 * b.DUMP_ELEMS and (got["grad.big.npy"] == -big).all()  # same indices for weight and gradient
    for f, a in got.items():
        assert (np.load(tmp_path / "b" / f) == a).all(), f


def test_exposure_model_serialises_buckets():
    b = _bench()
    # two 1 GB buckets at W = 2 (wire bytes = bytes): 1 GB at 100 GB/s = 10 ms each
    bk = [(-30.0, 1e9), (-5.0, 1e9)]
    # first: -30 -> -20; second starts at max(-5, -20) = -5 -> +5 ms exposed
    assert b.exposure_model(bk, 2, 100.0) == pytest.approx(5.0)
    # ready long before the end and fast links: nothing exposed
    assert b.exposure_model(bk, 2, 1000.0) == 0.0
    # a late first bucket delays the second (serialised on one stream)
    assert b.exposure_model([(-1.0, 1e9), (-0.5, 1e9)], 2, 100.0) == pytest.approx(19.0)
    # W = 8: 2 * 7 / 8 of the bytes on the wire
    assert b.exposure_model([(0.0, 8e9)], 8, 1000.0) == pytest.approx(14.0)
    assert b.exposure_model([], 8, 300.0) == 0.0
