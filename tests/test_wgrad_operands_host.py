"""picotron_amd/wgrad_operands.py, the one placement rule for the operands of a weight-gradient GEMM, on CPU tensors
(wgrad_pair is plain host logic): one test per row of the rule's behaviour table, a projection W [N, K] = [24, 16],
T = 8 tokens per micro-batch, groups of G = 2. A returned tensor is compared with wgrad_pair's own slot of the same
micro-batch by data_ptr, shape and stride; len(wgrad_pair._BUFS) shows that nothing was created where nothing should be.
"""
import pathlib
import re

import pytest
import torch

from picotron_amd import wgrad_operands as WO
from picotron_amd import wgrad_pair as WP

N, K, T, G = 24, 16, 8, 2
F32, CPU = torch.float32, torch.device("cpu")


@pytest.fixture
def proj(monkeypatch):
    monkeypatch.setenv("PICO_WGRAD_GROUP", str(G))
    monkeypatch.delenv("PICO_XT_WGRAD", raising=False)
    monkeypatch.delenv("PICO_WGRAD_PAIR", raising=False)
    WP.begin_step()
    WP.release()
    yield WO.Proj.of(torch.nn.Parameter(torch.zeros(N, K)))
    WP.begin_step()
    WP.release()


def _same(a, b):
    return a is not None and (a.data_ptr(), tuple(a.shape), a.stride()) == (b.data_ptr(), tuple(b.shape), b.stride())


def _fresh_xt(t):
    return t is not None and tuple(t.shape) == (K, T) and t.stride() == (T, 1) and t.dtype == F32


LIKE = torch.zeros(1)


def test_proj_is_a_tuple_of_weight_n_k():
    wq, wk = torch.zeros(24, 16), torch.zeros(8, 16)
    p = WO.Proj.of(wq, wk)
    w, n, k = p
    assert w is wq and (n, k) == (32, 16) and (p.weight, p.N, p.K) == (w, n, k)
    assert WO.Proj.of(wk) == (wk, 8, 16)


def test_xt_off_writes_nothing_and_creates_nothing(monkeypatch, proj):
    monkeypatch.setenv("PICO_XT_WGRAD", "0")
    assert not WO.xt_enabled()
    x2 = torch.zeros(T, K)
    with WP.micro_batch(0, 3):
        assert WO.xt_sink(proj, K, T, LIKE) is None
        assert WO.xt_sink(None, K, T, LIKE) is None
        out = WO.attach_t(torch.zeros(T, K), None)
        assert not hasattr(out, "_pico_t") and WO.transposed_of(out, T, K) is None
        assert WO.saved_input(x2, 3 * K, out) is x2
        assert WO.dy_sink_of_output(proj, T, N, LIKE) is None
        assert WO.dy_sink_of_input(proj.weight, x2, N, K, T, LIKE) is None
    assert len(WP._BUFS) == 0


@pytest.mark.parametrize("how", ["outside", "PICO_WGRAD_PAIR=0"])
def test_pairing_inactive_gives_a_fresh_xt_and_no_dy_sink(monkeypatch, proj, how):
    if how == "outside":
        got = WO.xt_sink(proj, K, T, LIKE), WO.dy_sink_of_output(proj, T, N, LIKE)
        dyi = WO.dy_sink_of_input(proj.weight, got[0].t(), N, K, T, LIKE)
    else:
        monkeypatch.setenv("PICO_WGRAD_PAIR", "0")
        with WP.micro_batch(0, 3):
            assert not WP.active()
            got = WO.xt_sink(proj, K, T, LIKE), WO.dy_sink_of_output(proj, T, N, LIKE)
            dyi = WO.dy_sink_of_input(proj.weight, got[0].t(), N, K, T, LIKE)
    assert _fresh_xt(got[0]) and got[1] is None and dyi is None
    assert len(WP._BUFS) == 0


def test_pairing_active_but_no_match_gives_a_fresh_xt(proj):
    with WP.micro_batch(0, 3):
        assert _fresh_xt(WO.xt_sink(WO.Proj(proj.weight, N, K + 8), K, T, LIKE))  # reader.K != K
        t = WO.xt_sink(proj, K, T + 4, LIKE)  # T % 8 != 0
        assert tuple(t.shape) == (K, T + 4) and t.is_contiguous()
        assert _fresh_xt(WO.xt_sink(None, K, T, LIKE))  # no reader
    assert len(WP._BUFS) == 0


def test_pairing_active_and_matching_gives_the_slot_views(proj):
    w = proj.weight
    for hint in (proj, tuple(proj)):  # a bare (weight, N, K) is accepted too
        for i in range(3):
            with WP.micro_batch(i, 3):
                xt = WO.xt_sink(hint, K, T, LIKE)
                b = WP._get(w)
                assert _same(xt, WP.xt_out(w, N, K, T, F32, CPU)) and _same(xt, b.xt_slot(i))
                assert xt.stride() == (G * T, 1)
                assert xt.data_ptr() == b.xt[(i // G) % 2][:, (i % G) * T:].data_ptr()
                want = WP.dy_out(w, N, K, T, F32, CPU)
                assert _same(WO.dy_sink_of_input(w, xt.t(), N, K, T, LIKE), want)
                assert _same(WO.dy_sink_of_output(hint, T, N, LIKE), want) and _same(want, b.dy_slot(i))
                assert WP._get(w) is b and len(WP._BUFS) == 1
                # and these are the operands plan() takes in place: no copy, the first of a group defers
                before = dict(WP.STATS)
                kind = WP.plan(w, want, xt.t())[0]
                assert kind == ("skip" if i == 0 else "gemm")
                assert WP.STATS["deferred"] - before["deferred"] == (1 if i == 0 else 0)
        WP.begin_step()


def test_norm_backward_never_creates_buffers(proj):
    w = proj.weight
    with WP.micro_batch(1, 3):
        assert WO.dy_sink_of_output(proj, T, N, LIKE) is None  # the writer's buffers are missing
        assert WO.dy_sink_of_output(None, T, N, LIKE) is None
        assert len(WP._BUFS) == 0
        WO.xt_sink(proj, K, T, LIKE)
        b = WP._get(w)
        assert _same(WO.dy_sink_of_output(proj, T, N, LIKE), b.dy_slot(1))
        assert WO.dy_sink_of_output(proj, 2 * T, N, LIKE) is None  # buffers of another shape
        assert WO.dy_sink_of_output(proj, T, N, torch.zeros(1, dtype=torch.bfloat16)) is None  # or dtype
        assert WO.dy_sink_of_output(proj, T, N + 8, LIKE) is None  # writer.N != N
        assert WO.dy_sink_of_output(WO.Proj(w, N + 8, K), T, N + 8, LIKE) is None
        assert WP._get(w) is b and len(WP._BUFS) == 1


def test_projection_backward_needs_its_saved_x_in_the_slot(proj):
    w = proj.weight
    with WP.micro_batch(0, 3):
        mine = WO.xt_sink(proj, K, T, LIKE)
    with WP.micro_batch(1, 3):
        b = WP._get(w)
        assert WO.dy_sink_of_input(w, torch.zeros(K, T).t(), N, K, T, LIKE) is None  # a fresh x^T
        assert WO.dy_sink_of_input(w, torch.zeros(T, K), N, K, T, LIKE) is None  # x itself
        assert WO.dy_sink_of_input(w, mine.t(), N, K, T, LIKE) is None  # another micro-batch's slot
        assert WO.dy_sink_of_input(w, b.xt_slot(1).t(), N, K, 2 * T, LIKE) is None  # another shape
        assert WO.dy_sink_of_input(torch.nn.Parameter(torch.zeros(N, K)), b.xt_slot(1).t(), N, K, T, LIKE) is None
        assert _same(WO.dy_sink_of_input(w, b.xt_slot(1).t(), N, K, T, LIKE), b.dy_slot(1))
        assert WP._get(w) is b and len(WP._BUFS) == 1


def test_ineligible_producer_writes_no_xt(proj):
    x2 = torch.zeros(T, K)
    with WP.micro_batch(0, 3):
        assert WO.xt_sink(proj, K, T, LIKE, eligible=False) is None
        assert WO.saved_input(x2, 3 * K, x2) is x2
    assert WO.xt_sink(proj, K, T, LIKE, eligible=False) is None
    assert len(WP._BUFS) == 0


def test_attached_transpose_and_saved_input_on_host_tensors(proj):
    x = torch.arange(T * K, dtype=F32).view(1, T, K)
    xt = x.view(T, K).t().contiguous()
    assert WO.attach_t(x, xt) is x and x._pico_t is xt
    assert WO.transposed_of(x, T, K) is xt
    assert WO.transposed_of(x, K, T) is None and WO.transposed_of(x, T, K + 1) is None  # of another shape
    assert WO.transposed_of(None, T, K) is None and WO.transposed_of(torch.zeros(T, K), T, K) is None
    # a tensor that is not on a HIP device is kept as it is, whatever is attached and however wide the output
    x2 = x.view(T, K)
    for n_out in (K, 3 * K):
        assert WO.saved_input(x2, n_out, x) is x2 and WO.saved_input(x2, n_out) is x2


def test_one_reader_of_the_switch_and_one_owner_of_the_attribute():
    root = pathlib.Path(WO.__file__).parent
    src = {p.relative_to(root).as_posix(): p.read_text() for p in root.rglob("*.py")}
    assert [n for n, s in src.items() if "PICO_XT_WGRAD" in s] == ["wgrad_operands.py"]
    assert [n for n, s in src.items() if re.search(r"_pico_t\b", s)] == ["wgrad_operands.py"]
    assert not [n for n, s in src.items() if re.search(r"\b_pair_xt\b|\b_pair_dy\b|\b_wgrad_input\b", s)]
