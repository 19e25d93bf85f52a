"""Where the operands of every weight-gradient GEMM of a training step come from (picotron_amd/wgrad_operands.py),
watched from outside: a spy on ops._wgrad_paired (the operands each projection hands to its wgrad GEMM, not cloned: the
pointers are the point) and on ops.transpose_2d (a separate transpose pass), wgrad_pair's buffers and its STATS.

Model: hidden 1024, intermediate 2048, 16 heads of 64, 2 layers, vocab 512, 2 x 128 tokens (T = 256) -- the smallest at
which all three x^T producers are eligible (the RMSNorm y^T form needs 1024 or 2048 columns); eager steps, no graphs,
no DP. A wrong placement never changes a gradient (wgrad_pair.plan copies or runs a GEMM per micro-batch instead), so
values cannot catch it; pointers, strides and counts do.
"""
import pytest
import torch

from picotron_amd import ops
from picotron_amd import wgrad_pair as WP

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CFG = dict(hidden_size=1024, intermediate_size=2048, num_attention_heads=16, num_key_value_heads=16,
           num_hidden_layers=2, vocab_size=512, max_position_embeddings=128)
MB, SEQ = 2, 128
T = MB * SEQ


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    for k in ("PICO_XT_WGRAD", "PICO_WGRAD_PAIR", "PICO_SWIGLU_T", "PICO_LM_WGRAD_GROUP", "PICO_UNFUSED"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PICO_WGRAD_GROUP", "2")
    WP.begin_step()
    WP.release()
    yield
    WP.begin_step()
    WP.release()


class _Run:
    """A model of CFG (+ overrides) with zeroed .grad (so every sink is the in-place one and the LM head groups) and the
    two spies. step() runs one eager train_step of n micro-batches and returns its loss."""

    def __init__(self, monkeypatch, n, **over):
        from picotron_amd.data import SyntheticDataLoader
        from picotron_amd.model import LlamaConfig, build_llama
        self.cfg = LlamaConfig(**{**CFG, **over})
        torch.manual_seed(7)
        self.m = build_llama(self.cfg, "cuda", BF)
        with torch.no_grad():
            self.m.final_proj.weight.normal_(0, 0.02, generator=torch.Generator("cuda").manual_seed(1))
        for p in self.m.parameters():
            p.grad = torch.zeros_like(p)
        self.n = n
        self.loader = SyntheticDataLoader(MB, SEQ, n, self.cfg.vocab_size, seed=5, num_batches=n, device="cuda")
        self.name = {}
        for li, layer in enumerate(self.m.decoder_layers):
            a, mlp = layer.attention, layer.mlp
            for nm, mod in (("qkv", a.q_proj), ("out", a.out_proj), ("gu", mlp.gate_proj), ("down", mlp.down_proj)):
                self.name[id(mod.weight)] = (li, nm)
        self.calls = []  # (micro-batch, (layer, projection), dy2, x2) of every ops._wgrad_paired call
        self.transposes = []  # (shape, out given, result's data_ptr) of every ops.transpose_2d call
        wgrad, tr = ops._wgrad_paired, ops.transpose_2d

        def spy_wgrad(params, dy2, x2):
            # eager micro-batches run one after the other: 4 L calls each
            self.calls.append((len(self.calls) // (4 * self.cfg.num_hidden_layers), self.name[id(params[0])], dy2, x2))
            return wgrad(params, dy2, x2)

        def spy_tr(x, out=None):
            r = tr(x, out=out)
            self.transposes.append((tuple(x.shape), out is not None, r.data_ptr()))
            return r
        monkeypatch.setattr(ops, "_wgrad_paired", spy_wgrad)
        monkeypatch.setattr(ops, "transpose_2d", spy_tr)

    def step(self):
        from picotron_amd.train import train_step
        del self.calls[:], self.transposes[:]
        for p in self.m.parameters():
            p.grad.zero_()
        loss = train_step(self.m, self.loader, "cuda")
        torch.cuda.synchronize()
        return loss

    def activation_transposes(self):
        return [t for t in self.transposes if not t[1]]

    def per_micro_batch(self):
        """{micro-batch: {(layer, projection): (dy2, x2)}}, after checking that each projection called once."""
        L = self.cfg.num_hidden_layers
        assert len(self.calls) == 4 * L * self.n
        got = {}
        for i, key, dy2, x2 in self.calls:
            assert key not in got.setdefault(i, {}), f"micro-batch {i}: {key} twice"
            got[i][key] = (dy2, x2)
        assert sorted(got) == list(range(self.n)) and all(len(v) == 4 * L for v in got.values())
        return got


def _is_transposed_view(x2, ld):
    """x2 [T, K] is the .t() of a [K, T] tensor with unit column stride and row stride ld."""
    return x2.shape[0] == T and x2.stride() == (1, ld)


def test_placement_under_pairing(monkeypatch):
    """Groups of 2 over 3 micro-batches: every projection's x^T and dy reach its wgrad GEMM in this micro-batch's
    group slots (same pointer, x^T with row stride G T), the LM head's too (it calls plan itself: STATS and its dy
    slots), no activation is transposed by a separate pass, and the grouping counts are those of the formula of
    test_wgrad_pairs_match_unpaired."""
    G, n = 2, 3
    r = _Run(monkeypatch, n)
    r.step()  # creates the buffers
    head = WP._get(r.m.final_proj.weight)
    assert head is not None and (head.N, head.K, head.T, head.G) == (r.cfg.vocab_size, r.cfg.hidden_size, T, G)
    head.dy.zero_()
    nbuf, s0 = len(WP._BUFS), dict(WP.STATS)
    r.step()
    L = r.cfg.num_hidden_layers
    assert len(WP._BUFS) == nbuf == 4 * L + 1
    for i, projs in r.per_micro_batch().items():
        for key, (dy2, x2) in projs.items():
            li, nm = key
            layer = r.m.decoder_layers[li]
            w = {"qkv": layer.attention.q_proj, "out": layer.attention.out_proj, "gu": layer.mlp.gate_proj,
                 "down": layer.mlp.down_proj}[nm].weight
            b = WP._get(w)
            assert b is not None and (b.T, b.G) == (T, G), (i, key)
            slot = b.xt_slot(i)
            assert x2.data_ptr() == slot.data_ptr() and tuple(x2.shape) == (T, b.K), (i, key)
            assert x2.stride() == (1, G * T) == slot.t().stride(), (i, key)
            assert dy2.data_ptr() == b.dy_slot(i).data_ptr() and tuple(dy2.shape) == (T, b.N), (i, key)
    assert r.activation_transposes() == []
    d = {k: WP.STATS[k] - s0[k] for k in s0}
    L4 = 4 * L + 1
    assert d == {"deferred": sum((min(G, n - g0) - 1) * L4 for g0 in range(0, n, G)),
                 "paired": sum(L4 for g0 in range(0, n, G) if n - g0 > 1)}, d
    # the head's dlogits went into its dy slots: micro-batches 0 and 1 fill both, micro-batch 2 the first again
    for h in range(G):
        assert bool((head.dy_slot(h) != 0).any()), h


def test_byproducts_without_pairing(monkeypatch):
    """PICO_WGRAD_PAIR=0: no group buffers, and still every projection's saved input is the transposed view of a
    contiguous x^T its producer wrote -- none made by a separate transpose pass."""
    monkeypatch.setenv("PICO_WGRAD_PAIR", "0")
    r = _Run(monkeypatch, 2)
    r.step()
    assert len(WP._BUFS) == 0
    for i, projs in r.per_micro_batch().items():
        for key, (dy2, x2) in projs.items():
            assert _is_transposed_view(x2, T), (i, key, x2.stride())
    assert r.activation_transposes() == []


def test_xt_wgrad_off():
    """PICO_XT_WGRAD=0: no x^T anywhere (every wgrad in the dy^T x form on x itself, nothing transposed), no group
    buffer ever created; the loss is that of PICO_XT_WGRAD=1 bit for bit (the forward values do not depend on it) and
    every gradient within the bound test_wgrad_pairs_match_unpaired uses for a changed GEMM form and summation order."""
    from conftest import rel_l2
    n, res = 3, {}
    for mode in ("0", "1"):
        with pytest.MonkeyPatch.context() as mp:  # each run its own spies
            mp.setenv("PICO_XT_WGRAD", mode)
            r = _Run(mp, n)
            loss = r.step()
            res[mode] = (loss, {nm: p.grad.float().cpu() for nm, p in r.m.named_parameters()})
            if mode == "0":
                assert len(WP._BUFS) == 0
                for i, projs in r.per_micro_batch().items():
                    for key, (dy2, x2) in projs.items():
                        assert x2.is_contiguous() and x2.shape[0] == T, (i, key, x2.stride())
                assert r.activation_transposes() == []
            else:
                assert len(WP._BUFS) == 4 * r.cfg.num_hidden_layers + 1
    assert res["0"][0] == res["1"][0], (res["0"][0], res["1"][0])
    for nm in res["0"][1]:
        e = rel_l2(res["0"][1][nm], res["1"][1][nm])
        print(f"XT_WGRAD 0 vs 1 {nm}: rel_l2 {e:.3e}")
        assert e < 5e-3, nm


def test_ineligible_norm_producer(monkeypatch):
    """hidden 512 (the RMSNorm y^T form needs 1024 or 2048 columns), 1 layer: the norms attach no y^T, and the inputs
    of the wide projections (n_out >= 3 K: q|k|v and gate|up) are transposed by exactly one transpose pass each per
    micro-batch; out and down still read their producers' by-products."""
    n = 2
    r = _Run(monkeypatch, n, hidden_size=512, num_attention_heads=8, num_key_value_heads=8, num_hidden_layers=1)
    seen = []
    layer = r.m.decoder_layers[0]
    for norm in (layer.input_layernorm, layer.post_attention_layernorm, r.m.final_norm):
        norm.register_forward_hook(lambda mod, args, out: seen.append(out[0] if isinstance(out, tuple) else out))
    r.step()
    assert len(seen) == 3 * n and all(getattr(y, "_pico_t", None) is None for y in seen)
    tr = r.activation_transposes()
    assert sorted(t[0] for t in tr) == [(T, 512)] * (2 * n), tr
    made = {t[2] for t in tr}
    for i, projs in r.per_micro_batch().items():
        for (li, nm), (dy2, x2) in projs.items():
            assert x2.shape[0] == T and x2.stride(0) == 1, (i, nm, x2.stride())  # a transposed view, every one
            if nm in ("qkv", "gu"):
                assert x2.stride() == (1, T) and x2.data_ptr() in made, (i, nm)
                assert WP._get(layer.attention.q_proj.weight if nm == "qkv" else layer.mlp.gate_proj.weight) is None


def test_saved_input_outcomes_on_the_device():
    """wgrad_operands.saved_input beyond the host test's `not on a HIP device` branch: an attached x^T of the right
    shape is used as it is; one of another shape is ignored; without one a wide projection transposes, a narrow
    one keeps x; PICO_XT_WGRAD=0 keeps x whatever is attached."""
    from picotron_amd import wgrad_operands as WO
    x = torch.randn(1, 64, 32, device="cuda", generator=torch.Generator("cuda").manual_seed(3)).to(BF)
    x2 = x.view(64, 32)
    assert WO.saved_input(x2, 95, x) is x2  # n_out < 3 K
    t = WO.saved_input(x2, 96, x)
    assert t.stride() == (1, 64) and torch.equal(t, x2)
    WO.attach_t(x, torch.empty(32, 128, dtype=BF, device="cuda"))  # of another shape
    assert WO.saved_input(x2, 95, x) is x2
    xt = x2.t().contiguous()
    WO.attach_t(x, xt)
    for n_out in (32, 96):
        t = WO.saved_input(x2, n_out, x)
        assert t.data_ptr() == xt.data_ptr() and t.stride() == (1, 64) and tuple(t.shape) == (64, 32)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PICO_XT_WGRAD", "0")
        assert WO.saved_input(x2, 96, x) is x2
