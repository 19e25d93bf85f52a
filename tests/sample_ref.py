"""fp64 reference of the fused sampler (picotron_amd.generate.sample_tokens / pico_sample) and the rule by which a
sampled token is accepted (tests/test_sample_host.py, tests/test_sample_gpu.py). A plain helper module: no tests.

The reference works a row at a time in numpy fp64, sums in vocabulary order with sequential loops (np.cumsum), and
shares nothing with the code under test but the Philox restatement of tests/test_adamw_sr_host.py (checked there
against Random123's known answers).

The tolerance tau(V) of the acceptance rule, derived, not fitted. With z_i = (x_i - max x) / T, w_i = exp(z_i):
  * the kernel forms z in fp32 with two roundings (the difference, the quotient): |dz_i| <= |z_i| 2^-23, which
    scales w_i by exp(dz_i), a relative error of |z_i| 2^-23;
  * its fp32 exp is good to 1 ulp; 2 ulp = 2^-22 relative are budgeted;
  * it sums fixed-point masses round(w_i 2^40): an absolute error of 2^-41 each, V 2^-41 over a row.
So the mass of any subset A of the kept set is off by at most E(A) = sum_A w_i (|z_i| 2^-23 + 2^-22) + |A| 2^-41. A
normalised cumulative C = M(A) / S with S = M(kept) moves by ((1 - C) E(A) + C E(kept minus A)) / S <= E(kept) / S.
The maximum is always kept and has w = 1, so S >= 1, and with p_i = w_i / S:
  E(kept) / S <= 2^-23 sum p_i |z_i| + 2^-22 + V 2^-41,  sum p_i |z_i| = H(p) - ln S <= ln V
(z_i = ln p_i + ln S <= 0, H the entropy of p, at most ln V). Hence
  tau(V) = ln(V) 2^-23 + 2^-22 + V 2^-41,
2.4e-6 at V = 2^20, below 2^-18 = 3.8e-6 over the whole supported range. The same bound holds for the top-p
decision, whose normaliser is the mass of the top-k set (it holds the maximum too). The reference's own fp64 error
(V 2^-53) and the conversion of the 64-bit draw to fp64 (2^-53) are far below it. The top-k threshold and the ties
are exact comparisons of logits: no tolerance.
"""
import math

import numpy as np

from test_adamw_sr_host import philox4x32_10

F32_MAX = float(np.finfo(np.float32).max)


def tau(V):
    return math.log(V) * 2.0 ** -23 + 2.0 ** -22 + V * 2.0 ** -41


def canon(x):
    """A row as fp64: NaN counts as -inf, +inf as the largest finite fp32."""
    x = np.asarray(x, dtype=np.float64).copy()
    x[np.isnan(x)] = -np.inf
    return np.minimum(x, F32_MAX)


def draw_words(seed, rows, counters):
    """r = (w[1] << 32) | w[0] of philox4x32_10(counter (row, n, 0, 0), key (seed low, seed high)), as Python ints."""
    rows, counters = np.asarray(rows), np.asarray(counters)
    ctr = np.zeros((len(rows), 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1] = rows.astype(np.uint32), counters.astype(np.uint32)
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32))
    return [(int(a[1]) << 32) | int(a[0]) for a in w]


class Row:
    """The reference for one row under one setting: .keep (bool [V]), .kept (its size), .w (fp64 masses, the maximum
    at 1), .C (normalised inclusive cumulative mass of the kept set in vocabulary order), .argmax (lowest index of
    the maximum), .margin (the smallest |mass{x >= t'} / mass(K) - p| over all values t' in the top-k set, inf with
    top-p off: how far the top-p cut is from flipping), .live (some logit is finite)."""

    def __init__(self, x, temperature, top_k=None, top_p=None, order=None):
        x = canon(x)
        V = x.shape[0]
        xmax = x.max()
        self.live = bool(xmax > -np.inf)
        self.argmax = int(np.flatnonzero(x == xmax)[0])
        self.margin = math.inf
        if not self.live:
            self.keep, self.kept, self.w, self.C = np.zeros(V, dtype=bool), 0, np.zeros(V), np.zeros(V)
            return
        if not temperature > 0:
            self.keep = np.zeros(V, dtype=bool)
            self.keep[self.argmax] = True
            self.kept, self.w = 1, self.keep.astype(np.float64)
            self.C = np.cumsum(self.w)
            return
        T = float(np.float32(temperature))
        w = np.exp((x - xmax) / T)
        if order is None:
            order = np.argsort(-x)  # any order within a tie: only whole tie groups are used
        nk = V
        if top_k is not None and 0 < top_k < V:
            nk = int(np.count_nonzero(x >= x[order[top_k - 1]]))  # ties at the k-th value stay
        if top_p is not None and 0 < float(np.float32(top_p)) < 1:
            p = float(np.float32(top_p))
            xs, ws = x[order[:nk]], w[order[:nk]]
            csum = np.cumsum(ws)
            ends = np.flatnonzero(np.append(xs[1:] != xs[:-1], True))  # last position of each distinct value
            share = csum[ends] / csum[-1]  # mass{x >= value} / mass(K)
            first = int(np.argmax(share >= p)) if (share >= p).any() else len(ends) - 1
            nk = int(ends[first]) + 1
            self.margin = float(np.abs(share - p).min())
        self.keep = np.zeros(V, dtype=bool)
        self.keep[order[:nk]] = True
        self.kept, self.w = nk, w
        c = np.cumsum(np.where(self.keep, w, 0.0))
        self.C = c / c[-1]

    def acceptable(self, r, t):
        """Every token the rule accepts for the draw r, written down before any sampler is asked: the kept tokens
        from the first whose C + t exceeds u to the last whose predecessor's C - t does not."""
        if not self.live:
            return [0]
        u = r / 2.0 ** 64
        lo = int(np.searchsorted(self.C, u - t, side="right"))
        hi = int(np.searchsorted(self.C, u + t, side="right"))
        return (np.flatnonzero(self.keep[lo:hi + 1]) + lo).tolist()

    def accepts(self, tok, r, t):
        """The acceptance rule for the 64-bit draw r: tok is kept and C[previous kept] - t <= u < C[tok] + t. Greedy
        rows (and rows without a finite logit) accept their one token only."""
        tok = int(tok)
        if not self.live:
            return tok == 0
        if not 0 <= tok < len(self.keep) or not self.keep[tok]:
            return False
        u = r / 2.0 ** 64
        lo = self.C[tok - 1] if tok > 0 else 0.0
        return lo - t <= u < self.C[tok] + t
