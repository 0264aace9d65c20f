"""On-device fidelity evaluator: precision / recall / density / coverage of a decoded table against the real one.

Did the generator collapse onto part of the data, and are its rows on the data manifold at all?  Marginals, pairwise
dependencies and the distance to the closest record do not say: a generator that emits one class only, with perfect
marginals inside it, scores well on all three.  The k-nearest-neighbour manifold metrics of Naeem et al., *Reliable
Fidelity and Diversity Metrics for Generative Models* (ICML 2020), do.  Precision and density measure fidelity (are
the generated rows inside the real manifold), recall and coverage measure diversity (is every real mode reached).

The metric (the contract)
-------------------------
Rows and ``d2(q, r)`` are exactly :class:`fed_tgan_amd.eval.privacy.DevicePrivacy`'s: the space of the decoded table,
continuous columns min-max scaled by the real table, and

    d2(q, r) = sum over continuous columns of (q_c - r_c)^2, in column order
               + number of categorical columns whose codes differ

in float64 from direct differences.  With real rows ``X_i`` (i < M), generated rows ``Y_j`` (j < N) and an integer k
(default 5, ``1 <= k <= FID_MAX_K = 8``):

* ``rr[i]``   = the k-th smallest ``d2(X_i, X_a)`` over ``a != i``, with multiplicity; computed once at construction;
* ``ff[j]``   = the same among the generated rows; ``+inf`` where there are fewer than k other rows;
* ``cntA[j]  = #{i : d2(Y_j, X_i) <= rr[i]}``;
* ``cntB[i]  = #{j : d2(X_i, Y_j) <= ff[j]}``;
* ``dminB[i] = min_j d2(X_i, Y_j)``;

* ``precision = #{j : cntA[j] > 0} / N``
* ``density   = (sum_j cntA[j]) / (k N)``
* ``recall    = #{i : cntB[i] > 0} / M``
* ``coverage  = #{i : dminB[i] <= rr[i]} / M``

Every count is an integer sum (int64) and each score one float64 division.  A NaN distance is inside no ball and is
never a minimum; ``<=`` is inclusive.  A high precision with a low recall / coverage is the signature of a generator
that stays on the manifold but reaches only part of it (mode collapse); a low precision says its rows are off the
manifold, whatever their marginals.

Baseline: ``precision_rr``, ``recall_rr``, ``density_rr``, ``coverage_rr`` are the same four scores with the real
rows of even index as the real table and the rows of odd index as the table scored (both as the whole real table
scales them), computed once at construction over buffers of their own.  They are what a perfect generator would
score *at half the table's size*: radii grow as a table shrinks, so they are a yardstick, not a ceiling.  They are
NaN with ``baseline=False`` or when the even half has fewer than k + 1 rows.

A real table with fewer than k + 1 rows is refused, and so is k outside ``1..FID_MAX_K``; date tables and real values
that are not finite are refused as ``DevicePrivacy`` refuses them.

``score(values)`` is a fixed launch sequence -- ``ops.nn_pack`` -> ``nn_topk`` (the generated rows against
themselves) -> ``nn_ball`` (generated queries, real balls) -> ``nn_ball`` (real queries, generated balls) ->
``prdc_reduce`` -- over buffers allocated at construction, without allocation or host round trip, so it can be
captured in a hipGraph (``graph=True``).  The ops come from :class:`fed_tgan_amd.ops.hip.HipOps`
(kernels/fidelity.hip) on a GPU and from :class:`fed_tgan_amd.ops.ref.TorchOps` elsewhere; the second is the first's
oracle.  All distances of the HIP pass come from one device function, so a distance of one launch and a radius of
another compare exactly: a generated copy of a real row lies on the boundary of every ball that row defines.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from .base import DeviceEvaluator, coded_table, column_slots

NN_CONT, NN_CAT = 0, 1
FID_MAX_K = 8
KEYS = ("precision", "recall", "density", "coverage", "precision_rr", "recall_rr", "density_rr", "coverage_rr")


class FidelityScores:
    """Scores of one table: ``buf`` = [precision, recall, density, coverage, and the four ``_rr`` baselines] on the
    device.  Nothing here synchronises except :meth:`floats`."""

    def __init__(self, buf: torch.Tensor, cnt_a: torch.Tensor, cnt_b: torch.Tensor, dmin_b: torch.Tensor,
                 rr: torch.Tensor):
        self.buf = buf
        self._cnt_a, self._cnt_b, self._dmin_b, self._rr = cnt_a, cnt_b, dmin_b, rr

    def floats(self) -> Dict[str, float]:
        return {k: float(v) for k, v in zip(KEYS, self.buf.cpu().tolist())}

    def rows(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """per generated row (the number of real balls it is inside: int32 [n], inside any: bool [n])"""
        return self._cnt_a, self._cnt_a > 0

    def real_rows(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """per real row (covered: a generated row lies in its ball, bool [M]; recalled: it lies in a generated row's
        ball, bool [M]) -- the real rows, that is the modes, the generator never reaches are those with False"""
        return self._dmin_b <= self._rr, self._cnt_b > 0


class DeviceFidelity(DeviceEvaluator):
    def __init__(self, real, meta: dict, vocabs: Sequence, device, ops=None, k: int = 5, max_rows: int = 40000,
                 baseline: bool = True, graph: bool = False):
        """real: the real table as a DataFrame, or already coded as a float64 [m, n_cols] array."""
        super().__init__(meta, device, ops, max_rows, graph)
        ops = self.ops
        self.k = k = int(k)
        if not 1 <= k <= FID_MAX_K:
            raise ValueError(f"{self.who}: k must be in 1..{FID_MAX_K}, got {k}")
        kind = [NN_CAT if cat else NN_CONT for cat in self.is_cat]
        slot, count = column_slots(kind)
        self.n_cat, self.n_cont = n_cat, n_cont = count.get(NN_CAT, 0), count.get(NN_CONT, 0)
        coded = coded_table(real, meta, vocabs, self.who, finite="array")
        m = coded.shape[0]
        if m < k + 1:
            raise ValueError(f"{self.who}: the real table has {m} rows; k = {k} needs at least {k + 1}")
        self.n_real = m
        dev = self.device
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        self.kind = torch.tensor(kind, **i32)
        self.slot = torch.tensor(slot, **i32)
        table = torch.from_numpy(np.ascontiguousarray(coded)).to(dev)
        cont_cols = torch.tensor([j for j, c in enumerate(kind) if c == NN_CONT], dtype=torch.long, device=dev)
        # MinMax on real, as DevicePrivacy scales: lo and 1 / (hi - lo) of the real columns (1 for a constant column)
        rc = table[:, cont_cols]
        self.lo = rc.min(dim=0).values.contiguous() if n_cont else torch.zeros(0, **f64)
        hi = rc.max(dim=0).values if n_cont else torch.zeros(0, **f64)
        span = hi - self.lo
        self.scale = torch.where(span > 0, 1.0 / torch.where(span > 0, span, torch.ones_like(span)),
                                 torch.ones_like(span)).contiguous()
        self.r_cont = torch.zeros(m, n_cont, **f64)
        self.r_cat = torch.zeros(m, n_cat, **i32)
        ops.nn_pack(table, self.kind, self.slot, self.lo, self.scale, self.r_cont, self.r_cat)
        self.rr = self._radii(self.r_cont, self.r_cat)
        self.scores = torch.zeros(len(KEYS), **f64)
        self.scores[4:] = float("nan")
        m_even, m_odd = (m + 1) // 2, m // 2
        if baseline and m_even >= k + 1:    # the odd rows against the even ones, once, over buffers of their own
            e_cont, e_cat = self.r_cont[0::2].contiguous(), self.r_cat[0::2].contiguous()
            self._alloc(m_odd, m_even)
            self.q_cont.copy_(self.r_cont[1::2])
            self.q_cat.copy_(self.r_cat[1::2])
            self._pass(e_cont, e_cat, self._radii(e_cont, e_cat), m_odd)
            self.scores[4:8] = self.scores[0:4]
            self.scores[:4] = 0.0
        self._alloc(self.max_rows, m)

    def _radii(self, cont: torch.Tensor, cat: torch.Tensor) -> torch.Tensor:
        """the squared distance of every row of a packed table to its k-th nearest other row"""
        rows = cont.shape[0]
        out = torch.zeros(rows, dtype=torch.float64, device=self.device)
        scratch = torch.zeros(self.ops.nn_topk_scratch(rows, rows, self.k), dtype=torch.float64, device=self.device)
        self.ops.nn_topk(cont, cat, cont, cat, True, self.k, out, scratch)
        return out

    def _alloc(self, rows: int, m: int) -> None:
        """buffers of a pass of up to ``rows`` generated rows against ``m`` real ones"""
        ops, dev = self.ops, self.device
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.q_cont = torch.zeros(rows, self.n_cont, **f64)
        self.q_cat = torch.zeros(rows, self.n_cat, **i32)
        self.ff = torch.zeros(rows, **f64)
        self.cnt_a = torch.zeros(rows, **i32)
        self.dmin_a = torch.zeros(rows, **f64)
        self.cnt_b = torch.zeros(m, **i32)
        self.dmin_b = torch.zeros(m, **f64)
        need = max(ops.nn_topk_scratch(rows, rows, self.k), ops.nn_ball_scratch(rows, m), ops.nn_ball_scratch(m, rows))
        self.scratch = torch.zeros(need, **f64)

    # ------------------------------------------------------------------ the pass
    def _pass(self, r_cont: torch.Tensor, r_cat: torch.Tensor, rr: torch.Tensor, n: int) -> None:
        ops, k = self.ops, self.k
        q_cont, q_cat, ff = self.q_cont[:n], self.q_cat[:n], self.ff[:n]
        ops.nn_topk(q_cont, q_cat, q_cont, q_cat, True, k, ff, self.scratch)
        ops.nn_ball(q_cont, q_cat, r_cont, r_cat, rr, self.cnt_a, self.dmin_a, self.scratch)
        ops.nn_ball(r_cont, r_cat, q_cont, q_cat, ff, self.cnt_b, self.dmin_b, self.scratch)
        ops.prdc_reduce(self.cnt_a, self.cnt_b, self.dmin_b, rr, n, r_cont.shape[0], k, self.scores)

    def _launch(self, values: torch.Tensor, n: int) -> None:
        self.ops.nn_pack(values, self.kind, self.slot, self.lo, self.scale, self.q_cont, self.q_cat)
        self._pass(self.r_cont, self.r_cat, self.rr, n)

    def _result(self, n: int) -> FidelityScores:
        return FidelityScores(self.scores.clone(), self.cnt_a[:n].clone(), self.cnt_b.clone(), self.dmin_b.clone(),
                              self.rr)

    def score(self, values: torch.Tensor) -> FidelityScores:
        """values: [n, n_cols] float64 on the evaluator's device, as ``generate_decoded`` returns them (finite
        values are a precondition).  The work is queued on the current stream; the returned scores are device
        tensors and nothing waits for them."""
        return super().score(values)
