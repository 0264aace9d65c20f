"""On-device ML-utility evaluator: train on the generated table, test on real rows (TSTR), and report the gap to the
same classifier trained on the real training rows.

Avg_JSD / Avg_WD, DCR / NNDR and Diff. Corr. compare the tables; this evaluator asks whether a model fitted on the
generated rows classifies held-out real rows.  The classifier is a class-balanced, L2-regularised multinomial logistic
regression; the reference's decision tree and random forest are ``eval/forest_device.py``, its MLP
``eval/mlp_device.py``.
Rows live in the space of the decoded table (``generate_decoded``'s ``[n, n_cols]`` float64: label codes in the
categorical columns, log1p values in the ``non_negative_cols``); the real tables are brought there with
:func:`fed_tgan_amd.eval.privacy.code_real_table`.

**Target.**  ``meta["target"]`` (or ``target=``), a categorical column with ``K`` categories (``K`` and every
``K_c`` below by the rule of :class:`DeviceCorrelation`: ``max(len(vocab), 1 + largest real code)``).  A training
row whose target is NaN or no code of ``[0, K)`` gets weight 0; such a test row is skipped.

**Features.**  Every other column.  A continuous column is ``(v - mean) / sd`` with the mean and the population sd
of the pooled real table (train and test), an sd of 0 taken as 1.  A categorical column with ``K_c`` categories is a
one-hot block of ``K_c + 1`` columns, the last for values that are no code.  A constant 1 comes last.  ``D = n_cont +
sum(K_c + 1) + 1``; the weights ``W`` are ``[D, K]`` float64 and start at 0.  The one-hot blocks never exist in memory.

**Sample weights.**  ``s_i = n_valid / (K_present count[y_i])``; classes absent from the training table have
probability 0, keep a zero weight column and are never predicted (with no class present, class 0 is).  ``S`` is the
sum of ``s`` (taken as 1 when no row is valid).

**Objective.**  ``f(W) = (sum_i s_i CE(softmax(F_i W), y_i) + |W without the intercept row|^2 / 2) / S``, the
objective of sklearn's ``LogisticRegression(C=1, class_weight="balanced")``.

**Solver.**  ``M = (F^T diag(s) F / 2 + diag(reg)) / S`` with ``reg`` 1 but 0 for the intercept, plus ``1e-10
trace(M) / D`` on the diagonal: Boehning's bound of the Hessian.  ``M^-1`` comes once per fit from the Cholesky
factor.  With ``V_0 = W_0 = 0`` and ``t_0 = 1``, ``iters`` times: ``W_{k+1} = V_k - M^-1 grad f(V_k)``, ``t_{k+1} = (1
+ sqrt(1 + 4 t_k^2)) / 2``, ``V_{k+1} = W_{k+1} + (t_k - 1) / t_{k+1} (W_{k+1} - W_k)``.  The softmax subtracts the
row maximum over the present classes.

**Scores** (``KEYS``).  The prediction is the largest logit over the present classes, the lowest class on a tie; the
confusion matrix is int32 ``[K, K]`` over the test rows; ``acc`` the accuracy and ``f1`` the support-weighted mean of
the per-class F1 (0 for a class with ``2 tp + fp + fn == 0``).  ``*_real`` come from the same fit on the real training
rows, done once at construction; a gap is real - fake; ``loss_fake = f(W_iters)`` and ``grad_fake = max |grad
f(W_iters)|`` say how far the fit got.

``score(values)`` is a fixed single-stream launch sequence (``ops.util_pack`` -> ``util_gram`` -> ``util_factor`` ->
``iters`` x ``util_step`` -> ``util_grad`` -> ``util_predict``) over buffers allocated at construction, without
allocation or host round trip, so it can be captured in a hipGraph (``graph=True``).  The ops come from
:class:`fed_tgan_amd.ops.hip.HipOps` (kernels/utility.hip) on a GPU and from :class:`fed_tgan_amd.ops.ref.TorchOps`
elsewhere; the second is the first's oracle.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .base import TstrEvaluator, column_slots, most_categories

UTIL_CONT, UTIL_CAT, UTIL_TARGET = 0, 1, 2
KEYS = ("f1_fake", "acc_fake", "f1_real", "acc_real", "f1_gap", "acc_gap", "loss_fake", "grad_fake")


def momentum_table(iters: int) -> List[float]:
    """beta_k = (t_k - 1) / t_{k+1} for k = 0 .. iters - 1, with t_0 = 1"""
    out, t = [], 1.0
    for _ in range(int(iters)):
        t1 = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out.append((t - 1.0) / t1)
        t = t1
    return out


class UtilityTable:
    """The packed form of a table of up to ``rows`` rows (``ops.util_pack`` fills it)."""

    def __init__(self, rows: int, n_cont: int, card: torch.Tensor, offs: torch.Tensor, D: int, K: int, device):
        f64 = dict(dtype=torch.float64, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.cont = torch.zeros(rows, n_cont, **f64)
        self.cat_t = torch.zeros(int(card.numel()), rows, **i32)
        self.y = torch.zeros(rows, **i32)
        self.s = torch.zeros(rows, **f64)
        self.counts = torch.zeros(K, **i32)
        self.info = torch.zeros(4, **f64)
        self.card, self.offs, self.D, self.K = card, offs, int(D), int(K)


class UtilityScores:
    """Scores of one table: ``buf`` = the eight numbers of ``KEYS`` on the device.  Nothing here synchronises except
    :meth:`floats`."""

    def __init__(self, buf: torch.Tensor, conf: torch.Tensor, W: torch.Tensor):
        self.buf = buf
        self._conf = conf
        self._W = W

    def floats(self) -> Dict[str, float]:
        return {k: float(v) for k, v in zip(KEYS, self.buf.cpu().tolist())}

    def confusion(self) -> torch.Tensor:
        """int32 [K, K] on the device: test rows by (real class, predicted class)"""
        return self._conf

    def weights(self) -> torch.Tensor:
        """W [D, K] float64 on the device, the fit on the generated table"""
        return self._W


class PackedFeatures:
    """What the evaluators that train on the packed feature table share (a mixin of a :class:`TstrEvaluator`): the
    columns' ``kind`` / ``slot``, the one-hot blocks' ``card`` / ``offs``, the standardisation ``mean`` / ``sd``, ``D``
    and its limits, and the table's allocation and packing."""

    def _setup_features(self, pooled: np.ndarray, card_of: Dict[int, int]) -> None:
        ops = self.ops
        kind = [UTIL_TARGET if name == self.target else UTIL_CAT if cat else UTIL_CONT
                for name, cat in zip(self.names, self.is_cat)]
        slot, count = column_slots(kind)
        n_cont = count.get(UTIL_CONT, 0)
        card = [card_of[j] for j, k in enumerate(kind) if k == UTIL_CAT]
        feat_names = [self.names[j] for j, k in enumerate(kind) if k == UTIL_CAT]
        self.kinds, self.n_cont, self.n_cat, self.card_list = kind, n_cont, len(card), card
        offs = [0]
        for Kc in card:
            offs.append(offs[-1] + Kc + 1)
        self.D = n_cont + offs[-1] + 1
        if self.D > int(ops.UTIL_MAX_FEATURES) or self.K > int(ops.UTIL_MAX_CLASSES):
            raise ValueError(
                f"{self.who}: {self.D} feature columns and {self.K} classes of the target {self.target!r}; the "
                f"limits are UTIL_MAX_FEATURES = {int(ops.UTIL_MAX_FEATURES)} and UTIL_MAX_CLASSES = "
                f"{int(ops.UTIL_MAX_CLASSES)}; " + most_categories(feat_names, card))
        cont_cols = [j for j, k in enumerate(kind) if k == UTIL_CONT]
        mean = pooled[:, cont_cols].mean(axis=0) if cont_cols else np.zeros(0)
        sd = pooled[:, cont_cols].std(axis=0) if cont_cols else np.zeros(0)
        sd = np.where(sd > 0, sd, 1.0)
        i32 = dict(dtype=torch.int32, device=self.device)
        f64 = dict(dtype=torch.float64, device=self.device)
        self.kind = torch.tensor(kind, **i32)
        self.slot = torch.tensor(slot, **i32)
        self.card = torch.tensor(card, **i32)
        self.offs = torch.tensor(offs, **i32)
        self.mean = torch.tensor(mean, **f64)
        self.sd = torch.tensor(sd, **f64)

    def _table(self, rows: int) -> UtilityTable:
        return UtilityTable(rows, self.n_cont, self.card, self.offs, self.D, self.K, self.device)

    def _pack(self, values: torch.Tensor, table: UtilityTable) -> None:
        self.ops.util_pack(values, self.kind, self.slot, self.mean, self.sd, table)


class DeviceUtility(PackedFeatures, TstrEvaluator):
    LIMITS = "max_rows must be >= 1 and iters >= 0"

    def __init__(self, train_real, test_real, meta: dict, vocabs: Sequence, device, ops=None,
                 target: Optional[str] = None, iters: int = 200, max_rows: int = 40000, graph: bool = False,
                 cardinalities: Optional[Sequence[int]] = None):
        """train_real / test_real: the real training and held-out rows as DataFrames, or already coded as float64
        [m, n_cols] arrays.  cardinalities: categories per categorical column (in column order, the target
        included), for coded arrays whose codes do not show them all."""
        super().__init__(meta, device, ops, max_rows, graph)
        self.iters = int(iters)
        if self.iters < 0:
            raise ValueError(f"DeviceUtility: {self.LIMITS}")
        coded, pooled, card_of = self._real_tables(train_real, test_real, meta, vocabs, target, cardinalities)
        self._setup_features(pooled, card_of)
        dev = self.device
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        self.betas = momentum_table(self.iters)
        D, K = self.D, self.K
        self.M, self.Minv = torch.zeros(D, D, **f64), torch.zeros(D, D, **f64)
        self.Lt, self.X = torch.zeros(D, D, **f64), torch.zeros(D, D, **f64)
        self.W, self.V, self.G = torch.zeros(D, K, **f64), torch.zeros(D, K, **f64), torch.zeros(D, K, **f64)
        self.loss = torch.zeros(1, **f64)
        self.conf = torch.zeros(K, K, **i32)
        self.real = torch.zeros(2, **f64)
        self.scores = torch.zeros(len(KEYS), **f64)
        self._fit_real(*coded)

    def _keep_real(self) -> None:
        self.real.copy_(self.scores[:2])
        self.W_real, self.conf_real = self.W.clone(), self.conf.clone()

    def _alloc(self, rows: int) -> None:
        dev, ops = self.device, self.ops
        self.train = self._table(rows)
        self.part = torch.zeros(max(ops.util_part(rows, self.D, self.K), 1), dtype=torch.float64, device=dev)
        self.lossp = torch.zeros((rows + ops.UTIL_CHUNK - 1) // ops.UTIL_CHUNK, dtype=torch.float64, device=dev)

    # ------------------------------------------------------------------ the pass
    def _fit(self, values: torch.Tensor, n: int) -> None:
        ops, t = self.ops, self.train
        self._pack(values, t)
        ops.util_gram(t, n, self.M, self.part)
        ops.util_factor(self.M, self.Lt, self.X, self.Minv)
        self.W.zero_()
        self.V.zero_()
        for beta in self.betas:
            ops.util_step(t, n, self.V, self.W, self.Minv, self.G, self.loss, self.part, self.lossp, beta)
        ops.util_grad(t, n, self.W, self.G, self.loss, self.part, self.lossp)

    def _launch(self, values: torch.Tensor, n: int) -> None:
        self._fit(values, n)
        self.ops.util_predict(self.test, self.n_test, self.train.counts, self.W, self.conf, self.G, self.loss,
                              self.real, self.scores)

    def _result(self, n: int) -> UtilityScores:
        return UtilityScores(self.scores.clone(), self.conf.clone(), self.W.clone())

    def score(self, values: torch.Tensor) -> UtilityScores:
        """values: [n, n_cols] float64 on the evaluator's device, as ``generate_decoded`` returns them (finite
        values in the continuous columns are a precondition).  The work is queued on the current stream; the
        returned scores are device tensors and nothing waits for them."""
        return super().score(values)
