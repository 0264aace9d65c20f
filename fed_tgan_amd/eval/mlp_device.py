"""On-device MLP utility: a one-hidden-layer network trained on the generated table and tested on real rows (TSTR),
the fourth of the reference's ``utility_analysis.py`` classifiers beside the logistic regression
(``eval/utility_device.py``) and the trees (``eval/forest_device.py``).

**Target, features, packing.**  Exactly :class:`DeviceUtility`'s: the same ``kind`` / ``slot`` / ``card`` / ``offs`` /
``mean`` / ``sd``, the same :class:`UtilityTable` filled by ``ops.util_pack``, ``D = n_cont + sum(K_c + 1) + 1`` with
the constant 1 as the last feature, the same limits ``UTIL_MAX_FEATURES`` / ``UTIL_MAX_CLASSES`` and the same refusals
(dates, a regression target, non-finite real values).  The rows are unweighted, as the reference's ``MLPClassifier``
has no class weights: a row whose target is a code of ``[0, K)`` counts 1, any other row 0; ``table.s`` is not used,
only ``y`` and ``counts``.

**Model.**  ``h = relu(F W1)``, ``z = [h | 1] W2``.  ``W1`` is ``[D, H]``, its last row the hidden bias (``F``'s last
column is the 1); ``W2`` is ``[H + 1, K]``, its last row the output bias; everything is float64 in one flat buffer
``theta = [W1 | W2]``; ``1 <= H <= MLP_MAX_HIDDEN = 128``.  Classes absent from the training table (``counts[c] ==
0``) have probability 0 and are never predicted: the softmax and the argmax run over the present classes, the lowest
class on a tie, class 0 with none present.

**Initial weights.**  sklearn's Glorot rule: ``W1[:-1]`` and the hidden bias uniform in ``+-sqrt(6 / (D - 1 + H))``,
``W2[:-1]`` and the output bias uniform in ``+-sqrt(6 / (H + K))``, drawn once on the host with
``numpy.random.default_rng(seed)`` in the order ``W1[:-1]``, hidden bias, ``W2[:-1]``, output bias, and kept on the
device as ``theta0``.  A fit starts with ``theta <- theta0`` and zero Adam moments; no device RNG is involved.

**Batches.**  With ``nb = ceil(n / batch)``, step ``k = 0 .. steps - 1`` uses batch ``b = k mod nb``: the rows ``b, b +
nb, b + 2 nb, ... < n``, at most ``batch`` of them.  The stride is deliberate: a training table sorted by class, or a
conditional generation grouped by value, still gives mixed batches without a shuffle.  ``1 <= batch <= MLP_MAX_BATCH
= 1024``.

**Objective and step.**  With ``m`` the valid rows of the batch (1 when there is none), ``g`` is the gradient of ``(sum
over the valid rows of CE(softmax(z_i), y_i) + alpha / 2 |W1 and W2 without their bias rows|^2) / m``.  Adam in
sklearn's form with ``t = k + 1``: ``m_t = 0.9 m + 0.1 g``, ``v_t = 0.999 v + 0.001 g^2``, ``theta -= lr sqrt(1 -
0.999^t) / (1 - 0.9^t) m_t / (sqrt(v_t) + 1e-8)``; the scalar factor is computed on the host per step
(:func:`step_sizes`).  The number of steps is fixed, there is no early stopping; ``0 <= steps <= MLP_MAX_STEPS =
10000`` (a captured pass holds two graph nodes per step).

**Scores** (``KEYS``).  ``mlp_f1_fake``, ``mlp_acc_fake``, ``mlp_f1_real``, ``mlp_acc_real`` (the same fit on the real
training rows, done once at construction), the gaps real - fake, and ``mlp_loss_fake``: the objective over the whole
generated table (``m`` its valid rows) after the last step.  Confusion matrix (int32 ``[K, K]``), weighted F1 and
accuracy as in :class:`DeviceUtility`.

**Not the reference's numbers.**  sklearn's ``MLPClassifier`` sees integer-coded categories, shuffles its batches and
stops itself; here the categories are one-hot, the batches strided and the steps fixed.

``score(values)`` is a fixed single-stream launch sequence (``ops.util_pack``, ``theta <- theta0`` and zeroed moments,
``steps`` x ``ops.mlp_step``, ``ops.mlp_loss``, ``ops.mlp_predict``) over buffers allocated at construction, without
allocation or host round trip, so it can be captured in a hipGraph (``graph=True``).  Every fp64 sum has an order fixed
by the shapes alone, so a table scores bit-identically on every run.  The ops come from
:class:`fed_tgan_amd.ops.hip.HipOps` (kernels/mlp.hip) on a GPU and from :class:`fed_tgan_amd.ops.ref.TorchOps`
elsewhere; the second is the first's oracle.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .base import TstrEvaluator
from .utility_device import PackedFeatures

KEYS = ("mlp_f1_fake", "mlp_acc_fake", "mlp_f1_real", "mlp_acc_real", "mlp_f1_gap", "mlp_acc_gap", "mlp_loss_fake")


def step_sizes(steps: int, lr: float) -> List[float]:
    """lr sqrt(1 - 0.999^t) / (1 - 0.9^t) for t = 1 .. steps"""
    return [lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t) for t in range(1, int(steps) + 1)]


def initial_weights(D: int, H: int, K: int, seed: int) -> np.ndarray:
    """theta0 = [W1 | W2] flat, by sklearn's Glorot rule (see the module docstring)"""
    g = np.random.default_rng(int(seed))
    b1, b2 = math.sqrt(6.0 / (D - 1 + H)), math.sqrt(6.0 / (H + K))
    parts = [g.uniform(-b1, b1, (D - 1, H)), g.uniform(-b1, b1, H), g.uniform(-b2, b2, (H, K)), g.uniform(-b2, b2, K)]
    return np.concatenate([p.reshape(-1) for p in parts])


class MLPScores:
    """Scores of one table: ``buf`` = the seven numbers of ``KEYS`` on the device.  Nothing here synchronises except
    :meth:`floats`."""

    def __init__(self, buf: torch.Tensor, conf: torch.Tensor, theta: torch.Tensor, D: int, H: int, K: int):
        self.buf = buf
        self._conf = conf
        self._theta, self._shape = theta, (int(D), int(H), int(K))

    def floats(self) -> Dict[str, float]:
        return {k: float(v) for k, v in zip(KEYS, self.buf.cpu().tolist())}

    def confusion(self) -> torch.Tensor:
        """int32 [K, K] on the device: test rows by (real class, predicted class)"""
        return self._conf

    def weights(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(W1 [D, H], W2 [H + 1, K]) float64 on the device, the fit on the generated table"""
        D, H, K = self._shape
        return self._theta[:D * H].view(D, H), self._theta[D * H:].view(H + 1, K)


class DeviceMLP(PackedFeatures, TstrEvaluator):
    LIMITS = "max_rows must be >= 1"

    def __init__(self, train_real, test_real, meta: dict, vocabs: Sequence, device, ops=None,
                 target: Optional[str] = None, hidden: int = 100, steps: int = 1000, batch: int = 512,
                 lr: float = 1e-3, alpha: float = 1e-4, seed: int = 0, max_rows: int = 40000, graph: bool = False,
                 cardinalities: Optional[Sequence[int]] = None):
        """train_real / test_real: the real training and held-out rows as DataFrames, or already coded as float64
        [m, n_cols] arrays.  cardinalities: categories per categorical column (in column order, the target
        included), for coded arrays whose codes do not show them all."""
        super().__init__(meta, device, ops, max_rows, graph)
        ops = self.ops
        self.hidden, self.steps, self.batch = int(hidden), int(steps), int(batch)
        self.lr, self.alpha, self.seed = float(lr), float(alpha), int(seed)
        if not 1 <= self.hidden <= int(ops.MLP_MAX_HIDDEN):
            raise ValueError(f"DeviceMLP: hidden {self.hidden} is outside 1 .. MLP_MAX_HIDDEN = "
                             f"{int(ops.MLP_MAX_HIDDEN)}")
        if not 1 <= self.batch <= int(ops.MLP_MAX_BATCH):
            raise ValueError(f"DeviceMLP: batch {self.batch} is outside 1 .. MLP_MAX_BATCH = {int(ops.MLP_MAX_BATCH)}")
        if not 0 <= self.steps <= int(ops.MLP_MAX_STEPS):
            raise ValueError(f"DeviceMLP: steps {self.steps} is outside 0 .. MLP_MAX_STEPS = {int(ops.MLP_MAX_STEPS)}"
                             "; a captured pass holds two graph nodes per step")
        if self.seed < 0 or not self.lr > 0.0 or not self.alpha >= 0.0:
            raise ValueError("DeviceMLP: seed and alpha must be >= 0 and lr > 0")
        coded, pooled, card_of = self._real_tables(train_real, test_real, meta, vocabs, target, cardinalities)
        self._setup_features(pooled, card_of)
        dev, D, H, K = self.device, self.D, self.hidden, self.K
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        self.lrs = step_sizes(self.steps, self.lr)
        self.theta0 = torch.from_numpy(initial_weights(D, H, K, self.seed)).to(dev)
        self.theta, self.m, self.v = (torch.zeros_like(self.theta0) for _ in range(3))
        rows = self.batch
        self.h, self.dh = torch.zeros(rows, H, **f64), torch.zeros(rows, H, **f64)
        self.dz = torch.zeros(rows, K, **f64)
        self.cnt = torch.zeros((rows + int(ops.MLP_ROWS) - 1) // int(ops.MLP_ROWS), **i32)
        self.conf = torch.zeros(K, K, **i32)
        self.real = torch.zeros(2, **f64)
        self.scores = torch.zeros(len(KEYS), **f64)
        self._fit_real(*coded)

    def _keep_real(self) -> None:
        self.real.copy_(self.scores[:2])
        self.theta_real, self.conf_real = self.theta.clone(), self.conf.clone()

    def _alloc(self, rows: int) -> None:
        R = int(self.ops.MLP_ROWS)
        self.train = self._table(rows)
        self.loss = torch.zeros(1 + (rows + R - 1) // R, dtype=torch.float64, device=self.device)

    # ------------------------------------------------------------------ the pass
    def _fit(self, values: torch.Tensor, n: int) -> None:
        ops, t, H = self.ops, self.train, self.hidden
        self._pack(values, t)
        self.theta.copy_(self.theta0)
        self.m.zero_()
        self.v.zero_()
        nb = (n + self.batch - 1) // self.batch
        for k, lr_t in enumerate(self.lrs):
            ops.mlp_step(t, n, k % nb, nb, self.theta, self.m, self.v, self.h, self.dz, self.dh, self.cnt, H,
                         self.alpha, lr_t)
        ops.mlp_loss(t, n, self.theta, H, self.alpha, self.loss)

    def _launch(self, values: torch.Tensor, n: int) -> None:
        self._fit(values, n)
        self.ops.mlp_predict(self.test, self.n_test, self.train.counts, self.theta, self.hidden, self.conf, self.loss,
                             self.real, self.scores)

    def _result(self, n: int) -> MLPScores:
        return MLPScores(self.scores.clone(), self.conf.clone(), self.theta.clone(), self.D, self.hidden, self.K)

    def score(self, values: torch.Tensor) -> MLPScores:
        """values: [n, n_cols] float64 on the evaluator's device, as ``generate_decoded`` returns them (finite
        values in the continuous columns are a precondition).  The work is queued on the current stream; the
        returned scores are device tensors and nothing waits for them."""
        return super().score(values)
