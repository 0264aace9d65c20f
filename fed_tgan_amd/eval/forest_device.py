"""On-device tree utility: a histogram decision tree (``dt``) and a random forest (``rf``) are trained on the generated
table and tested on real rows (TSTR); the gap to the same models trained on the real training rows is reported.

:class:`fed_tgan_amd.eval.utility_device.DeviceUtility` covers the reference's logistic regression; this evaluator
covers its two tree models (the MLP is ``eval/mlp_device.py``).  Rows live in the space of the decoded table
(``generate_decoded``'s ``[n, n_cols]`` float64: label codes in the categorical columns, log1p values in the
``non_negative_cols``); the real tables are brought there with :func:`fed_tgan_amd.eval.privacy.code_real_table`.
Tables with date columns, non-finite real values or a target that is not categorical are refused, and ``K`` and every
``K_c`` follow the rule of ``DeviceUtility``: ``max(len(vocab), 1 + largest real code, cardinalities[s])``.

**Bins.**  Every feature column becomes one byte per row, stored feature-major.  A categorical feature with ``K_c``
categories has bins ``0 .. K_c``, the last for a value that is NaN or no code; splits are ordinal on the code (what the
reference's trees do on label codes; our codes are frequency-ordered, theirs lexicographic).  A continuous feature gets
its edges once, at construction, on the host, from the pooled real table (train and test): with at most 256 distinct
values the midpoints between neighbouring distinct values, otherwise 255 edges at the ``k / 256`` quantiles (midpoint
interpolation), made distinct.  ``bin(v)`` is the number of edges ``e`` with ``v > e``, so "bin <= t" means ``v <=
edge_t``; a NaN lands in bin 0.  ``TREE_MAX_BINS = 256``: a categorical feature with ``K_c + 1 > 256`` is refused.
``TREE_MAX_CLASSES = 64``.

**Rows and class weights.**  A training row whose target is NaN or no code of ``[0, K)`` is left out; such a test row
is skipped.  ``count_c`` is the number of valid training rows of class ``c``; ``w_c = double(n_valid) /
(double(K_present) * double(count_c))``, 0 for an absent class (sklearn's ``class_weight="balanced"``).  The weights
are those of the whole table for every tree; the bootstrap does not change them.

**Criterion.**  A node has integer class counts ``n_c``, multiplicities included.  For a side of a candidate split
``m_c = double(n_c) * w_c``, ``T`` is the sum of ``m_c`` and ``Q`` the sum of ``m_c * m_c``, both over ``c = 0 .. K -
1`` in that order, each product rounded before it is added; the side's term is ``Q / T``.  A candidate (feature ``f``,
bin ``t``, left = "bin <= t") is valid if both sides hold at least ``min_leaf`` rows, multiplicities counted; its score
is ``Q_L / T_L + Q_R / T_R`` (maximising it minimises the weighted Gini impurity).  The right side's counts are the
node's minus the left's, in integers.  Every float operation is one correctly rounded fp64 operation in this order,
without contraction.  The best candidate of a node has the largest score; on a tie the lowest feature, then the lowest
bin.

**Growth** is level by level.  A node is split if its depth is below ``max_depth``, it holds rows of more than one
class and it has a valid candidate; no improvement threshold applies (sklearn's ``min_impurity_decrease = 0``: an XOR
table still splits).  Otherwise it is a leaf.  Nodes are stored per tree in level order, within a level by heap index
(root 1, children ``2 g`` and ``2 g + 1``), as the arrays ``feature`` (-1 for a leaf), ``bin``, ``left`` (the right
child is ``left + 1``), ``heap`` (0 for an unused slot) and ``counts [nodes, K]`` int32.  A tree's capacity is
``min(2^(max_depth + 1) - 1, 2 max_rows - 1)`` nodes; all buffers are sized at construction, and a configuration whose
buffers would pass ``max_scratch_bytes`` is refused.  ``TREE_MAX_DEPTH = 20``.

**The two models.**  ``dt`` is one tree over every valid row once, with every feature a candidate at every node.
``rf`` is ``trees`` trees: tree ``t`` draws ``n`` rows with replacement, draw ``j`` being row ``mulhi32(word(t, j),
n)`` with ``word`` the first output word of the project's Philox4x32-10 on the counter ``(j, t, TREE_STREAM_DRAW, 0)``
under the key ``seed``; multiplicities are added as integers and invalid rows then dropped.  At a node with heap index
``g`` feature ``f`` has the key ``word(f, t, TREE_STREAM_FEAT, g)``; among the features that have a valid candidate at
the node, the ``max(1, isqrt(F))`` with the smallest ``(key, f)`` compete (sklearn's rule: it keeps drawing until a
feature with a valid split is found).  Only integer Philox outputs are used.

**Prediction and scores.**  A test row walks a tree by its bins.  ``dt`` predicts the leaf's largest ``m_c`` (the
lowest class on a tie, class 0 for an empty tree).  ``rf`` adds ``p_{t,c} = m_c / T_leaf`` over the trees in tree order
(``T_leaf`` the sum of ``m_c`` in class order) and takes the largest, the lowest class on a tie.  A class absent from
the training table has ``w_c = 0`` and is never predicted.  The confusion matrices are int32 ``[K, K]``; weighted F1
and accuracy as in ``utility_device.py``, the F1 terms added in class order.  ``KEYS``: ``dt_f1_fake, dt_acc_fake,
dt_f1_real, dt_acc_real, dt_f1_gap, dt_acc_gap`` and the same six with ``rf_``; ``*_real`` come from the fits on the
real training rows, done once at construction; a gap is real - fake.

Everything above is integers, or fp64 in a fixed order, so trees, confusion matrices and scores are bit-identical on
every run, eager or replayed, and between the backends.

**Not the reference's numbers.**  sklearn grows unbounded-depth trees on exact thresholds with random tie-breaking;
here the thresholds are binned, the depth is limited and ties are broken in a fixed order.

``score(values)`` is a fixed single-stream launch sequence (``ops.tree_pack``, then per model ``tree_bootstrap`` ->
``tree_grow`` -> ``tree_predict`` -> ``tree_scores``) over buffers allocated at construction, without allocation or
host round trip, its number of launches a function of ``max_depth`` alone, so it can be captured in a hipGraph
(``graph=True``).  The ops come from :class:`fed_tgan_amd.ops.hip.HipOps` (kernels/forest.hip) on a GPU and from
:class:`fed_tgan_amd.ops.ref.TorchOps` elsewhere; the second is the first's oracle.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .base import TstrEvaluator, column_slots, most_categories

TREE_CONT, TREE_CAT, TREE_TARGET = 0, 1, 2
MODELS = ("dt", "rf")
_SIX = ("f1_fake", "acc_fake", "f1_real", "acc_real", "f1_gap", "acc_gap")
KEYS = tuple(f"{m}_{k}" for m in MODELS for k in _SIX)


def bin_edges(col: np.ndarray, max_bins: int = 256) -> np.ndarray:
    """the ascending distinct edges of a continuous column (see the module docstring)"""
    u = np.unique(col)
    if len(u) <= max_bins:
        e = (u[:-1] + u[1:]) / 2.0
    else:
        e = np.quantile(col, np.arange(1, max_bins) / float(max_bins), method="midpoint")
    return np.unique(e)


def tree_capacity(max_depth: int, rows: int) -> Tuple[int, int]:
    """(nodes of a tree, nodes of a level below max_depth) for tables of up to ``rows`` rows"""
    return min(2 ** (max_depth + 1) - 1, 2 * rows - 1), min(2 ** max_depth, rows)


def model_bytes(T: int, rows: int, K: int, max_depth: int) -> int:
    cap, lvl = tree_capacity(max_depth, rows)
    return 4 * (3 * T * rows + T * cap * (6 + K) + 4 * T + T * lvl * K)


class TreeTable:
    """The binned form of a table of up to ``rows`` rows (``ops.tree_pack`` fills it), with the binning constants."""

    def __init__(self, rows: int, card, edges, eoff, nbins, max_bins: int, K: int, device):
        F = int(nbins.numel())
        self.bins = torch.zeros(F, rows, dtype=torch.uint8, device=device)
        self.y = torch.zeros(rows, dtype=torch.int32, device=device)
        self.counts = torch.zeros(K, dtype=torch.int32, device=device)
        self.cw = torch.zeros(K, dtype=torch.float64, device=device)
        self.card, self.edges, self.eoff, self.nbins = card, edges, eoff, nbins
        self.max_bins, self.F, self.K = int(max_bins), F, int(K)


class TreeModel:
    """``T`` trees of up to ``cap`` nodes over tables of up to ``rows`` rows, and the scratch of their growth."""

    def __init__(self, T: int, rows: int, K: int, max_depth: int, device):
        i32 = dict(dtype=torch.int32, device=device)
        self.T, self.K = int(T), int(K)
        self.cap, self.lvl_cap = tree_capacity(int(max_depth), int(rows))
        self.mult = torch.zeros(T, rows, **i32)
        self.rows = torch.zeros(2, T, rows, **i32)
        self.feature = torch.full((T, self.cap), -1, **i32)
        self.bin = torch.zeros(T, self.cap, **i32)
        self.left = torch.zeros(T, self.cap, **i32)
        self.heap = torch.zeros(T, self.cap, **i32)
        self.counts = torch.zeros(T, self.cap, K, **i32)
        self.seg = torch.zeros(T, self.cap, 2, **i32)
        self.level = torch.zeros(T, 4, **i32)
        self.lcounts = torch.zeros(T, self.lvl_cap, K, **i32)

    def arrays(self, t: int):
        return dict(feature=self.feature[t], bin=self.bin[t], left=self.left[t], heap=self.heap[t],
                    counts=self.counts[t])


class ForestScores:
    """Scores of one table: ``buf`` = the twelve numbers of ``KEYS`` on the device (zeros for a model that was not
    asked for).  Nothing here synchronises except :meth:`floats`."""

    def __init__(self, buf: torch.Tensor, conf: Dict[str, torch.Tensor], models: Dict[str, TreeModel]):
        self.buf = buf
        self._conf = conf
        self._models = models

    def floats(self) -> Dict[str, float]:
        host = self.buf.cpu().tolist()
        return {k: float(v) for k, v in zip(KEYS, host) if k.split("_")[0] in self._models}

    def confusion(self, model: str) -> torch.Tensor:
        """int32 [K, K] on the device: test rows by (real class, predicted class)"""
        return self._conf[model]

    def tree(self, model: str, t: int) -> Dict[str, torch.Tensor]:
        """the arrays ``feature, bin, left, heap, counts`` of tree t on the device: views of the evaluator's
        buffers, valid until its next ``score``"""
        return self._models[model].arrays(int(t))


class DeviceForest(TstrEvaluator):
    LIMITS = "max_rows, trees and min_leaf must be >= 1 and seed >= 0"
    REUSE_REAL_BUFFERS = True

    def __init__(self, train_real, test_real, meta: dict, vocabs: Sequence, device, ops=None,
                 target: Optional[str] = None, trees: int = 100, max_depth: int = 12, min_leaf: int = 1, seed: int = 0,
                 max_rows: int = 40000, graph: bool = False, cardinalities: Optional[Sequence[int]] = None,
                 models: Sequence[str] = MODELS, max_scratch_bytes: int = 256 << 20):
        """train_real / test_real: the real training and held-out rows as DataFrames, or already coded as float64
        [m, n_cols] arrays.  cardinalities: categories per categorical column (in column order, the target
        included), for coded arrays whose codes do not show them all."""
        super().__init__(meta, device, ops, max_rows, graph)
        ops, self.trees, self.max_depth = self.ops, int(trees), int(max_depth)
        self.min_leaf, self.seed = int(min_leaf), int(seed)
        self.model_names = tuple(m for m in MODELS if m in tuple(models))
        if not self.model_names or set(models) - set(MODELS):
            raise ValueError(f"DeviceForest: models must be a non-empty subset of {MODELS}, got {tuple(models)}")
        if self.trees < 1 or self.min_leaf < 1 or self.seed < 0:
            raise ValueError(f"DeviceForest: {self.LIMITS}")
        if not 0 <= self.max_depth <= int(ops.TREE_MAX_DEPTH):
            raise ValueError(f"DeviceForest: max_depth {self.max_depth} is outside 0 .. TREE_MAX_DEPTH = "
                             f"{int(ops.TREE_MAX_DEPTH)}")
        coded, pooled, card_of = self._real_tables(train_real, test_real, meta, vocabs, target, cardinalities)
        max_bins = int(ops.TREE_MAX_BINS)
        kind = [TREE_TARGET if name == self.target else TREE_CAT if cat else TREE_CONT
                for name, cat in zip(self.names, self.is_cat)]
        slot, _ = column_slots(kind, {TREE_CAT: TREE_CONT})          # the features are numbered together
        card, nbins, eoff, edges, feat_names = [], [], [0], [], []
        for j, k in enumerate(kind):
            if k == TREE_TARGET:
                continue
            feat_names.append(self.names[j])
            if k == TREE_CAT:
                card.append(card_of[j])
                nbins.append(card[-1] + 1)
            else:
                card.append(0)
                edges.append(bin_edges(pooled[:, j], max_bins))
                nbins.append(len(edges[-1]) + 1)
            eoff.append(eoff[-1] + (0 if k == TREE_CAT else len(edges[-1])))
        self.F = len(nbins)
        if self.F < 1 or self.F > int(ops.TREE_MAX_FEATURES):
            raise ValueError(f"DeviceForest: {self.F} feature columns; 1 .. {int(ops.TREE_MAX_FEATURES)} are supported")
        if max(nbins) > max_bins or self.K > int(ops.TREE_MAX_CLASSES):
            raise ValueError(
                f"DeviceForest: a feature with {max(nbins)} bins and {self.K} classes of the target {self.target!r}; "
                f"the limits are TREE_MAX_BINS = {max_bins} (categories + 1) and TREE_MAX_CLASSES = "
                f"{int(ops.TREE_MAX_CLASSES)}; " + most_categories(feat_names, card))
        self.kinds, self.card_list, self.nbins_list = kind, card, nbins
        self.edges_list = edges
        self.m_feat = max(1, math.isqrt(self.F))
        self.max_scratch_bytes = int(max_scratch_bytes)
        for rows in (self.n_train, self.max_rows):
            need = rows * (self.F + 4) + sum(model_bytes(self._T(m), rows, self.K, self.max_depth)
                                             for m in self.model_names)
            if need > self.max_scratch_bytes:
                cap, lvl = tree_capacity(self.max_depth, rows)
                raise ValueError(
                    f"DeviceForest: {rows} rows, {self.trees} trees of up to {cap} nodes (max_depth {self.max_depth}) "
                    f"and {self.K} classes need {need} bytes of buffers, more than max_scratch_bytes = "
                    f"{self.max_scratch_bytes}; lower trees, max_depth or the rows")
        dev = self.device
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        self.kind = torch.tensor(kind, **i32)
        self.slot = torch.tensor(slot, **i32)
        self.card = torch.tensor(card, **i32)
        self.eoff = torch.tensor(eoff, **i32)
        self.nbins = torch.tensor(nbins, **i32)
        self.edges = torch.tensor(np.concatenate(edges) if edges else np.zeros(0), **f64)
        self.max_bins = max(nbins)
        K = self.K
        self.conf = {m: torch.zeros(K, K, **i32) for m in self.model_names}
        self.real = {m: torch.zeros(2, **f64) for m in self.model_names}
        self.scores = torch.zeros(len(KEYS), **f64)
        self._fit_real(*coded)

    def _T(self, model: str) -> int:
        return 1 if model == "dt" else self.trees

    def _table(self, rows: int) -> TreeTable:
        return TreeTable(rows, self.card, self.edges, self.eoff, self.nbins, self.max_bins, self.K, self.device)

    def _pack(self, values: torch.Tensor, table: TreeTable) -> None:
        self.ops.tree_pack(values, self.kind, self.slot, table)

    def _keep_real(self) -> None:
        for i, m in enumerate(MODELS):
            if m in self.real:
                self.real[m].copy_(self.scores[6 * i:6 * i + 2])
        self.conf_real = {m: c.clone() for m, c in self.conf.items()}

    def _alloc(self, rows: int) -> None:
        self.train = self._table(rows)
        self.models = {m: TreeModel(self._T(m), rows, self.K, self.max_depth, self.device) for m in self.model_names}

    # ------------------------------------------------------------------ the pass
    def _launch(self, values: torch.Tensor, n: int) -> None:
        ops, t = self.ops, self.train
        self._pack(values, t)
        for i, m in enumerate(MODELS):
            if m not in self.models:
                continue
            model, forest = self.models[m], m == "rf"
            ops.tree_bootstrap(model.mult, n, forest, self.seed)
            ops.tree_grow(t, n, model, self.max_depth, self.min_leaf, self.m_feat if forest else self.F, self.seed)
            ops.tree_predict(self.test, self.n_test, t.cw, model, forest, self.conf[m])
            ops.tree_scores(self.conf[m], self.real[m], self.scores[6 * i:6 * i + 6])

    def _result(self, n: int) -> ForestScores:
        return ForestScores(self.scores.clone(), {m: c.clone() for m, c in self.conf.items()}, self.models)

    def score(self, values: torch.Tensor) -> ForestScores:
        """values: [n, n_cols] float64 on the evaluator's device, as ``generate_decoded`` returns them.  The work is
        queued on the current stream; the returned scores are device tensors and nothing waits for them.  In the
        checked native build an index outside its table raises here."""
        return super().score(values)
