"""What the on-device evaluators share: one base class and the helpers of their constructors.

An evaluator scores a decoded table (``generate_decoded``'s ``[n, n_cols]`` float64) against real rows prepared once
at construction.  :class:`DeviceEvaluator` owns the common construction (device, ops, ``max_rows``, column names, graph
bookkeeping) and ``score(values)``: the checks of the table, the pass itself, eager or replayed as a hipGraph, and the
result.  A subclass supplies its buffers (``self.scores`` among them), the fixed launch sequence ``_launch(values, n)``
over them and ``_result(n)``, which clones what the pass left into its own ``...Scores`` object.
:class:`TstrEvaluator` adds what the two train-on-synthetic, test-on-real evaluators share.

The ops come from :class:`fed_tgan_amd.ops.hip.HipOps` on a GPU and from :class:`fed_tgan_amd.ops.ref.TorchOps`
elsewhere (:func:`default_ops`); the two share one contract and the second is the first's oracle.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd
import torch

from ..data.constants import CATEGORICAL
from ..data.decode import meta_column_names
from ..utils.devsync import warm_and_capture

MAX_GRAPHS = 4     # captured passes that read the caller's own buffer; tables beyond them are staged into ours


def default_ops(device: torch.device):
    if device.type == "cuda":
        from ..ops.hip import HipOps
        return HipOps(device)
    from ..ops.ref import TorchOps
    return TorchOps()


def column_slots(kinds: Sequence[int], group: Optional[Dict[int, int]] = None) -> Tuple[List[int], Dict[int, int]]:
    """slot[j] = the index of column j among the columns of its kind, and the number of columns per kind.  ``group``
    maps a kind to the kind it is numbered with."""
    slot, seen = [], {}
    for k in kinds:
        g = k if group is None else group.get(k, k)
        slot.append(seen.get(g, 0))
        seen[g] = slot[-1] + 1
    return slot, seen


def check_real_columns(coded: np.ndarray, names: Sequence[str], is_cat: Sequence[bool], who: str,
                       codes: bool = True) -> None:
    """Every continuous column finite; with ``codes`` every categorical column finite and non-negative too."""
    for j, cat in enumerate(is_cat):
        col = coded[:, j]
        if cat and not codes:
            continue
        if not np.isfinite(col).all() or (cat and (col < 0).any()):
            raise ValueError(f"{who}: the real column {names[j]!r} holds a value that is not a "
                             + ("category code" if cat else "finite number"))


def coded_table(real, meta: dict, vocabs: Sequence, who: str, what: str = "real", lost_rows: bool = False,
                finite: Optional[str] = "all") -> np.ndarray:
    """A real table in the row space of the decoded table, float64 [m, n_cols]: a DataFrame through
    :func:`fed_tgan_amd.eval.privacy.code_real_table` (whose own messages name DevicePrivacy), anything else taken
    as already coded.  ``what`` names the table in the messages; ``lost_rows`` refuses a frame that coding shortened;
    ``finite``: ``"all"`` checks every column (:func:`check_real_columns`), ``"array"`` the continuous columns of an
    already coded table only, ``None`` leaves the check to the caller."""
    names = meta_column_names(meta)
    if isinstance(real, pd.DataFrame):
        from .privacy import code_real_table
        coded = code_real_table(real, meta, vocabs)
        if lost_rows and coded.shape[0] != len(real):
            raise ValueError(f"{who}: the {what} table lost rows in coding")
    else:
        coded = np.ascontiguousarray(np.asarray(real, dtype=np.float64))
        if coded.ndim != 2 or coded.shape[1] != len(names):
            raise ValueError(f"{who}: expected a coded [m, {len(names)}] {what} table, got {coded.shape}")
    is_cat = [c["type"] == CATEGORICAL for c in meta["columns"]]
    if finite == "array" and not isinstance(real, pd.DataFrame):
        check_real_columns(coded, names, is_cat, who, codes=False)
    if coded.shape[0] < 1:
        raise ValueError(f"{who}: the {what} table is empty")
    if finite == "all":
        check_real_columns(coded, names, is_cat, who)
    return coded


def category_counts(coded: np.ndarray, cat_cols: Sequence[int], vocabs: Sequence,
                    cardinalities: Optional[Sequence[int]], who: str) -> List[int]:
    """``K_c = max(len(vocab_c), 1 + largest real code, cardinalities[c])`` per categorical column, in column order."""
    if cardinalities is not None and len(cardinalities) != len(cat_cols):
        raise ValueError(f"{who}: cardinalities needs one entry per categorical column ({len(cat_cols)})")
    card = []
    for s, j in enumerate(cat_cols):
        K = 1 + int(coded[:, j].max())
        if s < len(vocabs):
            K = max(K, len(vocabs[s]))
        if cardinalities is not None:
            K = max(K, int(cardinalities[s]))
        card.append(K)
    return card


def most_categories(names: Sequence[str], card: Sequence[int]) -> str:
    worst = sorted(range(len(card)), key=lambda s: -card[s])[:5]
    return "the columns with the most categories are " + ", ".join(f"{names[s]!r} ({card[s]})" for s in worst)


class DeviceEvaluator:
    """A fixed launch sequence ``_launch(values, n)`` over buffers allocated at construction, scored eagerly or replayed
    as a hipGraph (``graph=True``), and its result ``_result(n)``.

    ``score`` ends with ``ops.check()`` where the ops have one.  That is the checked native build, whose status word
    is global: an index outside its table, in any kernel since the last check, raises there.  The release build has
    nothing to check."""

    DATES = "the decoded table holds their parts, not the dates, so rows would not be comparable"
    LIMITS = "max_rows must be >= 1"

    def __init__(self, meta: dict, device, ops, max_rows: int, graph: bool):
        self.who = type(self).__name__
        if meta.get("date_info"):
            raise ValueError(f"{self.who}: the table has date columns; {self.DATES}")
        self.device = torch.device(device)
        self.ops = default_ops(self.device) if ops is None else ops
        self.max_rows = int(max_rows)
        if self.max_rows < 1:
            raise ValueError(f"{self.who}: {self.LIMITS}")
        self.names: List[str] = meta_column_names(meta)
        self.n_cols = len(self.names)
        self.is_cat = [c["type"] == CATEGORICAL for c in meta["columns"]]
        self.graph = bool(graph) and self.device.type == "cuda"
        self._graphs: Dict[Tuple[int, int], object] = {}
        self._staged = None                          # [max_rows, n_cols], made when a table has to be staged

    def _launch(self, values: torch.Tensor, n: int) -> None:
        raise NotImplementedError

    def _result(self, n: int):
        raise NotImplementedError

    def _replay(self, values: torch.Tensor, n: int) -> None:
        # a captured pass reads the buffer it was captured on: generate_decoded returns the same one per n, so the
        # first few (n, buffer) pairs get a graph of their own; any further table is staged into one of ours
        g = self._graphs.get((n, values.data_ptr()))
        if g is None and len(self._graphs) >= MAX_GRAPHS:
            if self._staged is None:
                self._staged = torch.empty(self.max_rows, self.n_cols, dtype=torch.float64, device=self.device)
            stage = self._staged[:n]
            stage.copy_(values)
            values = stage
            g = self._graphs.get((n, values.data_ptr()))
        key = (n, values.data_ptr())
        if g is None:
            def launch():
                self._launch(values, n)
            g, = warm_and_capture(self.device, launch, [launch])
            self._graphs[key] = g
        g.replay()

    def score(self, values: torch.Tensor):
        """values: [n, n_cols] float64 on the evaluator's device, as ``generate_decoded`` returns them.  The work is
        queued on the current stream; the returned scores are device tensors and nothing waits for them."""
        if values.dim() != 2 or values.shape[1] != self.n_cols or values.dtype != torch.float64:
            raise ValueError(f"score: expected a float64 [n, {self.n_cols}] table, got {tuple(values.shape)} "
                             f"{values.dtype}")
        if values.device != self.scores.device:      # (not self.device: "cuda" and "cuda:0" compare unequal)
            raise ValueError(f"score: the table is on {values.device}, the evaluator on {self.scores.device}")
        n = int(values.shape[0])
        if n < 1 or n > self.max_rows:
            raise ValueError(f"score: {n} rows; this evaluator's buffers hold 1..{self.max_rows}")
        values = values.contiguous()
        if self.graph:
            self._replay(values, n)
        else:
            self._launch(values, n)
        out = self._result(n)
        check = getattr(self.ops, "check", None)
        if check is not None:
            check()
        return out


GraphedPass = DeviceEvaluator     # the name it had while it held the replay alone


class TstrEvaluator(DeviceEvaluator):
    """Train on the synthetic table, test on real rows: a categorical target, the real training and held-out rows
    coded once, and the same fit on the real training rows done once at construction.  A subclass supplies ``_table(
    rows)`` (an empty packed table), ``_pack(values, table)``, ``_alloc(rows)`` (``self.train`` and the scratch of a
    fit of up to ``rows`` rows) and ``_keep_real()``."""

    REUSE_REAL_BUFFERS = False      # keep the buffers of the real fit when max_rows == n_train

    def _real_tables(self, train_real, test_real, meta: dict, vocabs: Sequence, target: Optional[str],
                     cardinalities: Optional[Sequence[int]]):
        """Sets ``target``, ``K``, ``n_train`` and ``n_test``; returns the coded (training, test) tables, the two
        pooled, and ``K_c`` by column index."""
        who = self.who
        self.target = str(target if target is not None else meta.get("target") or "")
        if self.target not in self.names or not self.is_cat[self.names.index(self.target)]:
            raise ValueError(f"{who}: the target {self.target!r} is not a categorical column of the table; "
                             "regression targets are not supported")
        coded = [coded_table(real, meta, vocabs, who, f"real {what}", lost_rows=True, finite=None)
                 for what, real in (("training", train_real), ("test", test_real))]
        pooled = np.concatenate(coded, axis=0)
        check_real_columns(pooled, self.names, self.is_cat, who)
        cat_cols = [j for j, cat in enumerate(self.is_cat) if cat]
        card_of = dict(zip(cat_cols, category_counts(pooled, cat_cols, vocabs, cardinalities, who)))
        self.K = card_of[self.names.index(self.target)]
        self.n_train, self.n_test = int(coded[0].shape[0]), int(coded[1].shape[0])
        return coded, pooled, card_of

    def _fit_real(self, train: np.ndarray, test: np.ndarray) -> None:
        """the held-out rows are packed once; the real training rows are fitted once with the pass of score()"""
        dev = self.device
        self.test = self._table(self.n_test)
        self._pack(torch.from_numpy(test).to(dev), self.test)
        self._alloc(self.n_train)
        self._launch(torch.from_numpy(train).to(dev), self.n_train)
        self._keep_real()
        self.scores.zero_()
        if not (self.REUSE_REAL_BUFFERS and self.max_rows == self.n_train):
            self._alloc(self.max_rows)
