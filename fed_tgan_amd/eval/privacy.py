"""On-device privacy evaluator: DCR / NNDR of a decoded table against the real one.

Did the generator memorise real records?  The usual answer (CTAB-GAN and its successors report it) is two
nearest-neighbour metrics of every synthetic row against the real table:

* DCR, the distance to the closest record;
* NNDR, the nearest-neighbour distance ratio: nearest distance over second-nearest distance;

each reported as the 5th percentile over the synthetic rows, next to the same two numbers inside the real table
(every real row against the others), which serve as the baseline.

Rows live in the space of the decoded table (``generate_decoded``'s ``[n, n_cols]`` float64: label codes in the
categorical columns, log1p values in the ``non_negative_cols``, no integer rounding).  The real table is brought
there once: :class:`fed_tgan_amd.data.table.TablePreprocessor` with the lists ``meta`` carries, then the
vocabularies' codes, a real category outside a vocabulary getting a code past its end (it never equals a generated
code).  Continuous column c maps to ``(v - lo_c) * s_c`` with ``lo_c``, ``hi_c`` the real table's extremes and
``s_c = 1 / (hi_c - lo_c)`` (1 for a constant column), and

    d2(q, r) = sum over continuous columns of (q_c - r_c)^2 + number of categorical columns whose codes differ

in float64 from direct differences, so a copied record is at distance exactly 0.  DCR = sqrt(d1), NNDR =
sqrt(d1 / d2) with d1 <= d2 the two smallest d2 (with multiplicity), NNDR = 1 where d2 == 0 and 0 where there is no
second candidate.

``score(values)`` is a fixed launch sequence (``ops.nn_pack`` -> ``nn_top2`` -> ``nn_stats``) over buffers allocated
at construction, without allocation or host round trip, so it can be captured in a hipGraph (``graph=True``).  The
ops come from :class:`fed_tgan_amd.ops.hip.HipOps` (kernels/privacy.hip) on a GPU and from
:class:`fed_tgan_amd.ops.ref.TorchOps` elsewhere; the second is the first's oracle.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np
import pandas as pd
import torch

from ..data.constants import CATEGORICAL
from ..data.decode import meta_column_names
from ..data.table import TablePreprocessor
from .base import DeviceEvaluator, coded_table, column_slots

NN_CONT, NN_CAT = 0, 1
KEYS = ("dcr_p5", "nndr_p5", "dcr_min", "copies", "dcr_rr_p5", "nndr_rr_p5")


class PrivacyScores:
    """Scores of one table: ``buf`` = [dcr_p5, nndr_p5, dcr_min, copies, dcr_rr_p5, nndr_rr_p5] on the device.
    Nothing here synchronises except :meth:`floats`."""

    def __init__(self, buf: torch.Tensor, d1: torch.Tensor, d2: torch.Tensor, i1: torch.Tensor):
        self.buf = buf
        self._d1, self._d2, self._i1 = d1, d2, i1

    def floats(self) -> Dict[str, float]:
        return {k: float(v) for k, v in zip(KEYS, self.buf.cpu().tolist())}

    def rows(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """per-row (DCR, NNDR, index of a nearest real row) as device tensors"""
        d1, d2 = self._d1, self._d2
        none = torch.isinf(d2)
        ratio = torch.sqrt(torch.where(none, torch.zeros_like(d1), d1) /
                           torch.where(none | (d2 == 0), torch.ones_like(d2), d2))
        return torch.sqrt(d1), torch.where(d2 == 0, torch.ones_like(ratio), ratio), self._i1


def code_real_table(real: pd.DataFrame, meta: dict, vocabs: Sequence) -> np.ndarray:
    """The real frame in the row space of the decoded table: float64 [m, n_cols], columns in ``meta``'s order."""
    names = meta_column_names(meta)
    missing = [n for n in names if n not in real.columns]
    if missing:
        raise ValueError(f"DevicePrivacy: the real table lacks columns {missing[:5]}")
    cats = [c["column_name"] for c in meta["columns"] if c["type"] == CATEGORICAL]
    tp = TablePreprocessor(real[names], "real", str(meta.get("problem_type") or ""), str(meta.get("target") or ""),
                           cats, list(meta.get("non_negative_cols") or []))
    out = np.empty((len(tp.df), len(names)), dtype=np.float64)
    cursor = 0
    for j, name in enumerate(names):
        if name in cats:
            codes, labels = tp._cat_strings(name)
            vocab = vocabs[cursor]
            cursor += 1
            idx = pd.Index(vocab.classes_).get_indexer(np.asarray([str(s) for s in labels], dtype=object))
            unseen = idx < 0         # codes past the vocabulary: never equal to a generated code
            idx[unseen] = len(vocab) + np.arange(int(unseen.sum()))
            out[:, j] = idx[codes]
        else:
            v = pd.to_numeric(tp.df[name], errors="coerce").to_numpy(dtype=np.float64)
            if not np.isfinite(v).all():
                raise ValueError(f"DevicePrivacy: the real column {name!r} holds a value that is not a finite number")
            out[:, j] = v
    return out


class DevicePrivacy(DeviceEvaluator):
    def __init__(self, real, meta: dict, vocabs: Sequence, device, ops=None, max_rows: int = 40000,
                 baseline: bool = True, graph: bool = False, bounds=None):
        """real: the real table as a DataFrame, or already coded as a float64 [m, n_cols] array.  bounds: (lo, hi),
        float64 extremes per continuous column (in column order) to scale with instead of this table's own
        (:func:`table_bounds`, :func:`combine_bounds`): shards of one table scaled with the table's bounds give the
        distances the whole table gives (eval/fed_privacy.py)."""
        super().__init__(meta, device, ops, max_rows, graph)
        ops = self.ops
        kind = [NN_CAT if cat else NN_CONT for cat in self.is_cat]
        slot, count = column_slots(kind)
        self.n_cat, self.n_cont = n_cat, n_cont = count.get(NN_CAT, 0), count.get(NN_CONT, 0)
        coded = coded_table(real, meta, vocabs, self.who, finite="array")
        m = coded.shape[0]
        self.n_real = m
        dev = self.device
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        self.kind = torch.tensor(kind, **i32)
        self.slot = torch.tensor(slot, **i32)
        table = torch.from_numpy(np.ascontiguousarray(coded)).to(dev)
        cont_cols = torch.tensor([j for j, k in enumerate(kind) if k == NN_CONT], dtype=torch.long, device=dev)
        # MinMax on real, as stat_sim scales: lo and 1 / (hi - lo) of the real columns (1 for a constant column)
        rc = table[:, cont_cols]
        if bounds is not None:
            lo, hi = (np.ascontiguousarray(np.asarray(b, dtype=np.float64)).reshape(-1) for b in bounds)
            if lo.shape != (n_cont,) or hi.shape != (n_cont,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()):
                raise ValueError(f"{self.who}: bounds are two finite float64 [{n_cont}] rows (lo, hi), one entry per "
                                 "continuous column")
            self.lo, hi = torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)
        else:
            self.lo = rc.min(dim=0).values.contiguous() if n_cont else torch.zeros(0, **f64)
            hi = rc.max(dim=0).values if n_cont else torch.zeros(0, **f64)
        span = hi - self.lo
        self.scale = torch.where(span > 0, 1.0 / torch.where(span > 0, span, torch.ones_like(span)),
                                 torch.ones_like(span)).contiguous()
        self.r_cont = torch.zeros(m, n_cont, **f64)
        self.r_cat = torch.zeros(m, n_cat, **i32)
        ops.nn_pack(table, self.kind, self.slot, self.lo, self.scale, self.r_cont, self.r_cat)
        self.scores = torch.zeros(len(KEYS), **f64)
        self.scores[4:] = float("nan")
        if baseline:        # every real row against the others, once, over buffers of its own
            self._alloc(m)
            self._stats(self.r_cont, self.r_cat, m, True)
            self.scores[4:6] = self.scores[0:2]
            self.scores[:4] = 0.0
        self._alloc(self.max_rows)

    def _alloc(self, rows: int) -> None:
        ops, dev = self.ops, self.device
        f64 = dict(dtype=torch.float64, device=dev)
        self.q_cont = torch.zeros(rows, self.n_cont, **f64)
        self.q_cat = torch.zeros(rows, self.n_cat, dtype=torch.int32, device=dev)
        self.d1 = torch.zeros(rows, **f64)
        self.d2 = torch.zeros(rows, **f64)
        self.i1 = torch.zeros(rows, dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(ops.nn_scratch(rows, self.n_real), **f64)
        self.keys = torch.zeros(2, rows, **f64)
        self.tmp = torch.zeros(2, rows, **f64)
        self.part = torch.zeros(ops.nn_stats_part(rows), **f64)

    # ------------------------------------------------------------------ the pass
    def _stats(self, q_cont: torch.Tensor, q_cat: torch.Tensor, n: int, exclude_self: bool) -> None:
        ops = self.ops
        ops.nn_top2(q_cont, q_cat, self.r_cont, self.r_cat, exclude_self, self.d1, self.d2, self.i1, self.scratch)
        ops.nn_stats(self.d1, self.d2, n, self.keys, self.tmp, self.part, self.scores)

    def _launch(self, values: torch.Tensor, n: int) -> None:
        self.ops.nn_pack(values, self.kind, self.slot, self.lo, self.scale, self.q_cont, self.q_cat)
        self._stats(self.q_cont[:n], self.q_cat[:n], n, False)

    def _result(self, n: int) -> PrivacyScores:
        return PrivacyScores(self.scores.clone(), self.d1[:n].clone(), self.d2[:n].clone(), self.i1[:n].clone())

    def score(self, values: torch.Tensor) -> PrivacyScores:
        """values: [n, n_cols] float64 on the evaluator's device, as ``generate_decoded`` returns them (finite
        values are a precondition).  The work is queued on the current stream; the returned scores are device
        tensors and nothing waits for them."""
        return super().score(values)

    def guard(self, min_dcr: float = 0.0) -> "PrivacyGuard":
        """A :class:`PrivacyGuard` of radius ``min_dcr`` around this evaluator's real rows, sharing its packed table."""
        return PrivacyGuard._sharing(self, min_dcr)


def table_bounds(coded: np.ndarray, meta: dict) -> Tuple[np.ndarray, np.ndarray]:
    """(lo, hi) of a coded [m, n_cols] table: the float64 extremes of its continuous columns, in column order --
    what :class:`DevicePrivacy` scales with, and all of a client's shard that the federated audit shares."""
    cont = [j for j, c in enumerate(meta["columns"]) if c["type"] != CATEGORICAL]
    part = np.asarray(coded, dtype=np.float64)[:, cont]
    if part.shape[0] < 1:
        raise ValueError("table_bounds: the table is empty")
    return part.min(axis=0), part.max(axis=0)


def combine_bounds(pairs) -> Tuple[np.ndarray, np.ndarray]:
    """The bounds of the union of the tables the (lo, hi) pairs came from: elementwise min / max, exact."""
    pairs = [p for p in pairs if p is not None]
    if not pairs:
        raise ValueError("combine_bounds: no bounds")
    lo = np.min(np.stack([np.asarray(p[0], dtype=np.float64) for p in pairs]), axis=0)
    hi = np.max(np.stack([np.asarray(p[1], dtype=np.float64) for p in pairs]), axis=0)
    return lo, hi


def squared_radius(min_dcr) -> float:
    """t2 = T * T, one float64 product on the host; T must be a finite number >= 0."""
    t = float(min_dcr)
    if not np.isfinite(t) or t < 0:
        raise ValueError(f"min_dcr must be a finite number >= 0, got {min_dcr!r}")
    return t * t


class PrivacyGuard:
    """Generate only rows farther than ``min_dcr`` from every real record (``CTGANEngine.generate_decoded_guarded``).

    A generated row q is rejected iff some real row r has ``d2(q, r) <= t2`` with ``t2 = min_dcr * min_dcr`` and d2
    exactly :class:`DevicePrivacy`'s, so ``min_dcr = 0`` rejects exact copies only, and a row the guard keeps is a
    row the evaluator scores at ``d1 > t2``.  The guard holds what the evaluator holds -- the packed real table
    ``r_cont`` / ``r_cat``, ``lo``, ``scale``, ``kind``, ``slot`` -- and ``t2`` as a one-element device tensor, and
    refuses the same inputs (date tables, real values that are not finite).  The real records have to be on the
    generating machine."""

    def __init__(self, real, meta: dict, vocabs: Sequence, device, min_dcr: float = 0.0, ops=None):
        t2 = squared_radius(min_dcr)            # (refused before the table is packed)
        self._adopt(DevicePrivacy(real, meta, vocabs, device, ops=ops, max_rows=1, baseline=False), min_dcr, t2)

    @classmethod
    def _sharing(cls, evaluator: DevicePrivacy, min_dcr: float) -> "PrivacyGuard":
        self = cls.__new__(cls)
        self._adopt(evaluator, min_dcr, squared_radius(min_dcr))
        return self

    def _adopt(self, ev: DevicePrivacy, min_dcr: float, t2: float) -> None:
        self.device, self.ops = ev.device, ev.ops
        self.n_cols, self.n_cont, self.n_cat, self.n_real = ev.n_cols, ev.n_cont, ev.n_cat, ev.n_real
        self.kind, self.slot, self.lo, self.scale = ev.kind, ev.slot, ev.lo, ev.scale
        self.r_cont, self.r_cat = ev.r_cont, ev.r_cat
        self.min_dcr = float(min_dcr)
        self.t2 = torch.tensor([t2], dtype=torch.float64, device=self.device)

    def buffers(self, rows: int):
        """(q_cont, q_cat, near, scratch) for passes of up to ``rows`` rows"""
        dev = self.device
        return (torch.zeros(rows, self.n_cont, dtype=torch.float64, device=dev),
                torch.zeros(rows, self.n_cat, dtype=torch.int32, device=dev),
                torch.full((rows,), -1, dtype=torch.int32, device=dev),
                torch.zeros(self.ops.nn_scratch(rows, self.n_real), dtype=torch.float64, device=dev))

    def launch(self, values: torch.Tensor, q_cont, q_cat, near, scratch) -> None:
        """nn_pack -> nn_within of a decoded pass over buffers from :meth:`buffers`; nothing is allocated."""
        n = values.shape[0]
        self.ops.nn_pack(values, self.kind, self.slot, self.lo, self.scale, q_cont, q_cat)
        self.ops.nn_within(q_cont[:n], q_cat[:n], self.r_cont, self.r_cat, self.t2, near[:n], scratch)

    def near(self, values: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """values: any [n, n_cols] float64 table on the guard's device -> (too close: bool [n], near: int32 [n], the
        lowest index of a real row within the radius or -1)."""
        if values.dim() != 2 or values.shape[1] != self.n_cols or values.dtype != torch.float64:
            raise ValueError(f"near: expected a float64 [n, {self.n_cols}] table, got {tuple(values.shape)} "
                             f"{values.dtype}")
        if values.device != self.t2.device:
            raise ValueError(f"near: the table is on {values.device}, the guard on {self.t2.device}")
        n = int(values.shape[0])
        bufs = self.buffers(max(n, 1))
        if n:
            self.launch(values.contiguous(), *bufs)
        check = getattr(self.ops, "check", None)
        if check is not None:
            check()
        near = bufs[2][:n]
        return near >= 0, near
