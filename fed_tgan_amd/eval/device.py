"""On-device statistical-similarity evaluator: Avg_JSD / Avg_WD of a decoded table without the CSV.

:func:`fed_tgan_amd.eval.similarity.stat_sim` scores the written CSV on one CPU core (``read_csv``, a
``value_counts`` and a sort per column).  Everything those scores need is on the device before the table is
copied to the host: ``generate_decoded`` leaves the ``[n, n_cols]`` float64 table there.  :class:`DeviceSimilarity`
computes the same two numbers from that tensor:

* the real table is prepared once: categorical columns are coded through the vocabularies (compared by the string
  the CSV would carry, so ``"empty"`` is ``" "``) and counted; numeric columns are sorted once on the device;
* ``score(values)`` runs a fixed sequence of launches (``ops.sim_prepare`` -> ``sim_sort`` -> ``sim_w1`` /
  ``sim_jsd`` -> ``sim_mean``) over scratch buffers allocated at construction, with no allocation and no host round
  trip, so it can be captured in a hipGraph (``graph=True``);
* the scores stay on the device (``scores.avg_jsd`` / ``scores.avg_wd`` are 0-dim tensors); ``scores.columns()``
  copies the per-column values to the host as the frame of ``column_similarity``.

The ops come from :class:`fed_tgan_amd.ops.hip.HipOps` (kernels/similarity.hip) on a GPU and from
:class:`fed_tgan_amd.ops.ref.TorchOps` elsewhere; the two share one contract and the second is the first's oracle.

Tables with date columns are refused: the CSV re-joins the date parts into one column, which the decoded value
matrix does not hold, so the scores would not be comparable.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np
import pandas as pd
import torch

from ..data.constants import CATEGORICAL, EMPTY
from .base import MAX_GRAPHS, GraphedPass  # noqa: F401  (re-exported: tests and tools import them from here)
from .base import DeviceEvaluator, column_slots

SIM_PLAIN, SIM_NONNEG, SIM_CAT = 0, 1, 2


class SimilarityScores:
    """Scores of one table: ``[avg_jsd, avg_wd, jsd per categorical column, wd per continuous column]`` on the
    device.  Nothing here synchronises except :meth:`columns` and :meth:`floats`."""

    def __init__(self, buf: torch.Tensor, sim: "DeviceSimilarity"):
        self.buf = buf
        self._sim = sim

    @property
    def avg_jsd(self) -> torch.Tensor:
        return self.buf[0]

    @property
    def avg_wd(self) -> torch.Tensor:
        return self.buf[1]

    def floats(self) -> Tuple[float, float]:
        a = self.buf[:2].cpu().tolist()
        return float(a[0]), float(a[1])

    def columns(self) -> pd.DataFrame:
        """The frame of :func:`fed_tgan_amd.eval.similarity.column_similarity` (columns in the real frame's order)."""
        host = self.buf.cpu().tolist()
        s = self._sim
        rows = []
        for name in s.order:
            k, slot = s.col_of[name]
            if k == SIM_CAT:
                rows.append([name, "categorical", "JSD", host[2 + slot]])
            else:
                rows.append([name, "continuous", "WD", host[2 + s.n_cat + slot]])
        return pd.DataFrame(rows, columns=["column", "type", "metric", "value"])


def _csv_string(s: str) -> str:
    return " " if s == EMPTY else s


class DeviceSimilarity(DeviceEvaluator):
    DATES = "the CSV re-joins their parts into one column, so device scores would not be comparable with stat_sim"

    def __init__(self, real: pd.DataFrame, meta: dict, vocabs: Sequence, device, ops=None, max_rows: int = 40000,
                 graph: bool = False):
        super().__init__(meta, device, ops, max_rows, graph)
        ops, names = self.ops, self.names
        missing = [n for n in names if n not in real.columns]
        if missing:
            raise ValueError(f"DeviceSimilarity: the real table lacks columns {missing[:5]}")
        nonneg = set(meta.get("non_negative_cols") or [])
        kind = [SIM_CAT if cat else SIM_NONNEG if name in nonneg else SIM_PLAIN for name, cat in zip(names, self.is_cat)]
        slot, _ = column_slots(kind, {SIM_NONNEG: SIM_PLAIN})
        vocab_n, cat_counts, cont_vals = [], [], []
        cursor = 0
        for c in meta["columns"]:
            name = c["column_name"]
            if c["type"] == CATEGORICAL:
                strings = [_csv_string(s) for s in vocabs[cursor].tolist()]
                cursor += 1
                index = {s: i for i, s in enumerate(strings)}
                col = real[name].dropna()
                counts: Dict[int, int] = {}
                # real values outside the vocabulary: real categories the fake table always misses (extra slots)
                for s, cnt in col.astype(str).value_counts().items():
                    i = index.setdefault(s, len(index))
                    counts[i] = counts.get(i, 0) + int(cnt)
                row = np.zeros(len(index), dtype=np.int64)
                for i, cnt in counts.items():
                    row[i] = cnt
                vocab_n.append(len(strings))
                cat_counts.append(row)
            else:
                v = pd.to_numeric(real[name], errors="coerce").to_numpy(dtype=np.float64)
                cont_vals.append(v[np.isfinite(v)])
        self.col_of = {name: (k, sl) for name, k, sl in zip(names, kind, slot)}
        self.order = [n for n in real.columns if n in self.col_of]
        self.n_cat, self.n_cont = len(cat_counts), len(cont_vals)
        dev = self.device
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        self.kind = torch.tensor(kind, **i32)
        self.slot = torch.tensor(slot, **i32)
        self.vocab = torch.tensor(vocab_n, **i32)
        width = max([len(r) for r in cat_counts] + [1])
        rc = np.zeros((self.n_cat, width), dtype=np.int32)
        for i, r in enumerate(cat_counts):
            rc[i, :len(r)] = r
        self.real_counts = torch.from_numpy(rc).to(dev)
        self.counts = torch.zeros(self.n_cat, width, **i32)
        ldr = max([len(v) for v in cont_vals] + [1])
        rk = np.full((self.n_cont, ldr), np.inf)
        for i, v in enumerate(cont_vals):
            rk[i, :len(v)] = v
        self.real_keys = torch.from_numpy(rk).to(dev)
        self.n_real = torch.tensor([len(v) for v in cont_vals], **i32)
        if self.n_cont:
            ops.sim_sort(self.real_keys, ldr, torch.empty_like(self.real_keys))
        self.keys = torch.empty(self.n_cont, self.max_rows, **f64)
        self.tmp = torch.empty(self.n_cont, self.max_rows, **f64)
        self.valid = torch.zeros(self.n_cont, **i32)
        self.part = torch.zeros(ops.sim_w1_part(self.n_cont, ldr + self.max_rows), **f64)
        self.scores = torch.zeros(2 + self.n_cat + self.n_cont, **f64)
        self._jsd = self.scores[2:2 + self.n_cat]
        self._wd = self.scores[2 + self.n_cat:]

    # ------------------------------------------------------------------ the pass
    def _launch(self, values: torch.Tensor, n: int) -> None:
        ops = self.ops
        ops.sim_prepare(values, self.kind, self.slot, self.vocab, self.keys, self.valid, self.counts)
        ops.sim_sort(self.keys, n, self.tmp)
        ops.sim_w1(self.real_keys, self.n_real, self.keys, self.valid, n, self._wd, self.part)
        ops.sim_jsd(self.real_counts, self.counts, self._jsd)
        ops.sim_mean(self.scores, self.n_cat, self.n_cont)

    def _result(self, n: int) -> SimilarityScores:
        return SimilarityScores(self.scores.clone(), self)

    def score(self, values: torch.Tensor) -> SimilarityScores:
        """values: [n, n_cols] float64 on the evaluator's device, as ``generate_decoded`` returns them.  The work is
        queued on the current stream; the returned scores are device tensors and nothing waits for them.  In the
        checked native build a code outside its vocabulary raises here."""
        return super().score(values)
