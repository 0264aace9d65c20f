"""On-device correlation evaluator: the distance between the pairwise association matrices of the real and a
generated table (CTAB-GAN's "Diff. Corr.").

Avg_JSD / Avg_WD look at one column at a time and DCR / NNDR at whole rows; neither sees whether the generator kept
the dependencies between columns.  This evaluator does.  Rows live in the space of the decoded table
(``generate_decoded``'s ``[n, n_cols]`` float64: label codes in the categorical columns, log1p values in the
``non_negative_cols``); the real table is brought there with :func:`fed_tgan_amd.eval.privacy.code_real_table`.
The log scale is deliberate: it keeps one heavy-tailed value from deciding a Pearson coefficient, so for
non-negative columns the numbers are not what a tool working on the CSV would print.

For ``n`` rows and ``C`` columns the association matrix ``A`` is ``[C, C]`` float64 with ``A[i][i] = 1`` and

* continuous i, continuous j: Pearson r from centred sums, ``Sxy / sqrt(Sxx Syy)``, clamped to [-1, 1], 0 when either
  column is constant;
* categorical i, categorical j: Theil's U of i given j, ``(H(i) - H(i|j)) / H(i)`` from the integer contingency
  table with natural logs, clamped to [0, 1], 1 when ``H(i) == 0`` (the matrix is asymmetric);
* categorical a, continuous x (both positions): the correlation ratio ``sqrt(sum_k S_k^2 / n_k / Sxx)`` with ``S_k``
  the sum of the centred x over the rows of category k, over the categories with ``n_k > 0``, clamped to [0, 1], 0
  when ``Sxx == 0``.

Categorical column c has ``K_c = max(len(vocab_c), 1 + largest real code)`` categories (``cardinalities=`` may raise
it); a generated value that is NaN or no code of ``[0, K_c)`` counts in one extra overflow bin ``K_c``, which behaves
like a category.  The scores (``KEYS``): ``corr_diff = ||A_real - A_fake||_F``, ``corr_mean_abs`` and ``corr_max_abs``
the mean and the maximum of ``|A_real - A_fake|`` over the off-diagonal entries, and ``corr_diff_rr`` the sampling
noise baseline: the ``corr_diff`` between the real rows of even and of odd index (NaN with ``baseline=False`` or fewer
than two real rows).

``score(values)`` is a fixed single-stream launch sequence (``ops.corr_pack`` -> ``corr_moments`` -> ``corr_counts``
-> ``corr_matrix`` -> ``corr_diff``) over buffers allocated at construction, without allocation or host round trip,
so it can be captured in a hipGraph (``graph=True``).  The ops come from :class:`fed_tgan_amd.ops.hip.HipOps`
(kernels/correlation.hip) on a GPU and from :class:`fed_tgan_amd.ops.ref.TorchOps` elsewhere; the second is the
first's oracle.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import pandas as pd
import torch

from .base import DeviceEvaluator, category_counts, coded_table, column_slots, most_categories

CORR_CONT, CORR_CAT = 0, 1
KEYS = ("corr_diff", "corr_mean_abs", "corr_max_abs", "corr_diff_rr")
PAIR_KINDS = {(CORR_CONT, CORR_CONT): "pearson", (CORR_CAT, CORR_CAT): "theils_u"}


class CorrelationScores:
    """Scores of one table: ``buf`` = [corr_diff, corr_mean_abs, corr_max_abs, corr_diff_rr] on the device.
    Nothing here synchronises except :meth:`floats` and :meth:`pairs`."""

    def __init__(self, buf: torch.Tensor, a_fake: torch.Tensor, ev: "DeviceCorrelation"):
        self.buf = buf
        self._a = a_fake
        self._ev = ev

    def floats(self) -> Dict[str, float]:
        return {k: float(v) for k, v in zip(KEYS, self.buf.cpu().tolist())}

    def matrix(self) -> torch.Tensor:
        """A_fake, [C, C] float64 on the device"""
        return self._a

    def pairs(self, k: int = 10) -> pd.DataFrame:
        """The k column pairs whose association differs most between the real and the generated table (host frame:
        column_i, column_j, kind, real, fake, abs_diff).  Symmetric entries are listed once, Theil's U in both
        directions."""
        ev = self._ev
        real, fake = ev.A_real.cpu().numpy(), self._a.cpu().numpy()
        rows = []
        for i in range(ev.n_cols):
            for j in range(ev.n_cols):
                ki, kj = ev.kinds[i], ev.kinds[j]
                if i == j or (ki != kj or ki == CORR_CONT) and j < i:
                    continue
                rows.append((ev.names[i], ev.names[j], PAIR_KINDS.get((ki, kj), "correlation_ratio"),
                             float(real[i, j]), float(fake[i, j]), abs(float(real[i, j]) - float(fake[i, j]))))
        frame = pd.DataFrame(rows, columns=["column_i", "column_j", "kind", "real", "fake", "abs_diff"])
        frame = frame.sort_values("abs_diff", ascending=False, kind="stable")
        return frame.head(max(int(k), 0)).reset_index(drop=True)


class DeviceCorrelation(DeviceEvaluator):
    DATES = "the decoded table holds their parts, not the dates, so columns would not be comparable"

    def __init__(self, real, meta: dict, vocabs: Sequence, device, ops=None, max_rows: int = 40000,
                 baseline: bool = True, graph: bool = False, cardinalities: Optional[Sequence[int]] = None,
                 max_scratch_bytes: int = 256 << 20):
        """real: the real table as a DataFrame, or already coded as a float64 [m, n_cols] array.  cardinalities:
        categories per categorical column (in column order), for a coded array whose codes do not show them all."""
        super().__init__(meta, device, ops, max_rows, graph)
        ops = self.ops
        self.kinds = kind = [CORR_CAT if cat else CORR_CONT for cat in self.is_cat]
        slot, count = column_slots(kind)
        self.n_cat, self.n_cont = n_cat, n_cont = count.get(CORR_CAT, 0), count.get(CORR_CONT, 0)
        coded = coded_table(real, meta, vocabs, self.who)
        self.n_real = m = coded.shape[0]
        cat_cols = [j for j, k in enumerate(kind) if k == CORR_CAT]
        card = category_counts(coded, cat_cols, vocabs, cardinalities, self.who)
        self.card_list = card
        offs = [0]
        for K in card:
            offs.append(offs[-1] + K + 1)
        self.W = n_cont + offs[-1]
        # the tables: the columns' margins, then every pair a < b
        pairs = [(a, -1, card[a] + 1, 1) for a in range(n_cat)]
        pairs += [(a, b, card[a] + 1, card[b] + 1) for a in range(n_cat) for b in range(a + 1, n_cat)]
        poff = [0]
        for _, _, ka, kb in pairs:
            poff.append(poff[-1] + ka * kb)
        lds_limit = int(ops.CORR_LDS_BINS)
        in_lds = [ka * kb for _, _, ka, kb in pairs if ka * kb <= lds_limit]
        self.lds_bins = max(in_lds + [1])
        self.global_pairs = [(a, b) for a, b, ka, kb in pairs if ka * kb > lds_limit]
        self.scratch_bytes = 4 * poff[-1]
        if self.scratch_bytes > int(max_scratch_bytes) or poff[-1] >= 2 ** 31 or self.W >= 2 ** 31:
            raise ValueError(
                f"DeviceCorrelation: the contingency tables need {self.scratch_bytes} bytes of scratch, more than "
                f"max_scratch_bytes = {int(max_scratch_bytes)}; "
                + most_categories([self.names[j] for j in cat_cols], card))
        dev = self.device
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        self.kind = torch.tensor(kind, **i32)
        self.slot = torch.tensor(slot, **i32)
        self.card = torch.tensor(card, **i32)
        self.offs = torch.tensor(offs, **i32)
        self.pairs_t = torch.tensor(pairs, **i32).reshape(len(pairs), 4)
        self.poff = torch.tensor(poff, dtype=torch.int64, device=dev)
        self.counts = torch.zeros(max(poff[-1], 1), **i32)
        self.G = torch.zeros(self.W, n_cont, **f64)
        self.mean = torch.zeros(n_cont, **f64)
        self.A_real = torch.zeros(self.n_cols, self.n_cols, **f64)
        self.A = torch.zeros(self.n_cols, self.n_cols, **f64)
        self.scores = torch.zeros(len(KEYS), **f64)
        table = torch.from_numpy(coded).to(dev)
        self._alloc(m)
        rr = float("nan")
        if baseline and m >= 2:         # the real table's halves against each other, over the same pass
            even, odd = table[0::2].contiguous(), table[1::2].contiguous()
            self._matrix(even, int(even.shape[0]), self.A_real)
            self._matrix(odd, int(odd.shape[0]), self.A)
            ops.corr_diff(self.A_real, self.A, self.scores)
            rr = self.scores[0].clone()
        self._matrix(table, m, self.A_real)
        self.A.zero_()
        self.scores.zero_()
        self.scores[3] = rr
        self._alloc(self.max_rows)

    def _alloc(self, rows: int) -> None:
        dev = self.device
        self.cont = torch.zeros(rows, self.n_cont, dtype=torch.float64, device=dev)
        self.cat_t = torch.zeros(self.n_cat, rows, dtype=torch.int32, device=dev)
        self.part = torch.zeros(self.ops.corr_part(rows, self.W, self.n_cont), dtype=torch.float64, device=dev)

    # ------------------------------------------------------------------ the pass
    def _matrix(self, values: torch.Tensor, n: int, A: torch.Tensor) -> None:
        ops = self.ops
        ops.corr_pack(values, self.kind, self.slot, self.card, self.cont, self.cat_t, self.mean, self.part)
        ops.corr_moments(self.cont, self.cat_t, n, self.mean, self.card, self.offs, self.G, self.part)
        ops.corr_counts(self.cat_t, n, self.pairs_t, self.poff, self.counts, self.lds_bins)
        ops.corr_matrix(self.G, self.counts, self.poff, self.kind, self.slot, self.card, self.offs, n, A)

    def _launch(self, values: torch.Tensor, n: int) -> None:
        self._matrix(values, n, self.A)
        self.ops.corr_diff(self.A_real, self.A, self.scores)

    def _result(self, n: int) -> CorrelationScores:
        return CorrelationScores(self.scores.clone(), self.A.clone(), self)

    def score(self, values: torch.Tensor) -> CorrelationScores:
        """values: [n, n_cols] float64 on the evaluator's device, as ``generate_decoded`` returns them (finite
        values in the continuous columns are a precondition).  The work is queued on the current stream; the
        returned scores are device tensors and nothing waits for them."""
        return super().score(values)
