"""Completion of partial rows: "here is a table with holes, fill them".

A request of :mod:`models.conditional` is one condition for a whole table.  Here every row fixes its own cells: the
input is a table ``known`` [N, n_cols] in the decoded (model) space -- label codes for categorical columns, log1p
values in the non-negative columns -- and a mask of the same shape that says which cells are known.
``CTGANEngine.generate_decoded_known`` generates ``tries`` candidate rows per known row, each under the row's own
condition, and keeps the candidate closest to the known cells (the privacy evaluator's mixed distance over the
known cells alone); the known cells of the result are the input's, the others the winner's.

:func:`parse_known` brings a DataFrame or a CSV to that form, :func:`build_known` chooses, once per table and
vectorised over its rows, the condition that drives each row's candidates:

* the row's known categorical cell whose option has the fewest training rows (ties: the lowest column) -- the
  value the unconditioned generator is least likely to produce by itself;
* else, for a row that knows only continuous cells, the mode of its first known continuous column that most
  likely produced the value: the largest ``count_k * N(x; mu_k, sd_k)`` among the modes with ``|x - mu_k| <= 4
  sd_k`` (the decode reaches no further);
* else none: the generation sampler's own draw stays.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from ..data.constants import CATEGORICAL, CONTINUOUS, EMPTY
from .conditional import _span_of, mode_tables

BLANK = ""      # a blank cell of a CSV read as text


def _is_blank(v) -> bool:
    if v is None:
        return True
    if isinstance(v, str):
        return v == BLANK
    try:
        return bool(np.isnan(v))
    except TypeError:
        return False


def _label(v) -> str:
    """A cell of a categorical column as the vocabulary spells it: an integral float prints as an integer (a column
    of codes with holes is read as float)."""
    if isinstance(v, (float, np.floating)) and float(v).is_integer():
        return str(int(v))
    return str(v)


def parse_known(frame_or_path, meta: dict, vocabs: Sequence, transformer) -> Tuple[np.ndarray, np.ndarray]:
    """(known float64 [N, n_cols], mask uint8 [N, n_cols]) of a partial table: a DataFrame, or the path of a CSV
    (read as text, so a blank cell is a blank and nothing else).  Columns are matched by name, in any order.

    * a model column the table lacks is unknown for every row; a column the model does not have is refused;
    * a blank (empty string, None) or NaN cell is unknown;
    * a categorical cell holds a label as the CSV prints it; ``" "`` and the literal ``empty`` are the category
      the CSV prints as a blank; a label outside the vocabulary, or one the model has no option for, raises
      ValueError naming the column, the value and the first row that holds it;
    * a continuous cell holds a finite number; in a non-negative column it is converted with log1p and a negative
      value is an error;
    * a table with date columns is refused (their parts are not cells of the input).

    Unknown cells hold 0.0 in ``known``; nothing reads them."""
    import pandas as pd
    if meta.get("date_info"):
        raise ValueError("completion of partial rows does not take tables with date columns "
                         f"({sorted(meta['date_info'])})")
    if isinstance(frame_or_path, (str, bytes)) or hasattr(frame_or_path, "__fspath__"):
        frame = pd.read_csv(frame_or_path, dtype=str, keep_default_na=False)
    else:
        frame = frame_or_path
    names = [c["column_name"] for c in meta["columns"]]
    extra = [str(c) for c in frame.columns if c not in names]
    if extra:
        raise ValueError(f"the partial table has columns the model does not have: {extra[:5]}")
    nonneg = set(meta.get("non_negative_cols") or [])
    n = len(frame)
    known = np.zeros((n, len(names)), dtype=np.float64)
    mask = np.zeros((n, len(names)), dtype=np.uint8)
    cursor = 0
    for j, c in enumerate(meta["columns"]):
        name = c["column_name"]
        is_cat = c["type"] == CATEGORICAL
        vocab = None
        if is_cat:
            vocab = vocabs[cursor]
            cursor += 1
        if name not in frame.columns or n == 0:
            continue
        col = frame[name]
        codes, uniq = pd.factorize(col.astype(object), use_na_sentinel=False)
        blank = np.asarray([_is_blank(u) for u in uniq], dtype=bool)
        value = np.zeros(len(uniq), dtype=np.float64)

        def first_row(k):
            return int(np.nonzero(codes == k)[0][0])

        if is_cat and transformer.meta[j]["type"] != CONTINUOUS:
            labels = [str(s) for s in vocab.tolist()]
            options = set(float(x) for x in transformer.meta[j]["i2s"])
            for k, u in enumerate(uniq):
                if blank[k]:
                    continue
                s = _label(u)
                if s == " " or s == EMPTY:
                    s = EMPTY
                if s not in labels:
                    raise ValueError(f"column {name!r}: value {u!r} (row {first_row(k)}) is not in the vocabulary")
                code = labels.index(s)
                if float(code) not in options:
                    raise ValueError(f"column {name!r}: value {u!r} (row {first_row(k)}) is not among the model's "
                                     "options")
                value[k] = float(code)
        else:
            for k, u in enumerate(uniq):
                if blank[k]:
                    continue
                try:
                    x = float(u)
                except (TypeError, ValueError):
                    raise ValueError(f"column {name!r}: value {u!r} (row {first_row(k)}) is not a number") from None
                if not np.isfinite(x):
                    raise ValueError(f"column {name!r}: value {u!r} (row {first_row(k)}) is not finite")
                if name in nonneg:
                    if x < 0:
                        raise ValueError(f"column {name!r} is non-negative; value {u!r} (row {first_row(k)}) is "
                                         "negative")
                    x = float(np.log1p(x))
                value[k] = x
        known[:, j] = value[codes]
        mask[:, j] = (~blank[codes]).astype(np.uint8)
    return known, mask


def column_scales(transformer) -> Tuple[np.ndarray, np.ndarray]:
    """(kind int32 [n_cols]: 0 continuous / 1 categorical, scale float64 [n_cols]) of the match: a continuous
    column is scaled by 1 / (max - min) of the model's own meta (1 where they are equal or absent), the choice
    DevicePrivacy makes with a real table's bounds."""
    kind = np.zeros(len(transformer.meta), dtype=np.int32)
    scale = np.ones(len(transformer.meta), dtype=np.float64)
    for j, m in enumerate(transformer.meta):
        if m["type"] != CONTINUOUS:
            kind[j] = 1
            continue
        lo, hi = m.get("min"), m.get("max")
        if lo is not None and hi is not None:
            span = float(hi) - float(lo)
            if np.isfinite(span) and span > 0:
                scale[j] = 1.0 / span
    return kind, scale


def build_known(transformer, counts, known, mask) -> Dict[str, np.ndarray]:
    """The per-table arrays of ``generate_decoded_known``: ``drv_span`` / ``drv_opt`` int32 [N] (the condition that
    drives each row's candidates, span -1 for none; this module's docstring), ``kind`` int32 / ``scale`` float64
    [n_cols] (:func:`column_scales`), and ``known`` / ``mask`` as contiguous float64 / uint8 arrays.  ``counts``:
    CondTables.counts, the training rows per span and option.  Raises ValueError for a known cell that is not
    finite or a known categorical code the model has no option for."""
    known = np.ascontiguousarray(np.asarray(known, dtype=np.float64))
    mask = np.ascontiguousarray((np.asarray(mask) != 0).astype(np.uint8))
    meta = transformer.meta
    if known.ndim != 2 or known.shape != mask.shape or known.shape[1] != len(meta):
        raise ValueError(f"known and mask must both be [N, {len(meta)}], got {known.shape} and {mask.shape}")
    on = mask != 0
    if not np.isfinite(np.where(on, known, 0.0)).all():
        raise ValueError("a known cell holds a value that is not a finite number")
    known = np.where(on, known, 0.0)
    counts = np.asarray(counts, dtype=np.float64)
    n = known.shape[0]
    kind, scale = column_scales(transformer)
    drv_span = np.full(n, -1, dtype=np.int32)
    drv_opt = np.zeros(n, dtype=np.int32)
    cat_cols = [j for j in range(len(meta)) if kind[j] == 1]
    cont_cols = [j for j in range(len(meta)) if kind[j] == 0]
    if n and cat_cols:
        # training rows of each known categorical cell's option (inf: unknown cell); argmin takes the lowest column
        rarity = np.full((n, len(cat_cols)), np.inf)
        option = np.zeros((n, len(cat_cols)), dtype=np.int64)
        for p, j in enumerate(cat_cols):
            rows = np.nonzero(on[:, j])[0]
            if rows.size == 0:
                continue
            i2s = np.asarray(meta[j]["i2s"], dtype=np.float64)
            order = np.argsort(i2s, kind="stable")
            pos = np.searchsorted(i2s[order], known[rows, j])
            pos = np.minimum(pos, len(i2s) - 1)
            hit = i2s[order][pos] == known[rows, j]
            if not hit.all():
                bad = rows[~hit][0]
                raise ValueError(f"column {j}: value {known[bad, j]!r} (row {int(bad)}) is not among the model's "
                                 "options")
            o = order[pos]
            option[rows, p] = o
            rarity[rows, p] = counts[_span_of(transformer, j)][o]
        pick = np.argmin(rarity, axis=1)
        has = np.isfinite(rarity[np.arange(n), pick])
        drv_span[has] = np.asarray([_span_of(transformer, j) for j in cat_cols], dtype=np.int32)[pick[has]]
        drv_opt[has] = option[np.arange(n), pick][has]
    if n and cont_cols:
        rest = (drv_span < 0) & on[:, cont_cols].any(axis=1)
        first = np.asarray(cont_cols)[np.argmax(on[:, cont_cols], axis=1)]
        for j in np.unique(first[rest]):
            rows = np.nonzero(rest & (first == j))[0]
            mu, sd = mode_tables(transformer, int(j))
            span = _span_of(transformer, int(j))
            z = (known[rows, j][:, None] - mu[None, :]) / sd[None, :]
            w = counts[span][:len(mu)][None, :] * np.exp(-0.5 * z * z) / (sd[None, :] * np.sqrt(2.0 * np.pi))
            w = np.where(np.abs(z) <= 4.0, w, -1.0)
            k = np.argmax(w, axis=1)
            reach = w[np.arange(len(rows)), k] >= 0.0
            drv_span[rows[reach]] = span
            drv_opt[rows[reach]] = k[reach]
    return {"known": known, "mask": mask, "drv_span": drv_span, "drv_opt": drv_opt, "kind": kind, "scale": scale}
