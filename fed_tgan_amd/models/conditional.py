"""Conditional generation requests: "n rows with these category values".

CTGAN trains its generator on a conditional vector (one option of one softmax span set to 1) and a cross-entropy
that makes it honour the option, but ``sample_zero`` -- and ``CTGANEngine.generate_decoded`` -- draw that vector at
random.  A request fixes it: the **driving** column's requested value goes into the conditional vector of every
generated row, and every requested column (driving or not) is enforced by rejecting, on the device, the rows whose
decoded value differs (the generator is not guaranteed to obey its condition).

``where`` is an ordered mapping from a categorical column name to a value or a ``{value: weight}`` mapping; at most
one column may carry weights, and it drives (else the first column does).  ``n`` is apportioned to the driving
column's values by largest remainder (ties in request order); the table comes back with exactly those counts,
grouped by value in request order.  :func:`build_request` resolves names and strings to the device buffers
``CTGANEngine.generate_decoded_where`` and the ``cond_request`` / ``cond_partition`` ops consume.
"""
from __future__ import annotations

from typing import Dict, List, Mapping, Sequence, Tuple

import numpy as np
import torch

from ..data.constants import CATEGORICAL, CONTINUOUS, EMPTY

MAX_BINS = 64      # requested values of the driving column (the kernels' bin limit, csrc/kernels/launch.h)


class ConditionalSamplingError(RuntimeError):
    """``max_passes`` generation passes did not fill every quota.  ``filled`` holds the per-value counts reached (in
    request order), ``quotas`` the counts asked for and ``values`` the requested values; no table is returned."""

    def __init__(self, message: str, filled: Sequence[int], quotas: Sequence[int], values: Sequence = ()):
        super().__init__(message)
        self.filled = [int(x) for x in filled]
        self.quotas = [int(x) for x in quotas]
        self.values = list(values)


def apportion(n: int, weights: Sequence[float]) -> List[int]:
    """Largest-remainder split of ``n`` over ``weights`` (ties go to the earlier entry): [1, 1, 1], 100 -> 34 33 33."""
    w = [float(x) for x in weights]
    if not w or any(not np.isfinite(x) or x < 0 for x in w):
        raise ValueError(f"weights must be finite and non-negative, got {list(weights)}")
    tot = sum(w)
    if tot <= 0:
        raise ValueError("weights sum to zero")
    n = int(n)
    if n < 0:
        raise ValueError("n must be non-negative")
    share = [n * x / tot for x in w]
    base = [int(np.floor(s)) for s in share]
    order = sorted(range(len(w)), key=lambda i: (-(share[i] - base[i]), i))
    for i in order[:n - sum(base)]:
        base[i] += 1
    return base


def _span_of(transformer, j: int) -> int:
    """The conditional-vector span of output column j: every column contributes exactly one softmax span (a
    continuous column its mode indicator, a categorical one its one-hot)."""
    if transformer.layout.n_col != len(transformer.meta):
        raise ValueError("the span layout does not hold one conditional span per column")
    return int(j)


def request_from_codes(transformer, where: Sequence[Tuple[int, object]], n: int, device, labels=None) -> Dict:
    """The request buffers from resolved columns: ``where`` = [(output column j, code | {code: weight}), ...] with
    label codes as ``transformer.meta[j]["i2s"]`` holds them."""
    if not where:
        raise ValueError("an empty condition; use generate_decoded for unconditional rows")
    meta = transformer.meta
    seen = set()
    drive = None
    for pos, (j, v) in enumerate(where):
        if not 0 <= int(j) < len(meta):
            raise ValueError(f"unknown column index {j}")
        if meta[j]["type"] == CONTINUOUS:
            raise ValueError(f"column {j} is continuous; conditions are on categorical columns")
        if j in seen:
            raise ValueError(f"column {j} is conditioned twice")
        seen.add(j)
        if isinstance(v, Mapping):
            if drive is not None:
                raise ValueError("at most one column may carry a {value: weight} mapping")
            drive = pos
    drive = 0 if drive is None else drive

    def option(j, code):
        i2s = list(meta[j]["i2s"])
        if code not in i2s:
            raise ValueError(f"column {j}: value {code!r} is not among the model's options")
        return i2s.index(code)

    dj, dv = where[drive]
    items = list(dv.items()) if isinstance(dv, Mapping) else [(dv, 1.0)]
    if not items:
        raise ValueError("the driving column requests no value")
    if len(items) > MAX_BINS:
        raise ValueError(f"{len(items)} requested values; the kernels' bin limit is {MAX_BINS}")
    quotas = apportion(n, [w for _, w in items])
    bin_opt = [option(dj, c) for c, _ in items]
    fixed = [(j, v) for pos, (j, v) in enumerate(where) if pos != drive]
    for j, c in fixed:
        option(j, c)
    dev = torch.device(device)
    i32 = lambda v: torch.tensor(list(v), dtype=torch.int32, device=dev)      # noqa: E731
    i64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)      # noqa: E731
    f64 = lambda v: torch.tensor(list(v), dtype=torch.float64, device=dev)    # noqa: E731
    seg = np.concatenate([[0], np.cumsum(quotas)[:-1]]).astype(np.int64)
    return {
        "drive": i32([_span_of(transformer, dj), dj]),
        "bin_opt": i32(bin_opt), "bin_code": f64(float(c) for c, _ in items),
        "quota": i64(quotas), "filled": torch.zeros(len(items), dtype=torch.int64, device=dev), "seg_off": i64(seg),
        "fixed_j": i32(j for j, _ in fixed), "fixed_code": f64(float(c) for _, c in fixed),
        "stats": torch.zeros(2, dtype=torch.int64, device=dev),
        # host-side description (not read by the ops)
        "n": int(n), "quotas": list(quotas), "values": list(labels) if labels is not None else [c for c, _ in items],
    }


def build_request(transformer, meta: dict, vocabs, where: Mapping, n: int, device) -> Dict:
    """Resolve ``where`` ({column name: value | {value: weight}}, names as in ``meta["columns"]``, values as the CSV
    prints them) against the table meta, the label vocabularies and the model's options into request buffers on
    ``device``.  Raises ValueError for an unknown or continuous column, a value outside the vocabulary or the model's
    options, negative weights or weights summing to zero, and more values than the kernels' bin limit."""
    if not isinstance(where, Mapping) or not where:
        raise ValueError("where must be a non-empty mapping {column: value | {value: weight}}")
    names = [c["column_name"] for c in meta["columns"]]
    voc_of, cursor = {}, 0
    for j, c in enumerate(meta["columns"]):
        if c["type"] == CATEGORICAL:
            voc_of[j] = vocabs[cursor]
            cursor += 1

    def code_of(j, value):
        printed = [(" " if s == EMPTY else s) for s in voc_of[j].tolist()]
        s = str(value)
        if s in printed:
            return printed.index(s)
        if s == EMPTY and " " in printed:
            return printed.index(" ")
        raise ValueError(f"column {names[j]!r}: value {value!r} is not in the vocabulary")

    resolved, labels = [], None
    for name, v in where.items():
        if name not in names:
            raise ValueError(f"unknown column {name!r}")
        j = names.index(name)
        if j not in voc_of or transformer.meta[j]["type"] == CONTINUOUS:
            raise ValueError(f"column {name!r} is continuous; conditions are on categorical columns")
        if isinstance(v, Mapping):
            if len(v) > MAX_BINS:
                raise ValueError(f"column {name!r}: {len(v)} requested values; the kernels' bin limit is {MAX_BINS}")
            codes = {}
            for val, w in v.items():
                c = code_of(j, val)
                if c in codes:
                    raise ValueError(f"column {name!r}: value {val!r} is requested twice")
                codes[c] = w
            resolved.append((j, codes))
            labels = [str(x) for x in v]
        else:
            resolved.append((j, code_of(j, v)))
    if labels is None:
        labels = [str(next(iter(where.values())))]
    try:
        return request_from_codes(transformer, resolved, n, device, labels=labels)
    except ValueError as e:
        raise ValueError(f"{e} (columns: {[names[j] for j, _ in resolved]})") from None


def parse_where(pairs: Sequence[str] = (), where_json: str | None = None) -> Dict:
    """The command line's ``-where COL=VALUE`` (repeatable) and ``-where_json`` into one ordered mapping."""
    import json
    where: Dict = {}
    if where_json:
        obj = json.loads(where_json)
        if not isinstance(obj, dict):
            raise ValueError("-where_json must be a JSON object")
        where.update(obj)
    for p in pairs or ():
        if "=" not in p:
            raise ValueError(f"-where takes COL=VALUE, got {p!r}")
        k, v = p.split("=", 1)
        where[k] = v
    return where
