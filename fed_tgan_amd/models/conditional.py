"""Conditional generation requests: "n rows with these category values, inside these ranges".

CTGAN trains its generator on a conditional vector (one option of one softmax span set to 1) and a cross-entropy
that makes it honour the option, but ``sample_zero`` -- and ``CTGANEngine.generate_decoded`` -- draw that vector at
random.  A request fixes it: the **driving** column's requested value goes into the conditional vector of every
generated row, and every requested column (driving or not) is enforced by rejecting, on the device, the rows whose
decoded value differs (the generator is not guaranteed to obey its condition).

``where`` is an ordered mapping from a column name to a spec:

* categorical column, a value or a ``{value: weight}`` mapping; at most one column may carry weights, and it drives.
  ``n`` is apportioned to its values by largest remainder (ties in request order); the table comes back with exactly
  those counts, grouped by value in request order;
* categorical column, a list of values (a **set**): any of these, in the model's own proportions;
* continuous column, ``{"min": a, "max": b}`` (a **range**, either key may be absent): ``lo <= x <= hi`` on the
  decoded value, exact float64 compares, NaN outside.

The driver is the weighted column if there is one, else the first entry.  Under a scalar or weighted driver the ranges
and sets are filters.  When a range or a set drives, the request has one bin, the rows come back in generation order,
and the options of the driving span are drawn by weight: for a range the training rows of a mode times the share of
its Gaussian inside the range (a mode whose reach ``mean +- 4 sd`` misses the range is never drawn), for a set the
training rows of the listed options.  :func:`build_request` resolves names and strings to the device buffers
``CTGANEngine.generate_decoded_where`` and the ``cond_request`` / ``pred_request`` / ``pred_mark`` /
``cond_partition`` ops consume.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, List, Mapping, Sequence, Tuple

import numpy as np
import torch

from ..data.constants import CATEGORICAL, CONTINUOUS, EMPTY

MAX_BINS = 64      # requested values of the driving column (the kernels' bin limit, csrc/kernels/launch.h)
PRED_MAX = 16      # range / set predicates of a request (csrc/kernels/launch.h)
PRED_RANGE, PRED_SET = 0, 1


class ConditionalSamplingError(RuntimeError):
    """``max_passes`` generation passes did not fill every quota.  ``filled`` holds the per-value counts reached (in
    request order), ``quotas`` the counts asked for and ``values`` the requested values; no table is returned."""

    def __init__(self, message: str, filled: Sequence[int], quotas: Sequence[int], values: Sequence = ()):
        super().__init__(message)
        self.filled = [int(x) for x in filled]
        self.quotas = [int(x) for x in quotas]
        self.values = list(values)


@dataclasses.dataclass(frozen=True)
class Range:
    """A resolved range in the decoded (model) space; an open side is -inf / +inf."""
    lo: float
    hi: float


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


def _continuous_error(what: str) -> ValueError:
    return ValueError(f"{what} is continuous; a condition on it is a range {{\"min\": .., \"max\": ..}} (either key "
                      "may be absent), values and weights are for categorical columns")


def parse_range(what: str, spec) -> Tuple[float, float]:
    """(min, max) of a range mapping, an absent key as -inf / +inf; ValueError for anything but a mapping with
    the keys ``min`` and/or ``max``, finite, ``min <= max``."""
    if not isinstance(spec, Mapping) or not spec or not set(spec) <= {"min", "max"}:
        raise _continuous_error(what)
    out = []
    for key, default in (("min", -math.inf), ("max", math.inf)):
        if key not in spec:
            out.append(default)
            continue
        try:
            v = float(spec[key])
        except (TypeError, ValueError):
            raise ValueError(f"{what}: {key} {spec[key]!r} is not a number") from None
        if not math.isfinite(v):
            raise ValueError(f"{what}: {key} must be finite, got {spec[key]!r}")
        out.append(v)
    if out[0] > out[1]:
        raise ValueError(f"{what}: min {out[0]!r} exceeds max {out[1]!r}")
    return out[0], out[1]


def _normal_mass(a: float, b: float) -> float:
    """Phi(b) - Phi(a) for a <= b, from erfc on the side where both are small (no cancellation in a tail)."""
    r2 = math.sqrt(2.0)
    if a > 0:
        return 0.5 * (math.erfc(a / r2) - math.erfc(b / r2))
    if b < 0:
        return 0.5 * (math.erfc(-b / r2) - math.erfc(-a / r2))
    return 1.0 - 0.5 * math.erfc(b / r2) - 0.5 * math.erfc(-a / r2)


def mode_tables(transformer, j: int) -> Tuple[np.ndarray, np.ndarray]:
    """(mu, sd) float64 of continuous column j's valid modes, in the order and with the values of the decode tables."""
    c = list(transformer.cont_index).index(int(j))
    mu, sd = transformer.decode_tables()
    nv = int(np.asarray(transformer.components[c]).sum())
    return np.asarray(mu[c, :nv], dtype=np.float64), np.asarray(sd[c, :nv], dtype=np.float64)


def range_weights(transformer, j: int, lo: float, hi: float, counts_row) -> Tuple[List[int], List[float]]:
    """(reachable modes, their driving weights) of a range on continuous column j: mode k reaches
    [mu_k - 4 sd_k, mu_k + 4 sd_k] (decode clamps alpha to [-1, 1]); a reachable mode weighs
    counts[k] * (Phi((hi - mu_k) / sd_k) - Phi((lo - mu_k) / sd_k))."""
    mu, sd = mode_tables(transformer, j)
    reach, w = [], []
    for k in range(len(mu)):
        if hi < -4.0 * sd[k] + mu[k] or lo > 4.0 * sd[k] + mu[k]:
            continue
        reach.append(k)
        w.append(float(counts_row[k]) * _normal_mass((lo - mu[k]) / sd[k], (hi - mu[k]) / sd[k]))
    return reach, w


def driver_table(options: Sequence[int], weights: Sequence[float]) -> Tuple[List[int], List[float]]:
    """(drv_opt, drv_cum): the options with positive weight, in option order, and their cumulative normalised weights
    ending at exactly 1.0; every weight zero: uniform over the options."""
    pairs = sorted(zip(options, weights))
    if not any(w > 0 for _, w in pairs):
        pairs = [(o, 1.0) for o, _ in pairs]
    pairs = [(o, w) for o, w in pairs if w > 0]
    cum = np.cumsum([w for _, w in pairs]) / float(sum(w for _, w in pairs))
    cum[-1] = 1.0
    return [int(o) for o, _ in pairs], [float(x) for x in cum]


def request_from_codes(transformer, where: Sequence[Tuple[int, object]], n: int, device, labels=None, counts=None,
                       describe=None, names=None) -> Dict:
    """The request buffers from resolved columns: ``where`` = [(output column j, spec), ...].  On a categorical
    column ``spec`` is a label code as ``transformer.meta[j]["i2s"]`` holds them, a ``{code: weight}`` mapping or a
    list of codes (a set); on a continuous one a ``{"min": a, "max": b}`` mapping in the decoded (model) space.
    ``counts``: CondTables.counts, needed when a range or a set drives.  ``describe`` / ``names``: the predicates'
    and columns' printed forms for messages (default: built from the codes and indices)."""
    if not where:
        raise ValueError("an empty condition; use generate_decoded for unconditional rows")
    meta = transformer.meta
    name_of = (lambda j: str(names[j])) if names is not None else (lambda j: str(j))      # noqa: E731
    col_txt = (lambda j: f"column {names[j]!r}") if names is not None else (lambda j: f"column {j}")      # noqa: E731
    seen = set()
    drive = None
    where = list(where)
    for pos, (j, v) in enumerate(where):
        if not 0 <= int(j) < len(meta):
            raise ValueError(f"unknown column index {j}")
        if meta[j]["type"] == CONTINUOUS:
            if not isinstance(v, Range):
                where[pos] = (j, Range(*parse_range(f"column {j}", v)))
        elif isinstance(v, Range):
            raise ValueError(f"column {j} is categorical; a range is for continuous columns")
        if j in seen:
            raise ValueError(f"column {j} is conditioned twice")
        seen.add(j)
        if isinstance(v, Mapping) and meta[j]["type"] != CONTINUOUS:
            if drive is not None:
                raise ValueError("at most one column may carry a {value: weight} mapping")
            drive = pos
    drive = 0 if drive is None else drive

    def option(j, code):
        i2s = list(meta[j]["i2s"])
        if code not in i2s:
            raise ValueError(f"column {j}: value {code!r} is not among the model's options")
        return i2s.index(code)

    def is_pred(v):
        return isinstance(v, (Range, list, tuple))

    for j, v in where:
        if isinstance(v, (list, tuple)):
            if not v:
                raise ValueError(f"column {j}: an empty list of values")
            if len(set(v)) != len(v):
                raise ValueError(f"column {j}: a value is listed twice")
    dj, dv = where[drive]
    pred_drives = is_pred(dv)
    if pred_drives:       # one bin; every entry is a predicate (a scalar: a one-value set)
        items, quotas, bin_opt, fixed = [(0.0, 1.0)], apportion(n, [1.0]), [0], []
        preds = [(j, v if is_pred(v) else [v]) for j, v in where]
    else:
        items = list(dv.items()) if isinstance(dv, Mapping) else [(dv, 1.0)]
        if not items:
            raise ValueError("the driving column requests no value")
        if len(items) > MAX_BINS:
            raise ValueError(f"{len(items)} requested values; the kernels' bin limit is {MAX_BINS}")
        quotas = apportion(n, [w for _, w in items])
        bin_opt = [option(dj, c) for c, _ in items]
        fixed = [(j, v) for pos, (j, v) in enumerate(where) if pos != drive and not is_pred(v)]
        for j, c in fixed:
            option(j, c)
        preds = [(j, v) for j, v in where if is_pred(v)]
    if len(preds) > PRED_MAX:
        raise ValueError(f"{len(preds)} range / set predicates; the limit is {PRED_MAX}")

    # the predicate buffers: ranges carry bounds, sets a byte per label code of their column
    p_kind, p_lo, p_hi, p_off, p_len, lut, auto = [], [], [], [], [], [], []
    for j, v in preds:
        if isinstance(v, Range):
            p_kind.append(PRED_RANGE)
            p_lo.append(float(v.lo))
            p_hi.append(float(v.hi))
            p_off.append(0)
            p_len.append(0)
            auto.append((name_of(j), "range", (float(v.lo), float(v.hi))))
        else:
            for c in v:
                option(j, c)
            codes = list(meta[j]["i2s"])
            if any(float(c) != int(c) or c < 0 for c in codes) or max(codes) >= 1 << 20:
                raise ValueError(f"{col_txt(j)}: a set needs label codes that are integers in [0, 2^20)")
            width = int(max(codes)) + 1
            bits = [0] * width
            for c in v:
                bits[int(c)] = 1
            p_kind.append(PRED_SET)
            p_lo.append(0.0)
            p_hi.append(0.0)
            p_off.append(len(lut))
            p_len.append(width)
            lut += bits
            auto.append((name_of(j), "set", tuple(v)))
    describe = list(describe) if describe is not None else auto

    dev = torch.device(device)
    i32 = lambda v: torch.tensor(list(v), dtype=torch.int32, device=dev)      # noqa: E731
    i64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)      # noqa: E731
    f64 = lambda v: torch.tensor(list(v), dtype=torch.float64, device=dev)    # noqa: E731
    seg = np.concatenate([[0], np.cumsum(quotas)[:-1]]).astype(np.int64)
    if pred_drives and labels is None:
        labels = [describe_predicate(describe[[j for j, _ in preds].index(dj)])]
    req = {
        "drive": i32([_span_of(transformer, dj), dj]),
        "bin_opt": i32(bin_opt), "bin_code": f64(float(c) for c, _ in items),
        "quota": i64(quotas), "filled": torch.zeros(len(items), dtype=torch.int64, device=dev), "seg_off": i64(seg),
        "fixed_j": i32(j for j, _ in fixed), "fixed_code": f64(float(c) for _, c in fixed),
        "stats": torch.zeros(2, dtype=torch.int64, device=dev),
        "pred_j": i32(j for j, _ in preds), "pred_kind": i32(p_kind), "pred_lo": f64(p_lo), "pred_hi": f64(p_hi),
        "pred_lut_off": i32(p_off), "pred_lut_len": i32(p_len),
        "pred_lut": torch.tensor(lut, dtype=torch.uint8, device=dev),
        "pred_stats": torch.zeros(2 + PRED_MAX, dtype=torch.int64, device=dev),
        # host-side description (not read by the ops)
        "n": int(n), "quotas": list(quotas), "values": list(labels) if labels is not None else [c for c, _ in items],
        "predicates": describe,
    }
    if pred_drives:
        span = _span_of(transformer, dj)
        if counts is None:
            raise ValueError("a range or a set that drives needs the span counts (counts=CondTables.counts)")
        row = np.asarray(counts, dtype=np.float64)[span]
        if isinstance(dv, Range):
            opts, w = range_weights(transformer, dj, dv.lo, dv.hi, row)
            if not opts:
                mu, sd = mode_tables(transformer, dj)
                shown = describe[[j for j, _ in preds].index(dj)][2]
                raise ValueError(f"{col_txt(dj)}: no mode of the model reaches the range [{shown[0]!r}, "
                                 f"{shown[1]!r}] (decoded [{dv.lo!r}, {dv.hi!r}]); the modes reach from "
                                 f"{float((mu - 4.0 * sd).min())!r} to {float((mu + 4.0 * sd).max())!r}")
        else:
            opts = [option(dj, c) for c in dv]
            w = [float(row[o]) for o in opts]
        d_opt, d_cum = driver_table(opts, w)
        req.update({"drv": i32([span, dj]), "drv_opt": i32(d_opt), "drv_cum": f64(d_cum)})
    return req


def describe_predicate(d) -> str:
    """One predicate of ``request["predicates"]`` as text: ``serror_rate in [0.9, 1.0]``, ``protocol_type in (tcp, udp)``."""
    name, kind, val = d
    if kind == "range":
        return f"{name} in [{val[0]!r}, {val[1]!r}]"
    return f"{name} in ({', '.join(str(v) for v in val)})"


def build_request(transformer, meta: dict, vocabs, where: Mapping, n: int, device, counts=None) -> Dict:
    """Resolve ``where`` ({column name: spec}, names as in ``meta["columns"]``, values and bounds as the CSV prints
    them; the specs: this module's docstring) against the table meta, the label vocabularies and the model's options
    into request buffers on ``device``.  The bounds of a column in ``meta["non_negative_cols"]`` are brought to the
    decoded space (log1p; ``min <= 0``: no lower bound; ``max < 0``: an error).  ``counts``: CondTables.counts, needed
    when a range or a set drives.  Raises ValueError for an unknown column, a value or weights on a continuous column,
    a value outside the vocabulary or the model's options, negative weights or weights summing to zero, more values
    than the kernels' bin limit, a malformed range or set, more than PRED_MAX predicates, and a driving range no mode
    reaches."""
    if not isinstance(where, Mapping) or not where:
        raise ValueError("where must be a non-empty mapping {column: value | {value: weight}}")
    names = [c["column_name"] for c in meta["columns"]]
    nonneg = set(meta.get("non_negative_cols") or [])
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

    resolved, labels, describe = [], None, []
    for name, v in where.items():
        if name not in names:
            raise ValueError(f"unknown column {name!r}")
        j = names.index(name)
        if j not in voc_of or transformer.meta[j]["type"] == CONTINUOUS:
            lo, hi = parse_range(f"column {name!r}", v)
            describe.append((name, "range", (lo, hi)))
            if name in nonneg:      # the decoded table holds log1p values; the CSV never prints below -0.0
                if hi < 0:
                    raise ValueError(f"column {name!r} is non-negative; max {hi!r} lies below every printed value")
                lo = -math.inf if lo <= 0 else math.log1p(lo)
                hi = math.log1p(hi) if math.isfinite(hi) else hi
            resolved.append((j, Range(lo, hi)))
        elif isinstance(v, Mapping):
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
        elif isinstance(v, (list, tuple)):
            if not v:
                raise ValueError(f"column {name!r}: an empty list of values")
            codes = []
            for val in v:
                c = code_of(j, val)
                if c in codes:
                    raise ValueError(f"column {name!r}: value {val!r} is listed twice")
                codes.append(c)
            resolved.append((j, codes))
            describe.append((name, "set", tuple(str(x) for x in v)))
        else:
            resolved.append((j, code_of(j, v)))
    weighted = [pos for pos, (_, v) in enumerate(resolved) if isinstance(v, Mapping)]
    drive_spec = resolved[weighted[0] if weighted else 0][1]
    if isinstance(drive_spec, (Range, list)):
        # a predicate drives: the scalars become one-value sets, described in request order like the rest
        describe, labels = [], None
        for (name, v), (j, r) in zip(where.items(), resolved):
            if isinstance(r, Range):
                lo, hi = parse_range(f"column {name!r}", v)
                describe.append((name, "range", (lo, hi)))
            else:
                describe.append((name, "set", tuple(str(x) for x in v) if isinstance(v, (list, tuple)) else (str(v),)))
    elif labels is None:
        labels = [str(next(iter(where.values())))]
    try:
        return request_from_codes(transformer, resolved, n, device, labels=labels, counts=counts, describe=describe,
                                  names=names)
    except ValueError as e:
        raise ValueError(f"{e} (columns: {[names[j] for j, _ in resolved]})") from None


def parse_where(pairs: Sequence[str] = (), where_json: str | None = None, ranges: Sequence[str] = ()) -> Dict:
    """The command line's ``-where COL=VALUE`` (repeatable), ``-where_json`` and ``-where_range COL=LO:HI``
    (repeatable, either side may be empty) into one ordered mapping."""
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
    for p in ranges or ():
        k, sep, v = p.partition("=")
        if not sep or not k or v.count(":") != 1:
            raise ValueError(f"-where_range takes COL=LO:HI, got {p!r}")
        spec = {}
        for key, text in zip(("min", "max"), v.split(":")):
            if text.strip():
                try:
                    spec[key] = float(text)
                except ValueError:
                    raise ValueError(f"-where_range {p!r}: {text!r} is not a number") from None
        if not spec:
            raise ValueError(f"-where_range {p!r}: give at least one bound")
        where[k] = spec
    return where
