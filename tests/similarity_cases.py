"""Shared cases of the similarity-evaluator tests (test_similarity_device.py on the CPU, test_hip_similarity.py on
the GPU): small real / fake tables of the Intrusion schema (data/synthetic.py) with the reference's corner cases
planted in them, and the CPU evaluator's answer for each, computed once.

A case is (real frame as a CSV reader delivers it, decoded fake values [m, n_cols] float64 as generate_decoded
returns them, meta, vocabs, categorical column names).  The expected per-column frame comes from
eval.similarity.column_similarity on the CSVs of both tables.
"""
from __future__ import annotations

import functools
import io

import numpy as np
import pandas as pd

from fed_tgan_amd.data.constants import CATEGORICAL
from fed_tgan_amd.data.decode import decode_frame
from fed_tgan_amd.data.demo import small_table
from fed_tgan_amd.eval.similarity import column_similarity, stat_sim

W1_TOL = 1e-10       # <= 1e5 fp64 terms of magnitude <= 1: ~1e-11
JSD_TOL = 1e-9       # where the reference value is >= JSD_FLOOR
JSD_FLOOR = 1e-3
JSD_ZERO_TOL = 1e-7  # below the floor the square root amplifies rounding: both values only have to be this small

CASES = ("mixed", "plain", "identical")


def through_csv(df: pd.DataFrame) -> pd.DataFrame:
    buf = io.StringIO()
    df.to_csv(buf, index=False)
    buf.seek(0)
    return pd.read_csv(buf)


@functools.lru_cache(maxsize=None)
def case(name: str):
    spec, df, tp, meta, vocabs, enc, tr, X = small_table()
    names = [c["column_name"] for c in meta["columns"]]
    cats = [c["column_name"] for c in meta["columns"] if c["type"] == CATEGORICAL]
    conts = [n for n in names if n not in cats]
    nonneg = [n for n in conts if n in meta["non_negative_cols"]]
    plain = [n for n in conts if n not in meta["non_negative_cols"]]
    if name == "identical":
        real, vals = df.iloc[:300].copy(), enc[:300].astype(np.float64).copy()
    elif name == "plain":
        real, vals = df.iloc[:500].copy(), enc[900:1200].astype(np.float64).copy()
    elif name == "mixed":
        real, vals = df.iloc[:700].copy(), enc[700:1100].astype(np.float64).copy()
        # a fake column with no real category (1.0); the real value is outside the vocabulary (an extra count slot)
        real[cats[0]] = "only_in_real"
        # a real category the fake table misses (the double-count quirk): the fake column drops its most common code
        j = names.index(cats[1])
        codes, cnt = np.unique(vals[:, j], return_counts=True)
        assert len(codes) >= 2
        top = codes[np.argmax(cnt)]
        vals[vals[:, j] == top, j] = codes[codes != top][0]
        # a fake-only category: the real column loses every row of one value the fake table has
        j = names.index(cats[2])
        fake_strings = set(vocabs[2].inverse_transform(vals[:, j].astype(int)).tolist())
        rc = real[cats[2]].astype(str).value_counts()
        drop = [s for s in rc.index[1:] if s in fake_strings]
        assert drop
        real.loc[real[cats[2]].astype(str) == drop[0], cats[2]] = rc.index[0]
        # a constant real column (scale 1) and fake values outside the real range
        real[plain[0]] = 5.0
        vals[:, names.index(plain[1])] *= 3.0
        vals[:7, names.index(plain[1])] = -11.0
        # a non-negative column with one code so negative that exp underflows: the CSV field is blank
        vals[3, names.index(nonneg[0])] = -800.0
    else:
        raise KeyError(name)
    real = through_csv(real.reset_index(drop=True))
    return real, np.ascontiguousarray(vals), meta, vocabs, cats


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """(column_similarity frame, (avg_jsd, avg_wd)) of the CPU evaluator on the case's CSVs"""
    real, vals, meta, vocabs, cats = case(name)
    fake = through_csv(decode_frame(vals.copy(), meta, vocabs))
    return column_similarity(real, fake, cats), stat_sim(real, fake, cats)


def assert_scores(got_cols: pd.DataFrame, got_avg, want_cols: pd.DataFrame, want_avg, what: str = ""):
    """the tolerances of both test files: W1 abs <= 1e-10; JSD abs <= 1e-9 where the reference is >= 1e-3, else
    both <= 1e-7"""
    assert got_cols["column"].tolist() == want_cols["column"].tolist(), what
    assert got_cols["metric"].tolist() == want_cols["metric"].tolist(), what
    for col, metric, g, w in zip(want_cols["column"], want_cols["metric"], got_cols["value"], want_cols["value"]):
        if np.isnan(w):
            assert np.isnan(g), (what, col, g, w)
        elif metric == "WD":
            assert abs(g - w) <= W1_TOL, (what, col, g, w)
        elif w >= JSD_FLOOR:
            assert abs(g - w) <= JSD_TOL, (what, col, g, w)
        else:
            assert g <= JSD_ZERO_TOL and w <= JSD_ZERO_TOL, (what, col, g, w)
    gj, gw = got_avg
    wj, ww = want_avg
    assert abs(gw - ww) <= W1_TOL or (np.isnan(gw) and np.isnan(ww)), (what, gw, ww)
    assert abs(gj - wj) <= (JSD_TOL if all(v >= JSD_FLOOR for v in want_cols["value"][want_cols["metric"] == "JSD"])
                            else JSD_ZERO_TOL), (what, gj, wj)
