"""Inputs of tests/test_hip_rng.py built in plain numpy, so that the conditions the GPU tests rest on (the share of
near-ties left out of the argmax checks) can be asserted on the CPU from the oracle alone (tests/test_rng_oracle.py),
and the oracle's answers, computed once per case and shared."""
from __future__ import annotations

import functools

import numpy as np

import rng_cases as rc
from helpers import table_spans, wide_spans

STEPS = (0, 5, (1 << 32) + 5)          # the last: the key's high-word path
TAU = 0.2
NEAR_TIE = 1e-3                        # argmax checks leave out spans whose top two perturbed logits are closer
ACT_ROWS = 64
ACT_SEED, ACT_STREAM_ID, SLERP_STREAM_ID = 4242, 2, 3
ACT_COND = 45                          # conditional columns after the activation's in the fused slerp's rows
ACT_SLERP_ROWS = 40
# case -> (D_min of wide_spans or None for the small table's layout, the step it runs at)
ACT_CASES = {"table": (None, STEPS[0]), "wide300": (300, STEPS[1]), "wide2300": (2300, STEPS[2]),
             "wide7000": (7000, STEPS[1])}

DEC_ROWS = 70
DEC_SEED, DEC_STREAM_ID = 777, 23
# (kind, start, width): a span wider than 64, a continuous column (tanh unit + 5 modes) and a width-5 span next to it
DEC_CUSTOM = ((1, 0, 70), (0, 70, 5), (1, 76, 5), (1, 81, 3))
DEC_CASES = {"table_zero": STEPS[0], "table_x3": STEPS[2], "custom_zero": STEPS[1], "custom_x3": STEPS[0]}


def normal32(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


# ----------------------------------------------------------------------------- activation
@functools.lru_cache(maxsize=None)
def act_case(name):
    """(spans, D, fp32 logits [ACT_ROWS, D], step)"""
    d_min, step = ACT_CASES[name]
    if d_min is None:
        _, X, spans, _ = table_spans()
        D = int(X.shape[1])
    else:
        spans, _, D = wide_spans(D_min=d_min, seed=4)
    return spans, D, normal32((ACT_ROWS, D), 52, 2.0), step


@functools.lru_cache(maxsize=None)
def act_oracle(name):
    """(fp64 activation, per softmax span: (start, width, oracle argmax [R], kept [R] = no near-tie))"""
    spans, D, logits, step = act_case(name)
    out, pert = rc.activate(logits, spans, TAU, ACT_SEED, ACT_STREAM_ID * 16, step)
    soft = [(s, w, pert[:, s:s + w].argmax(1), rc.top_two_gap(pert[:, s:s + w]) >= NEAR_TIE)
            for s, w, k in spans if k != 0]
    return out, soft


# ----------------------------------------------------------------------------- decode
def table_decode_cols():
    """(kind, start, width) per output column of the small table (models/generation.py set_generation_tables)"""
    tr, X, _, _ = table_spans()
    cols, pos, c = [], 0, 0
    for m in tr.meta:
        if m["type"] == "continuous":
            nv = int(tr.components[c].sum())
            cols.append((0, pos, nv))
            pos += 1 + nv
            c += 1
        else:
            cols.append((1, pos, int(m["size"])))
            pos += int(m["size"])
    assert pos == X.shape[1]
    return tuple(cols), pos


@functools.lru_cache(maxsize=None)
def dec_case(name):
    """(cols, D, fp32 logits [DEC_ROWS, D], step)"""
    layout, kind = name.split("_")
    cols, D = table_decode_cols() if layout == "table" else (DEC_CUSTOM, 84)
    logits = np.zeros((DEC_ROWS, D), dtype=np.float32) if kind == "zero" else normal32((DEC_ROWS, D), 120, 3.0)
    return cols, D, logits, DEC_CASES[name]


@functools.lru_cache(maxsize=None)
def dec_oracle(name):
    """(argmax [R, n_cols], kept [R, n_cols])"""
    cols, D, logits, step = dec_case(name)
    choice, gap = rc.decode_choice(logits, cols, DEC_SEED, DEC_STREAM_ID * 16, step)
    return choice, gap >= NEAR_TIE


def near_tie_shares():
    """(case, share of spans / cells the argmax checks leave out) for every case above"""
    res = []
    for name in ACT_CASES:
        kept = np.stack([k for _, _, _, k in act_oracle(name)[1]])
        res.append(("act_" + name, 1.0 - kept.mean()))
    for name in DEC_CASES:
        res.append(("dec_" + name, 1.0 - dec_oracle(name)[1].mean()))
    return res
