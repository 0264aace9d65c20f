"""Shared fixtures: a small encoded Intrusion-schema table and an autograd oracle of one step."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

# (the table fixture lives in the package: __graft_entry__.smoke() uses it too)
from fed_tgan_amd.data.demo import small_table  # noqa: F401


def d_forward_masked(X, Ws, bs, masks, v, e, slope=0.2):
    """Packed D forward with explicit dropout keep-masks (values 0 / 2)."""
    h = X
    for W, b, M in zip(Ws, bs, masks):
        h = F.leaky_relu(h @ W.t() + b, slope) * M
    return h @ v.view(-1, 1) + e


def keep_mask_from_ms(ms, pre, slope=0.2):
    s = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope))
    return ms / s


def table_spans():
    """(transformer, encoded matrix, activation spans, conditional spans) of the small table."""
    _, _, _, _, _, _, tr, X = small_table()
    spans = [(int(s), int(w), int(k)) for s, w, k in zip(tr.layout.start, tr.layout.width, tr.layout.kind)]
    cond = [(int(s), int(w)) for s, w in zip(tr.layout.cond_start, tr.layout.cond_width)]
    return tr, X, spans, cond


def wide_spans(D_min=1500, seed=0):
    """Synthetic layout wider than the register-prefetch path (D > 512): tanh + softmax spans,
    some wider than a wave."""
    rng = np.random.default_rng(seed)
    spans, cond, pos = [], [], 0
    while pos < D_min:
        spans.append((pos, 1, 0))
        pos += 1
        w = int(rng.choice([2, 3, 7, 13, 70, 130]))
        spans.append((pos, w, 1))
        cond.append((pos, w))
        pos += w
    return spans, cond, pos
