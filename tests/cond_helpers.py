"""Shared pieces of the conditional-generation tests (CPU and HIP): hand-made requests, the wired generator and the
checks of a returned table."""
from __future__ import annotations

import numpy as np
import torch


def names(meta):
    return [c["column_name"] for c in meta["columns"]]


def code(vocabs, column, value):
    v = [x for x in vocabs if x.column_name == column][0]
    return v.tolist().index(value)


def make_request(quota, filled, drive_j, codes, fixed=(), span=0, bin_opt=None, device="cpu"):
    """Request buffers (ops cond_request / cond_partition) from plain lists."""
    nb = len(quota)
    seg = np.concatenate([[0], np.cumsum(quota)[:-1]]).astype(np.int64)
    t = lambda v, dt: torch.tensor(list(v), dtype=dt, device=device)      # noqa: E731
    return {"drive": t([span, drive_j], torch.int32),
            "bin_opt": t(bin_opt if bin_opt is not None else range(nb), torch.int32),
            "bin_code": t(codes, torch.float64),
            "quota": t(quota, torch.int64), "filled": t(filled, torch.int64), "seg_off": t(seg, torch.int64),
            "fixed_j": t([j for j, _ in fixed], torch.int32), "fixed_code": t([c for _, c in fixed], torch.float64),
            "stats": torch.zeros(2, dtype=torch.int64, device=device)}


def request_to(req, device):
    return {k: (v.to(device).clone() if torch.is_tensor(v) else v) for k, v in req.items()}


def wire_generator(eng, tr):
    """G.out copies the conditional vector onto the categorical logits with weight 60: the Gumbel noise lies in about
    (-3.8, 16.2) (u clamped to [1e-20, 1 - 1e-7]), so the requested option wins the argmax with certainty."""
    lay = tr.layout
    W, b = eng.p["G.out.W"], eng.p["G.out.b"]
    with torch.no_grad():
        W.zero_()
        b.zero_()
        in_dim, C = W.shape[1], lay.n_opt
        for c, m in enumerate(tr.meta):
            if m["type"] == "continuous":
                continue
            for k in range(int(lay.cond_width[c])):
                W[int(lay.cond_start[c]) + k, in_dim - C + int(lay.cond_offset[c]) + k] = 60.0


def check_table(tab, req, meta, vocabs, where):
    """Exact per-value counts, grouped in request order; every requested column carries its value."""
    cols = names(meta)
    tab = tab.cpu().numpy()
    assert tab.shape == (req["n"], len(cols))
    dj = req["drive"].tolist()[1]
    pos = 0
    for c, q in zip(req["bin_code"].tolist(), req["quotas"]):
        assert (tab[pos:pos + q, dj] == c).all()
        pos += q
    for col, v in where.items():
        if not isinstance(v, dict):
            assert (tab[:, cols.index(col)] == code(vocabs, col, v)).all()
