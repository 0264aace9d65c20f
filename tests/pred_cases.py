"""Shared pieces of the predicate tests (CPU and HIP): hand-made predicate buffers, random decoded passes with NaN
cells and stray codes, the generator wired on its mode indicators, and the engine scenarios both backends run."""
from __future__ import annotations

import math

import numpy as np
import torch

from fed_tgan_amd.models.conditional import PRED_MAX, build_request
from fed_tgan_amd.models.samplers import CondTables
from cond_helpers import names
from helpers import small_table

RANGE, SET = 0, 1
SERROR = {"serror_rate": {"min": 0.9, "max": 1.0}}
TWO_RANGES = {"serror_rate": {"min": 0.9, "max": 1.0}, "src_bytes": {"min": 100, "max": 1000}}
CLASS_THEN_RANGE = {"class": {"back.": 2, "satan.": 1}, "serror_rate": {"min": 0.9, "max": 1.0}}


def counts():
    _, _, _, _, _, _, tr, X = small_table()
    return CondTables.from_encoded(X, tr.layout).counts


def request(where, n, device="cpu"):
    _, _, _, meta, vocabs, _, tr, _ = small_table()
    return build_request(tr, meta, vocabs, where, n, device, counts=counts())


def make_preds(preds, device="cpu"):
    """Predicate buffers from [(column, RANGE, lo, hi) | (column, SET, [allowed bytes])]."""
    j, kind, lo, hi, off, ln, lut = [], [], [], [], [], [], []
    for p in preds:
        j.append(p[0])
        kind.append(p[1])
        if p[1] == RANGE:
            lo.append(p[2]), hi.append(p[3]), off.append(0), ln.append(0)
        else:
            lo.append(0.0), hi.append(0.0), off.append(len(lut)), ln.append(len(p[2]))
            lut += list(p[2])
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=device)      # noqa: E731
    return {"pred_j": t(j, torch.int32), "pred_kind": t(kind, torch.int32), "pred_lo": t(lo, torch.float64),
            "pred_hi": t(hi, torch.float64), "pred_lut_off": t(off, torch.int32), "pred_lut_len": t(ln, torch.int32),
            "pred_lut": t(lut, torch.uint8), "pred_stats": torch.zeros(2 + PRED_MAX, dtype=torch.int64, device=device)}


def to_device(req, device):
    return {k: (v.to(device).clone() if torch.is_tensor(v) else v) for k, v in req.items()}


def mark_case(m, n_cols, P, seed):
    """(predicate buffers, decoded pass, targets): mixed kinds over random columns; cells are small integers (codes)
    on set columns with a share of non-integers, negatives, codes past the table, NaN and inf; a quarter of the
    targets are already cleared."""
    g = torch.Generator().manual_seed(seed)
    out = torch.rand(m, n_cols, generator=g, dtype=torch.float64) * 4.0 - 1.0
    preds = []
    for k in range(P):
        j = int(torch.randint(0, n_cols, (1,), generator=g))
        if k % 2 == 0:
            lo, hi = sorted((torch.rand(2, generator=g, dtype=torch.float64) * 4.0 - 1.0).tolist())
            lo = -math.inf if k % 6 == 2 else lo - 1.5
            hi = math.inf if k % 6 == 4 else hi + 1.5
            preds.append((j, RANGE, lo, hi))
        else:
            width = 3 + k % 4          # codes are 0..3: the narrow tables also meet codes past their end
            bits = (torch.rand(width, generator=g) < 0.9).to(torch.uint8).tolist()
            preds.append((j, SET, bits))
    set_cols = sorted({p[0] for p in preds if p[1] == SET})
    for j in set_cols:      # codes, with stray ones
        code = torch.randint(0, 4, (m,), generator=g).double()
        r = torch.rand(m, generator=g)
        code = torch.where(r < 0.02, code + 0.5, code)
        code = torch.where((r >= 0.02) & (r < 0.04), torch.full_like(code, 9.0), code)
        code = torch.where((r >= 0.04) & (r < 0.05), torch.full_like(code, -1.0), code)
        out[:, j] = code
    r = torch.rand(m, n_cols, generator=g)
    out = torch.where(r < 0.01, torch.full_like(out, math.nan), out)
    out = torch.where((r >= 0.01) & (r < 0.015), torch.full_like(out, math.inf), out)
    tgt = torch.where(torch.rand(m, generator=g) < 0.25, -1, 0).to(torch.int32)
    return make_preds(preds), out.contiguous(), tgt


def wire_generator_modes(eng, tr):
    """G.out copies the conditional vector onto the logits of its span with weight 60 -- the one-hot of a categorical
    column and the mode indicator of a continuous one -- and leaves every alpha logit 0: a row decodes to exactly
    the mean of the mode (or to the option) it was conditioned on; a span the condition does not name answers at
    random."""
    lay = tr.layout
    W, b = eng.p["G.out.W"], eng.p["G.out.b"]
    with torch.no_grad():
        W.zero_()
        b.zero_()
        in_dim, C = W.shape[1], lay.n_opt
        for c in range(len(tr.meta)):
            for k in range(int(lay.cond_width[c])):
                W[int(lay.cond_start[c]) + k, in_dim - C + int(lay.cond_offset[c]) + k] = 60.0


def mode_mean(tr, column, k):
    """The decode table's mean of valid mode k of a continuous column, as float64."""
    _, _, _, meta, _, _, _, _ = small_table()
    j = names(meta).index(column)
    mu, _ = tr.decode_tables()
    return float(mu[list(tr.cont_index).index(j), k])


def inside(tab, req):
    """Every row of a returned table satisfies every predicate of its request, in the decoded space."""
    tab = tab.cpu()
    ok = torch.ones(tab.shape[0], dtype=torch.bool)
    lut = req["pred_lut"].cpu()
    for j, kind, lo, hi, off, ln in zip(req["pred_j"].tolist(), req["pred_kind"].tolist(), req["pred_lo"].tolist(),
                                        req["pred_hi"].tolist(), req["pred_lut_off"].tolist(),
                                        req["pred_lut_len"].tolist()):
        v = tab[:, j]
        if kind == RANGE:
            ok &= (v >= lo) & (v <= hi)
        else:
            ok &= (v == v.trunc()) & (v >= 0) & (v < ln)
            ok &= lut[off + v.clamp(0, ln - 1).long()] != 0
    return bool(ok.all())


# ----------------------------------------------------------------------------- engine scenarios (either backend)
def scenario_wired_range(eng, tr, device, **kw):
    """serror_rate in [0.9, 1.0] drives a wired generator: the rejected rows are the ones that drew mode 2."""
    req = request(SERROR, 300, device)
    tab = eng.generate_decoded_where(300, req, chunk=128, **kw)
    lc = eng.last_conditional
    _, _, _, meta, _, _, _, _ = small_table()
    js = names(meta).index("serror_rate")
    assert tab.shape == (300, len(meta["columns"]))
    assert bool((tab[:, js] == mode_mean(tr, "serror_rate", 0)).all())
    assert lc["filled"] == [300] and lc["generated"] == lc["passes"] * 128
    (p,) = lc["predicates"]
    assert p["column"] == "serror_rate" and p["tested"] == lc["generated"]
    assert lc["kept"] >= lc["generated"] - p["rejected"]
    assert lc["passes"] <= 4            # a rejected row drew mode 2: 0.13 / 189 of the draws
    return tab


def scenario_wired_filter(eng, tr, device, **kw):
    """The same range as a filter behind a weighted class: counts grouped as today, every row inside the range."""
    _, _, _, meta, vocabs, _, _, _ = small_table()
    req = request(CLASS_THEN_RANGE, 300, device)
    tab = eng.generate_decoded_where(300, req, chunk=128, **kw)
    lc = eng.last_conditional
    jc = names(meta).index("class")
    codes = req["bin_code"].tolist()
    t = tab.cpu()
    assert lc["filled"] == [200, 100]
    assert bool((t[:200, jc] == codes[0]).all()) and bool((t[200:, jc] == codes[1]).all())
    assert inside(tab, req)
    (p,) = lc["predicates"]
    assert p["tested"] == lc["generated"] and p["rejected"] == lc["generated"] - lc["kept"]
    return tab


def scenario_random_init(eng, tr, device, **kw):
    """Two ranges on a random-init generator: several passes, exactly n rows, every row inside both."""
    req = request(TWO_RANGES, 300, device)
    tab = eng.generate_decoded_where(300, req, chunk=1024, **kw)
    lc = eng.last_conditional
    assert tab.shape[0] == 300 and inside(tab, req)
    assert bool(torch.isfinite(tab).all())
    assert lc["filled"] == [300] and 300 <= lc["kept"] <= lc["generated"] == lc["passes"] * 1024
    rej = [p["rejected"] for p in lc["predicates"]]
    assert len(rej) == 2 and sum(rej) == lc["generated"] - lc["kept"]
    assert lc["predicates"][1]["tested"] == lc["generated"] - rej[0]
    assert lc["passes"] >= 2            # at most 7 % of 1024 rows are inside both ranges
    return tab


def scenario_guard_range(eng, device, n=200, **kw):
    """The privacy guard at the median unguarded DCR against small_table's real rows, combined with a driving range:
    every returned row is outside the radius and inside the range."""
    from fed_tgan_amd.eval.privacy import DevicePrivacy
    _, _, _, meta, vocabs, enc, _, _ = small_table()
    ev = DevicePrivacy(np.asarray(enc, dtype=np.float64), meta, vocabs, device, ops=eng.ops, max_rows=n, baseline=False)
    T = float(ev.score(eng.generate_decoded(n)).rows()[0].median())
    assert T > 0
    guard = ev.guard(T)
    req = request(SERROR, n, device)
    tab = eng.generate_decoded_guarded(n, guard, request=req, chunk=1024, **kw)
    lg, lc = eng.last_guard, eng.last_conditional
    assert tab.shape[0] == n and lg["kept"] == n and inside(tab, req)
    assert lc["predicates"][0]["tested"] == lg["generated"] == lc["generated"] and lc["filled"] == [n]
    assert lg["rejected"] > 0 and lc["predicates"][0]["rejected"] > 0
    ev.score(tab)
    assert bool((ev.d1[:n] > guard.t2).all())
    return tab


def reference_pass(out, preds):
    """numpy statement of pred_mark's rule on a decoded pass: the first failing predicate per row, -1 for none."""
    out = np.asarray(out)
    first = np.full(out.shape[0], -1)
    for r in range(out.shape[0]):
        for k, p in enumerate(preds):
            v = out[r, p[0]]
            if p[1] == RANGE:
                ok = v >= p[2] and v <= p[3]
            else:
                ok = v == np.trunc(v) and 0 <= v < len(p[2]) and p[2][int(v)] != 0
            if not ok:
                first[r] = k
                break
    return first
