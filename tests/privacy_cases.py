"""Shared cases of the privacy-evaluator tests (test_privacy.py on the CPU, test_hip_privacy.py on the GPU): a
plain-numpy brute force of the whole contract (eval/privacy.py), random mixed tables, and tables of small integers
on which every sum is exact, so every implementation has to agree bit for bit, ties included.

Nothing here uses TorchOps: the brute force builds the full float64 d2 matrix from direct differences, column by
column, and takes the two smallest per row with np.partition and the percentiles with np.percentile.
"""
from __future__ import annotations

import numpy as np
import torch

from fed_tgan_amd.data.demo import small_table   # noqa: F401  (the front-end tests' table)
from fed_tgan_amd.eval import DevicePrivacy

INF = float("inf")

CONT, CAT = 0, 1
# d1 / d2: relative error <= 1e-12 max(1, d2).  Derived, not measured: a sum of at most 514 non-negative float64
# terms, each carrying <= 3 roundings, has relative error <= 516 * 2^-53 ~ 6e-14 in any order, with or without
# multiply-add contraction; 1e-12 leaves a factor above 10.  The six scores: 1e-12 absolute.
TOL = 1e-12
KEYS = ("dcr_p5", "nndr_p5", "dcr_min", "copies", "dcr_rr_p5", "nndr_rr_p5")
LAYOUTS = {"cont": (1, 0), "cat": (0, 1), "small": (5, 4), "intrusion": (22, 20), "wide": (300, 212)}


def dist2(q_cont, q_cat, r_cont, r_cat):
    """full [nq, nr] float64 matrix: continuous terms in column order, then the mismatch count"""
    d = np.zeros((q_cont.shape[0], r_cont.shape[0]), dtype=np.float64)
    for c in range(q_cont.shape[1]):
        diff = q_cont[:, c, None] - r_cont[None, :, c]
        d += diff * diff
    miss = np.zeros(d.shape, dtype=np.int64)
    for c in range(q_cat.shape[1]):
        miss += q_cat[:, c, None] != r_cat[None, :, c]
    return d + miss.astype(np.float64)


def top2(q_cont, q_cat, r_cont, r_cat, exclude_self=False):
    """(d1, d2, i1, the d2 matrix with the excluded pairs at +inf)"""
    d = dist2(q_cont, q_cat, r_cont, r_cat)
    if exclude_self:
        np.fill_diagonal(d, np.inf)
    nq, nr = d.shape
    padded = np.concatenate([d, np.full((nq, 2), np.inf)], axis=1)      # fewer than two candidates: +inf
    two = np.partition(padded, 1, axis=1)[:, :2]
    d1, d2 = two[:, 0], two[:, 1]
    i1 = np.where(np.isinf(d1), -1, np.argmin(d, axis=1)).astype(np.int32)     # argmin: the first of equal values
    return d1, d2, i1, d


def table_scores(d1, d2):
    dcr = np.sqrt(d1)
    with np.errstate(divide="ignore", invalid="ignore"):
        nndr = np.sqrt(np.where(np.isinf(d2), 0.0, d1) / np.where((d2 == 0) | np.isinf(d2), 1.0, d2))
    nndr = np.where(d2 == 0, 1.0, nndr)
    with np.errstate(invalid="ignore"):       # (a column of +inf interpolates inf - inf)
        return dcr, nndr, [float(np.percentile(dcr, 5)), float(np.percentile(nndr, 5)), float(dcr.min()),
                           float((d1 == 0).mean())]


def pack(coded, kinds, lo, scale):
    kinds = np.asarray(kinds)
    cont = (coded[:, kinds == CONT] - lo) * scale
    cat = coded[:, kinds == CAT].astype(np.int64)
    return np.ascontiguousarray(cont), np.ascontiguousarray(cat)


def expected(real_coded, fake_coded, kinds):
    """the whole contract by brute force: {the six scores, d1, d2, i1, dcr, nndr} of fake against real"""
    kinds = np.asarray(kinds)
    rc = real_coded[:, kinds == CONT]
    lo, hi = rc.min(axis=0), rc.max(axis=0)
    scale = np.where(hi > lo, 1.0 / np.where(hi > lo, hi - lo, 1.0), 1.0)
    r_cont, r_cat = pack(real_coded, kinds, lo, scale)
    q_cont, q_cat = pack(fake_coded, kinds, lo, scale)
    d1, d2, i1, _ = top2(q_cont, q_cat, r_cont, r_cat)
    dcr, nndr, four = table_scores(d1, d2)
    b1, b2, _, _ = top2(r_cont, r_cat, r_cont, r_cat, exclude_self=True)
    base = table_scores(b1, b2)[2]
    out = dict(zip(KEYS, four + base[:2]))
    out.update(d1=d1, d2=d2, i1=i1, dcr=dcr, nndr=nndr, lo=lo, scale=scale)
    return out


def random_packed(nq, nr, n_cont, n_cat, seed, same=False):
    """(q_cont, q_cat, r_cont, r_cat) in the packed space: continuous values around [0, 1], a few of the queries
    copied from reference rows, codes from a small alphabet (so categorical-only tables tie all the time)"""
    g = np.random.default_rng(seed)
    r_cont = g.random((nr, n_cont))
    r_cat = g.integers(0, 4, (nr, n_cat)).astype(np.int32)
    if same:
        return r_cont, r_cat, r_cont, r_cat
    q_cont = g.random((nq, n_cont)) * 1.5 - 0.25
    q_cat = g.integers(0, 5, (nq, n_cat)).astype(np.int32)
    take = g.integers(0, nr, nq)
    copy = g.random(nq) < 0.2
    q_cont[copy], q_cat[copy] = r_cont[take[copy]], r_cat[take[copy]]
    return q_cont, q_cat, r_cont, r_cat


def assert_top2(got_d1, got_d2, got_i1, want_d1, want_d2, q_cont, q_cat, r_cont, r_cat, exclude_self, what=""):
    """d1 / d2 within TOL of the reference; the reference's own d2 at the returned i1 equals the reference d1 within
    the same bound (near-ties may resolve to another row; an exact tie-break is checked on the integer cases)"""
    for got, want, name in ((got_d1, want_d1, "d1"), (got_d2, want_d2, "d2")):
        inf = np.isinf(want)
        assert np.array_equal(np.isinf(got), inf), (what, name)
        err = np.abs(got[~inf] - want[~inf]) / np.maximum(1.0, want[~inf])
        print(f"{what} {name} max rel err {err.max() if err.size else 0.0:.3e}")
        assert (err <= TOL).all(), (what, name, float(err.max()))
    none = np.isinf(want_d1)
    assert (got_i1[none] == -1).all(), what
    idx = got_i1[~none].astype(np.int64)
    rows = np.nonzero(~none)[0]
    assert ((idx >= 0) & (idx < r_cont.shape[0])).all(), what
    if exclude_self:
        assert (idx != rows).all(), what
    diff = q_cont[rows] - r_cont[idx]
    at = (diff * diff).sum(axis=1) if q_cont.shape[1] else np.zeros(len(rows))
    at = at + (q_cat[rows] != r_cat[idx]).sum(axis=1)
    err = np.abs(at - want_d1[~none]) / np.maximum(1.0, want_d1[~none])
    assert (err <= TOL).all(), (what, "i1", float(err.max()) if err.size else 0.0)


# ----------------------------------------------------------------------------- exact integer cases
EXACT_KINDS = (CONT, CAT, CONT, CONT, CAT)


def exact_case(nr, twins, nq=24, seed=0):
    """Real rows of small integers whose continuous columns span exactly [0, 1] (scale 1, lo 0): every d2 is an
    exact small integer and ties are everywhere.  twins: (a, b) index pairs, a < b: real row b is a copy of real row
    a, and no other real row equals them (a code of their own in the first categorical column).  The first len(twins)
    fake rows are copies of the twins, the next ones differ from a twin in one categorical column, the rest are
    random with continuous values in 0..3.  Returns (real_coded, fake_coded, kinds)."""
    g = np.random.default_rng(seed)
    kinds = np.asarray(EXACT_KINDS)
    real = np.zeros((nr, len(kinds)))
    real[:, kinds == CONT] = g.integers(0, 2, (nr, int((kinds == CONT).sum())))
    real[:, kinds == CAT] = g.integers(0, 3, (nr, int((kinds == CAT).sum())))
    if nr >= 2:
        real[0, kinds == CONT], real[1, kinds == CONT] = 0.0, 1.0
    for t, (a, b) in enumerate(twins):
        real[a, 1] = 10 + t
        real[b] = real[a]
    fake = np.zeros((nq, len(kinds)))
    fake[:, kinds == CONT] = g.integers(0, 4, (nq, int((kinds == CONT).sum())))
    fake[:, kinds == CAT] = g.integers(0, 3, (nq, int((kinds == CAT).sum())))
    for t, (a, b) in enumerate(twins):
        fake[t] = real[a]
        fake[len(twins) + t] = real[a]
        fake[len(twins) + t, 4] = 99
    return real, fake, kinds


# ----------------------------------------------------------------------------- shared checks (CPU ops / HIP ops)
def run_top2(ops, dev, q_cont, q_cat, r_cont, r_cat, exclude_self, guard=3):
    """nn_top2 of ops on numpy inputs -> (d1, d2, i1) numpy; the output tails and the scratch past its used part
    carry a guard value that has to survive"""
    nq, nr = q_cont.shape[0], r_cont.shape[0]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)      # noqa: E731
    d1 = torch.full((nq + guard,), -7.0, dtype=torch.float64, device=dev)
    d2 = torch.full((nq + guard,), -7.0, dtype=torch.float64, device=dev)
    i1 = torch.full((nq + guard,), -7, dtype=torch.int32, device=dev)
    used = ops.nn_scratch(nq, nr)
    scratch = torch.full((used + guard,), -7.0, dtype=torch.float64, device=dev)
    ops.nn_top2(t(q_cont, torch.float64), t(q_cat, torch.int32), t(r_cont, torch.float64), t(r_cat, torch.int32),
                exclude_self, d1, d2, i1, scratch)
    assert bool((d1[nq:] == -7.0).all()) and bool((d2[nq:] == -7.0).all()) and bool((i1[nq:] == -7).all())
    assert bool((scratch[used:] == -7.0).all())
    return d1[:nq].cpu().numpy(), d2[:nq].cpu().numpy(), i1[:nq].cpu().numpy()


def coded_evaluator(real, kinds, dev="cpu", ops=None, **kw):
    """DevicePrivacy on an already coded real table with the given column kinds"""
    meta = {"columns": [{"column_name": f"c{j}", "type": "categorical" if k == CAT else "continuous"}
                        for j, k in enumerate(kinds)], "non_negative_cols": []}
    return DevicePrivacy(np.asarray(real, dtype=np.float64), meta, [], dev, ops=ops, **kw)


def assert_scores(got: dict, want: dict, what=""):
    assert tuple(got) == KEYS
    for k in KEYS:
        print(f"{what} {k}: got {got[k]!r} want {want[k]!r}")
        if np.isfinite(want[k]):
            assert abs(got[k] - want[k]) <= TOL, (what, k, got[k], want[k])
        else:       # no candidate at all (a one-row real table against itself): numpy interpolates inf - inf = nan
            assert not np.isfinite(got[k]), (what, k, got[k], want[k])


def exact_top2(ops, dev, real, fake, kinds, exclude_self=False):
    """(got, want) of an integer table through nn_pack (lo 0, scale 1) and nn_top2"""
    want = expected(real, fake, kinds)
    assert (want["lo"] == 0.0).all() and (want["scale"] == 1.0).all()
    r_cont, r_cat = pack(real, kinds, want["lo"], want["scale"])
    q_cont, q_cat = (r_cont, r_cat) if exclude_self else pack(fake, kinds, want["lo"], want["scale"])
    w = top2(q_cont, q_cat, r_cont, r_cat, exclude_self)
    return run_top2(ops, dev, q_cont, q_cat, r_cont, r_cat, exclude_self), w[:3]


def assert_exact(got, want, what=""):
    for g, w, name in zip(got, want, ("d1", "d2", "i1")):
        assert np.array_equal(g, w), (what, name, np.nonzero(g != w)[0][:8])


def check_exact_cases(ops, dev, nr, twins):
    """the integer cases of both test files: copies, duplicated nearest rows, the lowest index, self exclusion"""
    real, fake, kinds = exact_case(nr, twins)
    got, want = exact_top2(ops, dev, real, fake, kinds)
    assert_exact(got, want, "fake vs real")
    d1, d2, i1 = got
    for t, (a, b) in enumerate(twins):
        assert d1[t] == 0.0 and d2[t] == 0.0 and i1[t] == a              # a copy of a duplicated record: the lower index
        k = len(twins) + t
        assert d1[k] == 1.0 and d2[k] == d1[k] and i1[k] == a            # a duplicated nearest row
    ev = coded_evaluator(real, kinds, dev, ops, max_rows=len(fake))
    s = ev.score(torch.from_numpy(fake).to(dev))
    exp = expected(real, fake, kinds)
    f = s.floats()
    assert f["copies"] == float((exp["d1"] == 0).mean()) and f["copies"] >= len(twins) / len(fake)
    assert f["dcr_min"] == 0.0
    assert_scores(f, exp, "exact")
    # the real table against itself: twins are at 0 from each other, nobody is their own neighbour
    got, want = exact_top2(ops, dev, real, fake, kinds, exclude_self=True)
    assert_exact(got, want, "real vs real")
    d1, d2, i1 = got
    assert (i1 != np.arange(nr)).all()
    for a, b in twins:
        assert d1[a] == 0.0 and d1[b] == 0.0 and i1[a] == b and i1[b] == a


def check_single_reference_row(ops, dev):
    q_cont = np.array([[0.0], [2.0]])
    q_cat = np.array([[1], [1]], dtype=np.int32)
    d1, d2, i1 = run_top2(ops, dev, q_cont, q_cat, q_cont[:1], np.array([[2]], dtype=np.int32), False)
    assert d1.tolist() == [1.0, 5.0] and d2.tolist() == [INF, INF] and i1.tolist() == [0, 0]
    d1, d2, i1 = run_top2(ops, dev, q_cont[:1], q_cat[:1], q_cont[:1], q_cat[:1], True)
    assert d1.tolist() == [INF] and d2.tolist() == [INF] and i1.tolist() == [-1]
    ev = coded_evaluator(np.array([[0.0, 2.0]]), [CONT, CAT], dev, ops, max_rows=2)
    f = ev.score(torch.tensor([[0.0, 1.0], [2.0, 1.0]], dtype=torch.float64, device=dev))
    assert f.floats()["nndr_p5"] == 0.0 and f.rows()[1].tolist() == [0.0, 0.0]      # no second candidate: NNDR 0
    assert f.rows()[0].tolist() == [1.0, 5.0 ** 0.5]                                  # (constant column: scale 1)
