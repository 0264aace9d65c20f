"""Shared cases of the fidelity-evaluator tests (test_fidelity.py on the CPU, test_hip_fidelity.py on the GPU): a
plain-numpy brute force of the whole contract (eval/fidelity.py) on top of privacy_cases.dist2, whose column-order
accumulation (a product, then a sum: no multiply-add) is the torch ops', and lattice tables on which every term and
every sum is exact in float64 with or without a fused multiply-add, so every implementation has to agree bit for bit,
ties, copies and boundary hits included.

Nothing here uses TorchOps: the brute force builds the full float64 d2 matrix and takes the k-th smallest per row with
np.partition, the counts with a comparison and a sum, the scores with one Python division of two integers each.
"""
from __future__ import annotations

import numpy as np
import torch

import privacy_cases as pc
from fed_tgan_amd.eval import DeviceFidelity

INF = float("inf")
KEYS = ("precision", "recall", "density", "coverage", "precision_rr", "recall_rr", "density_rr", "coverage_rr")
GUARD = -7.0


# ----------------------------------------------------------------------------- the brute force
def kth(d, k):
    """the k-th smallest entry of every row of a d2 matrix (excluded pairs at +inf), with multiplicity; +inf where a
    row has fewer than k candidates; a NaN is no candidate"""
    d = np.where(np.isnan(d), np.inf, d)
    padded = np.concatenate([d, np.full((d.shape[0], k), np.inf)], axis=1)
    return np.partition(padded, k - 1, axis=1)[:, k - 1]


def topk(q_cont, q_cat, r_cont, r_cat, k, exclude_self=False, d=None):
    d = pc.dist2(q_cont, q_cat, r_cont, r_cat) if d is None else d.copy()
    if exclude_self:
        np.fill_diagonal(d, np.inf)
    return kth(d, k)


def ball(d, rad):
    """(cnt int32, dmin) of a d2 matrix [nq, nr] against per-reference squared radii"""
    with np.errstate(invalid="ignore"):
        cnt = (d <= rad[None, :]).sum(axis=1).astype(np.int32)
    dmin = np.where(np.isnan(d), np.inf, d).min(axis=1) if d.shape[1] else np.full(d.shape[0], np.inf)
    return cnt, dmin


def four(cnt_a, cnt_b, dmin_b, rr, k):
    """the four scores: integer sums, one division each"""
    n, m = len(cnt_a), len(cnt_b)
    return [int((cnt_a > 0).sum()) / n, int((cnt_b > 0).sum()) / m, int(cnt_a.astype(np.int64).sum()) / (k * n),
            int((dmin_b <= rr).sum()) / m]


def prdc(r_cont, r_cat, q_cont, q_cat, k):
    """the contract in the packed space: {the four scores, rr, ff, cnt_a, cnt_b, dmin_b}"""
    rr = topk(r_cont, r_cat, r_cont, r_cat, k, True)
    ff = topk(q_cont, q_cat, q_cont, q_cat, k, True)
    d = pc.dist2(q_cont, q_cat, r_cont, r_cat)
    cnt_a, _ = ball(d, rr)
    cnt_b, dmin_b = ball(np.ascontiguousarray(d.T), ff)
    out = dict(zip(KEYS[:4], four(cnt_a, cnt_b, dmin_b, rr, k)))
    out.update(rr=rr, ff=ff, cnt_a=cnt_a, cnt_b=cnt_b, dmin_b=dmin_b)
    return out


def expected(real_coded, fake_coded, kinds, k, baseline=True):
    """the whole contract by brute force from coded tables: the eight scores and the per-row arrays"""
    kinds = np.asarray(kinds)
    rc = real_coded[:, kinds == pc.CONT]
    lo, hi = rc.min(axis=0), rc.max(axis=0)
    scale = np.where(hi > lo, 1.0 / np.where(hi > lo, hi - lo, 1.0), 1.0)
    r_cont, r_cat = pc.pack(real_coded, kinds, lo, scale)
    q_cont, q_cat = pc.pack(fake_coded, kinds, lo, scale)
    out = prdc(r_cont, r_cat, q_cont, q_cat, k)
    base = [float("nan")] * 4
    if baseline and (len(r_cont) + 1) // 2 >= k + 1:
        b = prdc(r_cont[0::2], r_cat[0::2], r_cont[1::2], r_cat[1::2], k)
        base = [b[key] for key in KEYS[:4]]
    out.update(zip(KEYS[4:], base))
    return out


# ----------------------------------------------------------------------------- tables
def lattice_packed(nq, nr, n_cont, n_cat, seed, same=False):
    """(q_cont, q_cat, r_cont, r_cat) in the packed space: continuous values on the lattice {0, 1/64, ..., 1}, codes
    in 0..3, a fifth of the queries copied from reference rows.  A difference is a multiple of 1/64 in [-1, 1], its
    square a multiple of 2^-12 <= 1, and a sum of a few hundred of them stays far below 2^53 ulps: every term and sum
    is exact however it is rounded, so distances tie exactly and copies sit exactly on the balls' boundaries."""
    g = np.random.default_rng(seed)
    r_cont = g.integers(0, 65, (nr, n_cont)) / 64.0
    r_cat = g.integers(0, 4, (nr, n_cat)).astype(np.int32)
    if same:
        return r_cont, r_cat, r_cont, r_cat
    q_cont = g.integers(0, 65, (nq, n_cont)) / 64.0
    q_cat = g.integers(0, 4, (nq, n_cat)).astype(np.int32)
    take = g.integers(0, nr, nq)
    copy = g.random(nq) < 0.2
    q_cont[copy], q_cat[copy] = r_cont[take[copy]], r_cat[take[copy]]
    return q_cont, q_cat, r_cont, r_cat


def lattice_dist2(q_cont, q_cat, r_cont, r_cat):
    """privacy_cases.dist2 of lattice tables by matrix products, for the shapes at which the column-by-column matrix
    takes many seconds.  Bit-equal to it: 64 times a lattice value is an integer <= 64, so |q|^2 + |r|^2 - 2 q.r is a
    sum of integers far below 2^53, exact in float64 in any order, and so are the division by 4096 and the one-hot
    products that count equal codes."""
    Q, R = q_cont * 64.0, r_cont * 64.0
    d = ((Q * Q).sum(axis=1)[:, None] + (R * R).sum(axis=1)[None, :] - 2.0 * (Q @ R.T)) / 4096.0
    equal = np.zeros(d.shape)
    for v in range(4):
        equal += (q_cat == v).astype(np.float64) @ (r_cat == v).astype(np.float64).T
    return d + (q_cat.shape[1] - equal)


def continuous_packed(nq, nr, n_cont, n_cat, seed):
    """random continuous reference rows and fresh random queries: no copies"""
    g = np.random.default_rng(seed)
    r_cont = g.random((nr, n_cont))
    r_cat = g.integers(0, 4, (nr, n_cat)).astype(np.int32)
    q_cont = g.random((nq, n_cont))
    q_cat = g.integers(0, 4, (nq, n_cat)).astype(np.int32)
    return q_cont, q_cat, r_cont, r_cat


def lattice_table(m, n, seed=0):
    """coded (real [m, 5], fake [n, 5], kinds) on the lattice; the real continuous columns span exactly [0, 1], so
    nn_pack leaves them as they are (lo 0, scale 1); a fifth of the fake rows are copies of real rows"""
    kinds = np.asarray(pc.EXACT_KINDS)
    n_cont, n_cat = int((kinds == pc.CONT).sum()), int((kinds == pc.CAT).sum())
    q_cont, q_cat, r_cont, r_cat = lattice_packed(n, m, n_cont, n_cat, seed)
    r_cont[0], r_cont[1] = 0.0, 1.0
    real, fake = np.zeros((m, len(kinds))), np.zeros((n, len(kinds)))
    real[:, kinds == pc.CONT], real[:, kinds == pc.CAT] = r_cont, r_cat
    fake[:, kinds == pc.CONT], fake[:, kinds == pc.CAT] = q_cont, q_cat
    return real, fake, kinds


# ----------------------------------------------------------------------------- shared checks (CPU ops / HIP ops)
def _dev(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)


def run_topk(ops, dev, q_cont, q_cat, r_cont, r_cat, k, exclude_self, guard=3):
    """nn_topk of ops on numpy inputs -> the radii as numpy; the output's tail and the scratch past the size
    nn_topk_scratch returns carry a guard value that has to survive"""
    nq, nr = q_cont.shape[0], r_cont.shape[0]
    out = torch.full((nq + guard,), GUARD, dtype=torch.float64, device=dev)
    used = ops.nn_topk_scratch(nq, nr, k)
    scratch = torch.full((used + guard,), GUARD, dtype=torch.float64, device=dev)
    ops.nn_topk(_dev(q_cont, torch.float64, dev), _dev(q_cat, torch.int32, dev), _dev(r_cont, torch.float64, dev),
                _dev(r_cat, torch.int32, dev), exclude_self, k, out, scratch)
    assert bool((out[nq:] == GUARD).all()) and bool((scratch[used:] == GUARD).all())
    return out[:nq].cpu().numpy()


def run_ball(ops, dev, q_cont, q_cat, r_cont, r_cat, rad, guard=3):
    """nn_ball of ops on numpy inputs -> (cnt int32, dmin) numpy, the guard tails checked as in run_topk"""
    nq, nr = q_cont.shape[0], r_cont.shape[0]
    cnt = torch.full((nq + guard,), int(GUARD), dtype=torch.int32, device=dev)
    dmin = torch.full((nq + guard,), GUARD, dtype=torch.float64, device=dev)
    used = ops.nn_ball_scratch(nq, nr)
    scratch = torch.full((used + guard,), GUARD, dtype=torch.float64, device=dev)
    ops.nn_ball(_dev(q_cont, torch.float64, dev), _dev(q_cat, torch.int32, dev), _dev(r_cont, torch.float64, dev),
                _dev(r_cat, torch.int32, dev), _dev(rad, torch.float64, dev), cnt, dmin, scratch)
    assert bool((cnt[nq:] == int(GUARD)).all()) and bool((dmin[nq:] == GUARD).all())
    assert bool((scratch[used:] == GUARD).all())
    return cnt[:nq].cpu().numpy(), dmin[:nq].cpu().numpy()


def run_reduce(ops, dev, cnt_a, cnt_b, dmin_b, rr, k, guard=3):
    """prdc_reduce of ops on numpy inputs with guarded tails -> the four scores as a list"""
    n, m = len(cnt_a), len(cnt_b)
    pad_i = np.full(guard, 5, dtype=np.int32)            # (would change every score if it were read)
    pad_f = np.full(guard, 0.0)
    scores = torch.full((4 + guard,), GUARD, dtype=torch.float64, device=dev)
    ops.prdc_reduce(_dev(np.concatenate([cnt_a, pad_i]), torch.int32, dev),
                    _dev(np.concatenate([cnt_b, pad_i]), torch.int32, dev),
                    _dev(np.concatenate([dmin_b, pad_f]), torch.float64, dev),
                    _dev(np.concatenate([rr, pad_f + 1.0]), torch.float64, dev), n, m, k, scores)
    assert bool((scores[4:] == GUARD).all())
    return scores[:4].cpu().tolist()


def column_radii(d, k):
    """per-reference radii for an op-level test, free of a second table: the k-th smallest distance of the queries
    to each reference row (+inf with fewer than k queries), so that query sits exactly on the boundary; every
    seventh radius is 0 (copies only) and every eleventh +inf"""
    rad = kth(np.ascontiguousarray(d.T), k)
    rad[3::7] = 0.0
    rad[5::11] = np.inf
    return rad


def check_exact(ops, dev, q_cont, q_cat, r_cont, r_cat, ks, same, what="", dist=pc.dist2):
    """nn_topk / nn_ball / prdc_reduce of ops against the brute force, bit for bit, for every k of ks on one d2
    matrix (dist: privacy_cases.dist2, or lattice_dist2 for a large lattice table)"""
    d = dist(q_cont, q_cat, r_cont, r_cat)
    for k in ks:
        want = topk(q_cont, q_cat, r_cont, r_cat, k, same, d=d)
        got = run_topk(ops, dev, q_cont, q_cat, r_cont, r_cat, k, same)
        assert np.array_equal(got, want), (what, k, "topk", np.nonzero(got != want)[0][:8])
        if r_cont.shape[0] - (1 if same else 0) < k:
            assert np.isinf(got).all(), (what, k)
        rad = want if same else column_radii(d, k)      # a table against itself: its own radii
        want_cnt, want_min = ball(d, rad)
        cnt, dmin = run_ball(ops, dev, q_cont, q_cat, r_cont, r_cat, rad)
        assert cnt.dtype == np.int32 and np.array_equal(cnt, want_cnt), (what, k, "cnt")
        assert np.array_equal(dmin, want_min), (what, k, "dmin")
        if same:        # every row is at 0 from itself and within the radius of its k nearest at least
            assert (dmin == 0.0).all() and (cnt >= 1).all()
        m = r_cont.shape[0]
        cnt_b, dmin_b = ball(np.ascontiguousarray(d.T), kth(d, k))
        rr = rad if same else kth(np.ascontiguousarray(d.T), k)
        scores = run_reduce(ops, dev, want_cnt, cnt_b, dmin_b, rr, k)
        assert scores == four(want_cnt, cnt_b, dmin_b, rr, k), (what, k, "scores", m)


def coded_evaluator(real, kinds, dev="cpu", ops=None, **kw):
    """DeviceFidelity on an already coded real table with the given column kinds"""
    meta = {"columns": [{"column_name": f"c{j}", "type": "categorical" if k == pc.CAT else "continuous"}
                        for j, k in enumerate(kinds)], "non_negative_cols": []}
    return DeviceFidelity(np.asarray(real, dtype=np.float64), meta, [], dev, ops=ops, **kw)


def assert_scores_equal(got: dict, want: dict, what=""):
    """the eight scores, exactly: each is one correctly rounded division of the same two integers"""
    assert tuple(got) == KEYS
    for key in KEYS:
        print(f"{what} {key}: got {got[key]!r} want {want[key]!r}")
        if np.isnan(want[key]):
            assert np.isnan(got[key]), (what, key, got[key])
        else:
            assert got[key] == want[key], (what, key, got[key], want[key])


def assert_rows_equal(scores, want, what=""):
    cnt_a, inside = (t.cpu().numpy() for t in scores.rows())
    covered, recalled = (t.cpu().numpy() for t in scores.real_rows())
    assert cnt_a.dtype == np.int32 and np.array_equal(cnt_a, want["cnt_a"]), what
    assert inside.dtype == np.bool_ and np.array_equal(inside, want["cnt_a"] > 0), what
    assert covered.dtype == np.bool_ and np.array_equal(covered, want["dmin_b"] <= want["rr"]), what
    assert recalled.dtype == np.bool_ and np.array_equal(recalled, want["cnt_b"] > 0), what
