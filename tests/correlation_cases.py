"""Shared cases of the correlation-evaluator tests (test_correlation.py on the CPU, test_hip_correlation.py on the
GPU): a plain-numpy brute force of the whole contract (eval/correlation.py), random mixed tables with planted
dependence, and the checks both backends go through.

Nothing here uses TorchOps: the brute force builds every contingency table with np.add.at and every moment from
direct centred sums, one column pair at a time.

Bounds (derived, not measured).  Counts are exact integers.  Pearson and the correlation ratio carry at most
n 2^-53 relative error in their sums, about 4e-12 at n = 40,000.  An entropy sum over probabilities that add to 1 is
bounded by ln(bins), at most about 11, times the same factor, and the division by H(i) amplifies it by 1 / H(i): the
tables here keep every non-constant categorical column's entropy at 0.1 nat or more (asserted in
:func:`association`), which gives about 5e-10 in the worst case.  So every entry of A: TOL = 1e-9 absolute;
corr_diff, a norm over C^2 entries each within TOL of its true value twice over: 2 C TOL; the other three scores,
corr_diff_rr among them: 2 TOL.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from fed_tgan_amd.data.demo import small_table   # noqa: F401  (the front-end tests' table)
from fed_tgan_amd.eval import DeviceCorrelation

CONT, CAT = 0, 1
TOL = 1e-9
MIN_ENTROPY = 0.1
KEYS = ("corr_diff", "corr_mean_abs", "corr_max_abs", "corr_diff_rr")
LAYOUTS = {"cont": (3, 0), "cat": (0, 3), "pair": (1, 1), "small": (5, 4), "intrusion": (22, 20), "wide": (40, 36)}


# ----------------------------------------------------------------------------- the brute force
def cards_of(real, kinds, cardinalities=None):
    """K_c of every categorical column of a coded real table: 1 + the largest real code, or what is given"""
    cat = [j for j, k in enumerate(kinds) if k == CAT]
    cards = [1 + int(real[:, j].max()) for j in cat]
    if cardinalities is not None:
        cards = [max(a, int(b)) for a, b in zip(cards, cardinalities)]
    return cards


def codes_of(col, K):
    """the overflow rule: a value that is NaN or no code of [0, K) is the extra category K"""
    with np.errstate(invalid="ignore"):
        ok = (col >= 0) & (col < K)
    return np.where(ok, np.where(ok, col, 0.0), float(K)).astype(np.int64)


def entropy(counts, n):
    p = counts[counts > 0] / float(n)
    return float(-(p * np.log(p)).sum())


def association(table, kinds, cards, check_entropy=True):
    """A [C, C] of the contract, one pair at a time"""
    table = np.asarray(table, dtype=np.float64)
    n, C = table.shape
    it = iter(cards)
    K = [next(it) if k == CAT else 0 for k in kinds]
    code = {j: codes_of(table[:, j], K[j]) for j in range(C) if kinds[j] == CAT}
    cen = {}
    for j in range(C):
        if kinds[j] == CONT:
            x = table[:, j]
            cen[j] = x - x.sum() / n
    marg = {j: np.bincount(code[j], minlength=K[j] + 1) for j in code}
    H = {j: entropy(marg[j], n) for j in code}
    if check_entropy:
        for j in code:
            assert H[j] == 0.0 or H[j] >= MIN_ENTROPY, f"column {j}: entropy {H[j]} is below the bound's assumption"
    A = np.eye(C)
    for i in range(C):
        for j in range(C):
            if i == j:
                continue
            if kinds[i] == CONT and kinds[j] == CONT:
                sxx, syy = (cen[i] * cen[i]).sum(), (cen[j] * cen[j]).sum()
                if sxx > 0 and syy > 0:
                    A[i, j] = min(1.0, max(-1.0, (cen[i] * cen[j]).sum() / math.sqrt(sxx * syy)))
                else:
                    A[i, j] = 0.0
            elif kinds[i] == CAT and kinds[j] == CAT:
                T = np.zeros((K[i] + 1, K[j] + 1), dtype=np.int64)
                np.add.at(T, (code[i], code[j]), 1)
                if H[i] == 0.0:
                    A[i, j] = 1.0
                    continue
                kk, ll = np.nonzero(T)
                t = T[kk, ll].astype(np.float64)
                h_cond = float(((t / n) * np.log(marg[j][ll] / t)).sum())
                A[i, j] = min(1.0, max(0.0, (H[i] - h_cond) / H[i]))
            else:
                a, x = (i, j) if kinds[i] == CAT else (j, i)
                sxx = (cen[x] * cen[x]).sum()
                if sxx > 0:
                    S = np.zeros(K[a] + 1)
                    np.add.at(S, code[a], cen[x])
                    live = marg[a] > 0
                    A[i, j] = min(1.0, max(0.0, math.sqrt((S[live] ** 2 / marg[a][live]).sum() / sxx)))
                else:
                    A[i, j] = 0.0
    return A


def diff_scores(A, B):
    C = A.shape[0]
    d = np.abs(A - B)
    off = d[~np.eye(C, dtype=bool)]
    return [float(np.sqrt((d * d).sum())), float(off.mean()) if C > 1 else 0.0, float(off.max()) if C > 1 else 0.0]


def expected(real, fake, kinds, cardinalities=None, baseline=True, check_entropy=True):
    """the whole contract by brute force: {the four scores, A_real, A_fake}"""
    cards = cards_of(real, kinds, cardinalities)
    a_real = association(real, kinds, cards, check_entropy)
    a_fake = association(fake, kinds, cards, check_entropy)
    rr = float("nan")
    if baseline and real.shape[0] >= 2:
        rr = diff_scores(association(real[0::2], kinds, cards, check_entropy),
                         association(real[1::2], kinds, cards, check_entropy))[0]
    out = dict(zip(KEYS, diff_scores(a_real, a_fake) + [rr]))
    out.update(A_real=a_real, A_fake=a_fake, cards=cards)
    return out


# ----------------------------------------------------------------------------- tables
def layout_kinds(n_cont, n_cat, seed=0):
    kinds = np.array([CONT] * n_cont + [CAT] * n_cat)
    np.random.default_rng(seed).shuffle(kinds)
    return kinds.tolist()


def random_table(n, kinds, seed, cards=None):
    """a coded table whose columns all lean on one hidden uniform: continuous = weight * hidden + noise, categorical
    = a noisy quantile bin of it.  cards: categories per categorical column (default 2..6, cycling)."""
    g = np.random.default_rng(seed)
    hidden = g.random(n)
    t = np.zeros((n, len(kinds)))
    s = 0
    for j, k in enumerate(kinds):
        if k == CAT:
            K = cards[s] if cards is not None else 2 + s % 5
            s += 1
            t[:, j] = np.minimum(np.floor((0.6 * hidden + 0.4 * g.random(n)) * K), K - 1)
        else:
            t[:, j] = g.normal() * 2.0 * hidden + g.normal(size=n) * 0.7 + 10.0 * g.normal()
    return t


def wide_cards(n_cat):
    return [2 + (7 * s) % 30 for s in range(n_cat)]       # 2..31


def planted(n, seed):
    """a uniform over 4 values; b = a with probability 0.9, else uniform; x = a + N(0, 0.3)"""
    g = np.random.default_rng(seed)
    a = g.integers(0, 4, n)
    b = np.where(g.random(n) < 0.9, a, g.integers(0, 4, n))
    x = a + g.normal(size=n) * 0.3
    return np.stack([a.astype(np.float64), b.astype(np.float64), x], axis=1), [CAT, CAT, CONT]


# ----------------------------------------------------------------------------- shared checks (CPU ops / HIP ops)
def coded_evaluator(real, kinds, dev="cpu", ops=None, **kw):
    """DeviceCorrelation on an already coded real table with the given column kinds"""
    meta = {"columns": [{"column_name": f"c{j}", "type": "categorical" if k == CAT else "continuous"}
                        for j, k in enumerate(kinds)], "non_negative_cols": []}
    return DeviceCorrelation(np.asarray(real, dtype=np.float64), meta, [], dev, ops=ops, **kw)


def run_matrix(ops, ev, table, guard=3):
    """A of a coded table through the four ops of ``ops`` on the column tables of evaluator ``ev``, over fresh
    buffers whose tails past the used part carry a guard value that has to survive; returns (A, G, counts) numpy"""
    dev = ev.device
    n = table.shape[0]
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    values = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float64)).to(dev)
    cont = torch.full((n + guard, ev.n_cont), -7.0, **f64)
    cat_t = torch.full((ev.n_cat, n + guard), -7, **i32)
    mean_all = torch.full((ev.n_cont + guard,), -7.0, **f64)
    mean = mean_all[:ev.n_cont]
    used = ops.corr_part(n, ev.W, ev.n_cont)
    part = torch.full((used + guard,), -7.0, **f64)
    total = int(ev.poff[-1])
    counts_all = torch.full((max(total, 1) + guard,), -7, **i32)
    counts = counts_all[:max(total, 1)]
    g_all = torch.full((ev.W * ev.n_cont + guard,), -7.0, **f64)
    G = g_all[:ev.W * ev.n_cont].view(ev.W, ev.n_cont)
    a_all = torch.full((ev.n_cols * ev.n_cols + guard,), -7.0, **f64)
    A = a_all[:ev.n_cols * ev.n_cols].view(ev.n_cols, ev.n_cols)
    ops.corr_pack(values, ev.kind, ev.slot, ev.card, cont, cat_t, mean, part)
    ops.corr_moments(cont, cat_t, n, mean, ev.card, ev.offs, G, part)
    ops.corr_counts(cat_t, n, ev.pairs_t, ev.poff, counts, ev.lds_bins)
    ops.corr_matrix(G, counts, ev.poff, ev.kind, ev.slot, ev.card, ev.offs, n, A)
    out_all = torch.full((3 + guard,), -7.0, **f64)
    ops.corr_diff(ev.A_real, A, out_all[:3])
    assert bool((out_all[3:] == -7.0).all()) and bool((out_all[:3] >= 0.0).all()), "corr_diff guard"
    assert bool((mean_all[ev.n_cont:] == -7.0).all()), "mean guard"
    assert bool((cont[n:] == -7.0).all()) and bool((cat_t[:, n:] == -7).all()), "pack wrote past its rows"
    assert bool((part[used:] == -7.0).all()), "part guard"
    assert bool((counts_all[max(total, 1):] == -7).all()), "counts guard"
    assert bool((g_all[ev.W * ev.n_cont:] == -7.0).all()) and bool((a_all[ev.n_cols ** 2:] == -7.0).all()), "G / A guard"
    if total:
        assert int(counts[:total].min()) >= 0
    return A.cpu().numpy().copy(), G.cpu().numpy().copy(), counts[:total].cpu().numpy().copy()


def assert_matrix(got, want, what=""):
    err = float(np.abs(got - want).max())
    print(f"{what} worst |A - A_ref| = {err:.3e}")
    assert np.isfinite(got).all(), what
    assert err <= TOL, (what, err, np.unravel_index(np.abs(got - want).argmax(), got.shape))


def assert_scores(got: dict, want: dict, C: int, what=""):
    assert tuple(got) == KEYS
    for k in KEYS:
        print(f"{what} {k}: got {got[k]!r} want {want[k]!r}")
        if np.isnan(want[k]):
            assert np.isnan(got[k]), (what, k, got[k])
        else:
            bound = 2 * C * TOL if k == "corr_diff" else 2 * TOL
            assert abs(got[k] - want[k]) <= bound, (what, k, got[k], want[k])


def check_layout(ops, dev, layout, n, seed=0):
    """a random real / generated table pair of a layout: the ops' matrix and the evaluator's scores against the brute
    force; returns the evaluator and the generated table"""
    n_cont, n_cat = LAYOUTS[layout]
    kinds = layout_kinds(n_cont, n_cat, seed)
    cards = wide_cards(n_cat) if layout == "wide" else None
    real = random_table(max(n, 2) + 40, kinds, 100 + seed, cards)
    fake = random_table(n, kinds, 200 + seed, cards)
    want = expected(real, fake, kinds, cardinalities=cards)
    ev = coded_evaluator(real, kinds, dev, ops, max_rows=n, cardinalities=cards)
    assert ev.card_list == want["cards"]
    A, _, _ = run_matrix(ops, ev, fake)
    assert_matrix(A, want["A_fake"], f"{layout} n={n} ops")
    s = ev.score(torch.from_numpy(fake).to(dev))
    assert_matrix(s.matrix().cpu().numpy(), want["A_fake"], f"{layout} n={n} score")
    assert_matrix(ev.A_real.cpu().numpy(), want["A_real"], f"{layout} n={n} real")
    assert_scores(s.floats(), want, len(kinds), f"{layout} n={n}")
    return ev, fake
