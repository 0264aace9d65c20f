"""The tree-utility evaluator's contract (fed_tgan_amd/eval/forest_device.py) restated by brute force in plain numpy
and Python loops, the tables of both test files, and the checks they share.

The brute force uses nothing of TorchOps: binning, Philox4x32-10 in Python integers, recursive growth with loops over
features, bins and classes in the stated float order (Python floats are fp64 and nothing is contracted), prediction
and scores.  Everything the evaluator computes is integers, or fp64 in a fixed order, so the comparisons are equalities:
tree arrays, multiplicities and confusion matrices match exactly, the scores within 8 K eps (the brute force adds the K
terms of the F1 in the same order; the bound covers a library that would not), and HIP ops and TorchOps bit for bit.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from fed_tgan_amd.data.demo import small_table   # noqa: F401  (the front-end tests' table)
from fed_tgan_amd.eval import DeviceForest
from fed_tgan_amd.eval.forest_device import KEYS, TreeModel, TreeTable
from utility_cases import CAT, CONT, TARGET, make_kinds, random_table

EPS = 2.0 ** -52
M32 = 0xFFFFFFFF
STREAM_DRAW, STREAM_FEAT = 0x74726231, 0x74726632
MAX_BINS = 256


# ----------------------------------------------------------------------------- Philox4x32-10, restated
def philox_word(seed, stream, w, hi, lo):
    """first output word for the counter (lo, hi, stream, w) under the key seed"""
    c = [lo & M32, hi & M32, stream & M32, w & M32]
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c[0]


def multiplicities(n, t, seed, bootstrap):
    m = np.zeros(n, dtype=np.int64)
    if not bootstrap:
        m[:] = 1
        return m
    for j in range(n):
        m[(philox_word(seed, STREAM_DRAW, 0, t, j) * n) >> 32] += 1
    return m


# ----------------------------------------------------------------------------- binning
def edges_of(col):
    u = sorted(set(float(v) for v in col))
    if len(u) <= MAX_BINS:
        e = [(a + b) / 2.0 for a, b in zip(u[:-1], u[1:])]
    else:
        s = np.sort(np.asarray(col, dtype=np.float64))
        e = []
        for k in range(1, MAX_BINS):           # the k / 256 quantile, midpoint interpolation
            pos = (len(s) - 1) * (k / float(MAX_BINS))
            lo, hi = int(math.floor(pos)), int(math.ceil(pos))
            e.append((s[lo] + s[hi]) / 2.0)
    return sorted(set(e))


def setup(train, test, kinds, cardinalities=None):
    """(cards per feature (0 for a continuous one), edges per feature, bins per feature, K)"""
    pooled = np.concatenate([train, test], axis=0)
    cards, edges, nbins, K, s = [], [], [], None, 0
    for j, k in enumerate(kinds):
        if k == CONT:
            cards.append(0)
            edges.append(edges_of(pooled[:, j]))
            nbins.append(len(edges[-1]) + 1)
            continue
        Kc = 1 + int(pooled[:, j].max())
        if cardinalities is not None:
            Kc = max(Kc, int(cardinalities[s]))
        s += 1
        if k == TARGET:
            K = Kc
        else:
            cards.append(Kc)
            edges.append([])
            nbins.append(Kc + 1)
    return cards, edges, nbins, K


def code_of(v, K):
    return int(v) if (v >= 0 and v < K) else K          # (a NaN fails both comparisons)


def binned(table, kinds, cards, edges, K):
    """(bins [F, n], y [n])"""
    n = table.shape[0]
    F = len(cards)
    bins, y = np.zeros((F, n), dtype=np.int64), np.zeros(n, dtype=np.int64)
    f = 0
    for j, k in enumerate(kinds):
        for r in range(n):
            v = table[r, j]
            if k == TARGET:
                y[r] = code_of(v, K)
            elif k == CAT:
                bins[f, r] = code_of(v, cards[f])
            else:
                bins[f, r] = sum(1 for e in edges[f] if v > e)
        f += k != TARGET
    return bins, y


def class_weights(y, K):
    counts = [int((y == c).sum()) for c in range(K)]
    nv, present = sum(counts), sum(c > 0 for c in counts)
    return counts, [float(nv) / (float(present) * float(c)) if c > 0 else 0.0 for c in counts]


# ----------------------------------------------------------------------------- growth
def side_term(n, w):
    T = Q = 0.0
    for c in range(len(w)):
        m = float(n[c]) * w[c]
        T = T + m
        Q = Q + m * m
    return Q / T


def node_split(rows, bins, y, mult, w, nbins, K, min_leaf, m_feat, seed, t, g):
    """(feature, bin, left counts) of the best split of a node, or None"""
    F = bins.shape[0]
    tot = [0] * K
    for r in rows:
        tot[y[r]] += int(mult[r])
    cand = {}
    for f in range(F):
        hist = [[0] * K for _ in range(nbins[f])]
        for r in rows:
            hist[min(bins[f, r], nbins[f] - 1)][y[r]] += int(mult[r])
        left, best = [0] * K, None
        for b in range(nbins[f] - 1):
            left = [a + h for a, h in zip(left, hist[b])]
            right = [a - b_ for a, b_ in zip(tot, left)]
            if sum(left) < min_leaf or sum(right) < min_leaf:
                continue
            s = side_term(left, w) + side_term(right, w)
            if best is None or s > best[0]:
                best = (s, b, list(left))
        if best is not None:
            cand[f] = best
    feats = sorted(cand)
    if m_feat < F:
        feats = sorted(sorted(feats, key=lambda f: (philox_word(seed, STREAM_FEAT, g, t, f), f))[:m_feat])
    pick = None
    for f in feats:
        if pick is None or cand[f][0] > cand[pick][0]:
            pick = f
    return None if pick is None else (pick, cand[pick][1], cand[pick][2])


def grow(bins, y, mult, w, nbins, K, max_depth, min_leaf, m_feat, seed, t):
    """the five arrays of one tree, in level order"""
    nodes = {}

    def rec(g, rows, depth):
        counts = [0] * K
        for r in rows:
            counts[y[r]] += int(mult[r])
        node = dict(counts=counts, feature=-1, bin=0)
        nodes[g] = node
        if depth >= max_depth or sum(c > 0 for c in counts) <= 1:
            return
        sp = node_split(rows, bins, y, mult, w, nbins, K, min_leaf, m_feat, seed, t, g)
        if sp is None:
            return
        node["feature"], node["bin"] = sp[0], sp[1]
        rec(2 * g, [r for r in rows if bins[sp[0], r] <= sp[1]], depth + 1)
        rec(2 * g + 1, [r for r in rows if bins[sp[0], r] > sp[1]], depth + 1)

    rec(1, [r for r in range(len(y)) if mult[r] > 0 and y[r] < K], 0)
    order = sorted(nodes)                 # heap indices grow with the level: this is level order
    index = {g: i for i, g in enumerate(order)}
    return dict(feature=np.array([nodes[g]["feature"] for g in order]), bin=np.array([nodes[g]["bin"] for g in order]),
                left=np.array([index[2 * g] if nodes[g]["feature"] >= 0 else 0 for g in order]),
                heap=np.array(order), counts=np.array([nodes[g]["counts"] for g in order]).reshape(len(order), K))


def leaf_of(tree, bins, r):
    i = 0
    while tree["feature"][i] >= 0:
        i = tree["left"][i] + (1 if bins[tree["feature"][i], r] > tree["bin"][i] else 0)
    return i


def predict(trees, bins, w, K, soft):
    n = bins.shape[1]
    pred = np.zeros(n, dtype=np.int64)
    for r in range(n):
        p = [0.0] * K
        for tree in trees:
            cnt = tree["counts"][leaf_of(tree, bins, r)]
            m = [float(cnt[c]) * w[c] for c in range(K)]
            if not soft:
                p = m
                break
            T = 0.0
            for c in range(K):
                T = T + m[c]
            if T > 0.0:
                p = [p[c] + m[c] / T for c in range(K)]
        best = 0
        for c in range(1, K):
            if p[c] > p[best]:
                best = c
        pred[r] = best
    return pred


def confusion(y, pred, K):
    conf = np.zeros((K, K), dtype=np.int64)
    for a, b in zip(y, pred):
        if a < K:
            conf[a, b] += 1
    return conf


def conf_scores(conf):
    total = int(conf.sum())
    if total == 0:
        return 0.0, 0.0
    f1 = 0.0
    for c in range(conf.shape[0]):
        tp, rs, cs = int(conf[c, c]), int(conf[c].sum()), int(conf[:, c].sum())
        if rs + cs > 0:
            f1 = f1 + float(rs) * ((2.0 * tp) / float(rs + cs))
    return f1 / total, float(int(np.trace(conf))) / total


def fit_models(table, kinds, cards, edges, nbins, K, p, bt, yt):
    """both models on one table: bins, weights, multiplicities, trees, predictions on the held-out bins"""
    bins, y = binned(table, kinds, cards, edges, K)
    counts, w = class_weights(y, K)
    n, F = len(y), len(cards)
    out = dict(bins=bins, y=y, counts=counts, w=w)
    for model, T, boot, m_feat in (("dt", 1, False, F), ("rf", p["trees"], True, max(1, math.isqrt(F)))):
        mult = [multiplicities(n, t, p["seed"], boot) for t in range(T)]
        trees = [grow(bins, y, mult[t], w, nbins, K, p["max_depth"], p["min_leaf"], m_feat, p["seed"], t)
                 for t in range(T)]
        conf = confusion(yt, predict(trees, bt, w, K, boot), K)
        out[model] = dict(mult=np.array(mult), trees=trees, conf=conf, scores=conf_scores(conf))
    return out


def expected(train, test, fake, kinds, p, cardinalities=None):
    """the whole contract by brute force"""
    cards, edges, nbins, K = setup(train, test, kinds, cardinalities)
    bt, yt = binned(test, kinds, cards, edges, K)
    out = dict(cards=cards, edges=edges, nbins=nbins, K=K, bt=bt, yt=yt)
    for side, table in (("real", train), ("fake", fake)):
        out[side] = fit_models(table, kinds, cards, edges, nbins, K, p, bt, yt)
    sc = {}
    for m in ("dt", "rf"):
        (f1, acc), (rf1, racc) = out["fake"][m]["scores"], out["real"][m]["scores"]
        sc.update(zip([f"{m}_{k}" for k in ("f1_fake", "acc_fake", "f1_real", "acc_real", "f1_gap", "acc_gap")],
                      [f1, acc, rf1, racc, rf1 - f1, racc - acc]))
    out["scores"] = sc
    return out


# ----------------------------------------------------------------------------- tables
P0 = dict(trees=3, max_depth=4, min_leaf=1, seed=5)


def _cardinalities(kinds, cards, K):
    it = iter(cards)
    return [K if k == TARGET else next(it) for k in kinds if k != CONT]


def _random_case(n, n_cont, cards, K, present=None, n_real=120, n_test=60, **p):
    kinds = make_kinds(n_cont, len(cards), seed=n_cont + len(cards))
    return dict(train=random_table(n_real, kinds, 1, cards, K), test=random_table(n_test, kinds, 2, cards, K),
                fake=random_table(n, kinds, 3, cards, K, present=present), kinds=kinds,
                cardinalities=_cardinalities(kinds, cards, K), p=dict(P0, **p))


def _coded(cols, y):
    return np.column_stack([np.asarray(c, dtype=np.float64) for c in cols] + [np.asarray(y, dtype=np.float64)])


def chain_table(n):
    """one continuous feature, sorted distinct values, alternating classes"""
    return _coded([np.arange(n) * 1.5], np.arange(n) % 2)


def xor_table(reps=10):
    a, b = np.repeat([0, 0, 1, 1], reps), np.repeat([0, 1, 0, 1], reps)
    return _coded([a, b], a ^ b)


def build_case(name):
    """dict(train, test, fake, kinds, cardinalities, p)"""
    if name.startswith("rows"):
        return _random_case(int(name[4:]), 3, [3, 4], 3)
    if name == "one_class":
        return _random_case(80, 3, [3, 4], 3, present=[1])
    if name == "no_valid":
        c = _random_case(40, 3, [3, 4], 3)
        c["fake"][:, c["kinds"].index(TARGET)] = float("nan")
        return c
    if name.startswith("classes"):
        K = int(name[7:])
        if K == 64:
            return _random_case(150, 1, [3], 64, n_real=200, n_test=80, trees=2, max_depth=3)
        return _random_case(120, 2, [3], K)
    if name == "absent":          # overflow codes and NaN targets in the generated table, absent classes
        c = _random_case(150, 3, [3, 5], 5, present=[1, 3])
        t, kinds = c["fake"], c["kinds"]
        tcol, ccol = kinds.index(TARGET), kinds.index(CAT)
        t[::7, tcol], t[3::11, tcol], t[5::13, tcol] = -1.0, float("nan"), 5.0
        t[::9, ccol], t[1::9, ccol], t[2::17, ccol] = 99.0, float("nan"), -2.0
        t[4::19, kinds.index(CONT)] = float("nan")
        c["test"][::10, tcol] = 7.0
        return c
    if name == "one_feature":
        return _random_case(100, 1, [], 3)
    if name in ("constant", "two_bins"):
        c = _random_case(100, 2, [3], 3)
        j = c["kinds"].index(CONT)
        for key in ("train", "test", "fake"):
            c[key][:, j] = 2.5 if name == "constant" else np.where(c[key][:, j] > 0, 1.0, -1.0)
        return c
    if name in ("cont256", "cont400"):
        c = _random_case(257, 2, [3], 3, n_real=300, n_test=100 if name == "cont256" else 150)
        j = c["kinds"].index(CONT)
        if name == "cont256":    # exactly 256 distinct values in the pooled real table
            c["train"][:, j] = np.arange(300) % 256 * 0.37
            c["test"][:, j] = np.arange(100) * 0.37
            c["fake"][:, j] = np.random.default_rng(4).uniform(-3, 98, 257)
        return c
    if name == "cat255":
        c = _random_case(300, 1, [255], 3, n_real=300)
        return c
    if name == "depth0":
        return _random_case(90, 3, [3, 4], 3, max_depth=0)
    if name == "depth1":
        return _random_case(90, 3, [3, 4], 3, max_depth=1)
    if name == "min_leaf3":
        return _random_case(200, 3, [3, 4], 3, min_leaf=3, max_depth=6)
    if name == "trees5":
        return _random_case(130, 3, [3, 4], 3, trees=5)
    if name in ("chain_short", "chain_full"):
        t = chain_table(16)
        return dict(train=t, test=t, fake=t, kinds=[CONT, TARGET], cardinalities=[2],
                    p=dict(P0, max_depth=3 if name == "chain_short" else 15))
    if name == "twins":           # two identical feature columns: the lower index wins
        c = _random_case(100, 2, [], 3)
        a, b = [j for j, k in enumerate(c["kinds"]) if k == CONT]
        for key in ("train", "test", "fake"):
            c[key][:, b] = c[key][:, a]
        return c
    if name == "symmetric":       # classes A B A over three values: both boundaries score the same, the lowest bin wins
        t = _coded([np.repeat([0, 1, 2], 6)], np.repeat([0, 1, 0], 6))
        return dict(train=t, test=t, fake=t, kinds=[CAT, TARGET], cardinalities=[3, 2], p=dict(P0))
    if name == "equal_masses":    # a root leaf with two equally heavy classes predicts the lower one
        t = _coded([np.arange(8) % 2], [0, 1, 0, 1, 1, 0, 1, 0])
        return dict(train=t, test=t, fake=t, kinds=[CAT, TARGET], cardinalities=[2, 2], p=dict(P0, max_depth=0))
    if name == "soft_tie":        # two rows, root leaves only: a seed under which the forest's votes tie exactly
        t = _coded([[0, 1]], [0, 1])
        for seed in range(64):
            tot = [0.0, 0.0]
            for tr in range(3):
                m = multiplicities(2, tr, seed, True)
                tot = [tot[c] + float(m[c]) / float(m.sum()) for c in range(2)]
            if tot[0] == tot[1]:
                return dict(train=t, test=t, fake=t, kinds=[CAT, TARGET], cardinalities=[2, 2],
                            p=dict(P0, max_depth=0, seed=seed))
        raise AssertionError("no seed ties the soft vote")
    if name == "xor":
        t = xor_table()
        return dict(train=t, test=t, fake=t, kinds=[CAT, CAT, TARGET], cardinalities=[2, 2, 2], p=dict(P0))
    raise KeyError(name)


CASES = ([f"rows{n}" for n in (1, 2, 63, 64, 65, 257, 513)] + ["one_class", "no_valid"] +
         [f"classes{K}" for K in (1, 2, 3, 64)] +
         ["absent", "one_feature", "constant", "two_bins", "cont256", "cont400", "cat255", "depth0", "depth1",
          "min_leaf3", "trees5", "chain_short", "chain_full", "twins", "symmetric", "equal_masses", "soft_tie", "xor"])
SMALLEST = "rows1"


def make_meta(kinds):
    return {"columns": [{"column_name": f"c{j}", "type": "continuous" if k == CONT else "categorical"}
                        for j, k in enumerate(kinds)], "non_negative_cols": [], "target": f"c{kinds.index(TARGET)}"}


def coded_evaluator(train, test, kinds, dev="cpu", ops=None, **kw):
    """DeviceForest on already coded real tables with the given column kinds"""
    return DeviceForest(np.asarray(train, dtype=np.float64), np.asarray(test, dtype=np.float64), make_meta(kinds), [],
                        dev, ops=ops, **kw)


def case_evaluator(c, dev, ops, **kw):
    p = c["p"]
    return coded_evaluator(c["train"], c["test"], c["kinds"], dev, ops, trees=p["trees"], max_depth=p["max_depth"],
                           min_leaf=p["min_leaf"], seed=p["seed"], max_rows=len(c["fake"]),
                           cardinalities=c["cardinalities"], **kw)


# ----------------------------------------------------------------------------- shared checks (CPU ops / HIP ops)
GUARD = 3


def run_ops(ops, ev, table, guard=GUARD):
    """pack -> per model bootstrap -> grow -> predict -> scores through ``ops`` on the constants of evaluator ``ev``,
    over fresh buffers whose tails carry a guard value that has to survive; returns numpy results"""
    dev = ev.device
    n, K = table.shape[0], ev.K
    values = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float64)).to(dev)
    tab = TreeTable(n + guard, ev.card, ev.edges, ev.eoff, ev.nbins, ev.max_bins, K, dev)
    tab.bins.fill_(249)
    tab.y.fill_(-7)
    ops.tree_pack(values, ev.kind, ev.slot, tab)
    assert bool((tab.bins[:, n:] == 249).all()) and bool((tab.y[n:] == -7).all()), "pack wrote past its rows"
    out = dict(bins=tab.bins[:, :n].cpu().numpy().astype(np.int64), y=tab.y[:n].cpu().numpy().astype(np.int64),
               counts=tab.counts.cpu().numpy().copy(), cw=tab.cw.cpu().numpy().copy())
    for i, (m, T, boot, m_feat) in enumerate((("dt", 1, False, ev.F), ("rf", ev.trees, True, ev.m_feat))):
        model = TreeModel(T, n + guard, K, ev.max_depth, dev)
        model.mult.fill_(-7)
        model.rows.fill_(-7)
        ops.tree_bootstrap(model.mult, n, boot, ev.seed)
        assert bool((model.mult[:, n:] == -7).all()), "bootstrap wrote past its rows"
        ops.tree_grow(tab, n, model, ev.max_depth, ev.min_leaf, m_feat, ev.seed)
        assert bool((model.mult[:, n:] == -7).all()) and bool((model.rows[:, :, n:] == -7).all()), "grow: row guard"
        conf_all = torch.full((K * K + guard,), -7, dtype=torch.int32, device=dev)
        sc_all = torch.full((6 + guard,), -7.0, dtype=torch.float64, device=dev)
        ops.tree_predict(ev.test, ev.n_test, tab.cw, model, boot, conf_all[:K * K].view(K, K))
        ops.tree_scores(conf_all[:K * K].view(K, K), ev.real[m], sc_all[:6])
        assert bool((conf_all[K * K:] == -7).all()) and bool((sc_all[6:] == -7).all()), "conf / scores guard"
        out[m] = dict(mult=model.mult[:, :n].cpu().numpy().astype(np.int64),
                      arrays={k: getattr(model, k).cpu().numpy().astype(np.int64)
                              for k in ("feature", "bin", "left", "heap", "counts")},
                      conf=conf_all[:K * K].view(K, K).cpu().numpy().astype(np.int64),
                      scores=sc_all[:6].cpu().numpy().copy())
    return out


def assert_trees(arrays, trees, what):
    """the ops' [T, cap] arrays against the brute force's trees: equal on the tree's nodes, unused beyond them"""
    for t, tree in enumerate(trees):
        m = len(tree["heap"])
        for k in ("feature", "bin", "left", "heap", "counts"):
            assert np.array_equal(arrays[k][t][:m], tree[k]), (what, t, k, arrays[k][t][:m], tree[k])
        assert (arrays["feature"][t][m:] == -1).all() and (arrays["heap"][t][m:] == 0).all(), (what, t, "tail")
        assert (arrays["counts"][t][m:] == 0).all() and (arrays["left"][t][m:] == 0).all(), (what, t, "tail")


def assert_side(got, want, K, what):
    assert np.array_equal(got["bins"], want["bins"]) and np.array_equal(got["y"], want["y"]), what + " bins"
    assert got["counts"].tolist() == want["counts"] and got["cw"].tolist() == want["w"], what + " weights"
    for m in ("dt", "rf"):
        assert np.array_equal(got[m]["mult"], want[m]["mult"]), f"{what} {m} multiplicities"
        assert_trees(got[m]["arrays"], want[m]["trees"], f"{what} {m}")
        assert np.array_equal(got[m]["conf"], want[m]["conf"]), f"{what} {m} confusion"
        for a, b in zip(got[m]["scores"][:2], want[m]["scores"]):
            assert abs(a - b) <= 8 * K * EPS, (what, m, a, b)


def same_results(a, b):
    """are two run_ops results equal bit for bit?"""
    ok = all(a[k].tobytes() == b[k].tobytes() for k in ("bins", "y", "counts", "cw"))
    for m in ("dt", "rf"):
        ok = ok and a[m]["mult"].tobytes() == b[m]["mult"].tobytes() and a[m]["conf"].tobytes() == b[m]["conf"].tobytes()
        ok = ok and a[m]["scores"].tobytes() == b[m]["scores"].tobytes()
        ok = ok and all(a[m]["arrays"][k].tobytes() == b[m]["arrays"][k].tobytes() for k in a[m]["arrays"])
    return ok


_EXPECTED = {}


def expected_case(name):
    """the brute force of a case, computed once and shared"""
    if name not in _EXPECTED:
        c = build_case(name)
        _EXPECTED[name] = (c, expected(c["train"], c["test"], c["fake"], c["kinds"], c["p"], c["cardinalities"]))
    return _EXPECTED[name]


def check_case(ops, dev, name, oracle_ops=None):
    """one case through ``ops``: op by op and end to end against the brute force, and (GPU) bit for bit against the
    oracle ops on the same device"""
    c, want = expected_case(name)
    K = want["K"]
    ev = case_evaluator(c, dev, ops)
    assert (ev.K, ev.card_list, ev.nbins_list) == (K, want["cards"], want["nbins"]), name
    assert [e.tolist() for e in ev.edges_list] == [e for e, k in zip(want["edges"], want["cards"]) if k == 0], name
    for m in ("dt", "rf"):       # the fits on the real training rows, done at construction
        assert np.array_equal(ev.conf_real[m].cpu().numpy(), want["real"][m]["conf"]), (name, m, "real")
    got = run_ops(ops, ev, c["fake"])
    assert_side(got, want["fake"], K, name)
    for m in ("dt", "rf"):
        assert all(int(row.sum()) == len(c["fake"]) for row in got[m]["mult"]), name + ": draws per tree"
    s = ev.score(torch.from_numpy(c["fake"]).to(dev))
    buf = s.buf.cpu().numpy()
    for key, v in zip(KEYS, buf):
        assert abs(v - want["scores"][key]) <= 8 * K * EPS, (name, key, v, want["scores"][key])
    for i, m in enumerate(("dt", "rf")):
        assert np.array_equal(s.confusion(m).cpu().numpy(), want["fake"][m]["conf"]), (name, m)
        assert buf[6 * i:6 * i + 6].tobytes() == got[m]["scores"].tobytes(), name + ": score() and the ops differ"
        for t, tree in enumerate(want["fake"][m]["trees"]):
            arr = {k: v.cpu().numpy()[None] for k, v in s.tree(m, t).items()}
            assert_trees(arr, [tree], f"{name} score() {m} {t}")
    if oracle_ops is not None:
        ref = run_ops(oracle_ops, ev, c["fake"])
        assert same_results(got, ref), name + ": HIP ops and TorchOps differ"
        rs = case_evaluator(c, dev, oracle_ops).score(torch.from_numpy(c["fake"]).to(dev))
        assert torch.equal(rs.buf.view(torch.int64), s.buf.view(torch.int64)), name + ": buf differs from TorchOps"
    return ev, c, got, want
