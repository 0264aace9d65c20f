"""Shared cases of the utility-evaluator tests (test_utility.py on the CPU, test_hip_utility.py on the GPU): a
plain-numpy brute force of the whole contract (eval/utility_device.py), table builders and the bounds.

Nothing here uses TorchOps: the brute force builds the feature matrix F with its one-hot blocks and works on it with
dense numpy products.

Bounds.  eps = 2^-52; gamma(m) = (m + 32) eps bounds the relative error of a sum of m products in any order, with
room for the divisions, exp and log around it (a few ulp each).

* pack (derived): a standardised value is one subtraction and one division, a weight two products and a division:
  4 eps relative.  Counts are integers.
* Gram (derived): |M - M'| <= 2 gamma(n) (|F|^T diag(s) |F| / 2 + diag(reg)) / S entrywise.
* M^-1 (derived): (A + E)^-1 - A^-1 = -A^-1 E A^-1 to first order, and an inverse through a Cholesky factor carries a
  forward error of c D eps |A| |A^-1|^2: every entry within 2 |A^-1|_2^2 (|tol_M|_F + 32 D eps |A|_2).
* one step (derived): W_1 = -M^-1 G_0, so |dW_1| <= tol_Minv colsum|G_0| + |M^-1| tol_G + gamma(D) |M^-1| |G_0|,
  with tol_G = 2 gamma(n + K) |F|^T |R| / S.
* W after several steps: no bound can be derived, the iteration may amplify a rounding difference.  Measured
  instead, on the reference alone: the brute force summing over the whole table against summing in row groups of
  UTIL_CHUNK rows, over every table of the two test files at 5 and 20 steps.  The largest difference seen was
  W_SPREAD (below); the bound is 16 times that, the factor covering a third order, the MFMA's.
* scores (derived): f1 and acc come from integers, 8 K eps.  loss: |df| <= sum|grad f| W_TOL + 2 gamma(n + K) f.
  grad: the Hessian is bounded by M (Boehning), so |dg| <= |M|_2 sqrt(D K) W_TOL + max tol_G.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from fed_tgan_amd.data.demo import small_table   # noqa: F401  (the front-end tests' table)
from fed_tgan_amd.eval import DeviceUtility
from fed_tgan_amd.eval.utility_device import KEYS, UtilityTable, momentum_table

CONT, CAT, TARGET = 0, 1, 2
EPS = 2.0 ** -52
CHUNK = 128                 # UTIL_CHUNK: the row group of the chunked summation order
W_SPREAD = 2.3e-14          # measured (2.21e-14): the largest |W_whole - W_chunked| over the tests' tables at 5 and 20 steps
W_TOL = 16 * W_SPREAD


def gamma(m):
    return (m + 32) * EPS


# ----------------------------------------------------------------------------- the brute force
def codes_of(col, K):
    """the overflow rule: a value that is NaN or no code of [0, K) is the extra category K"""
    with np.errstate(invalid="ignore"):
        ok = (col >= 0) & (col < K)
    return np.where(ok, np.where(ok, col, 0.0), float(K)).astype(np.int64)


def setup(train, test, kinds, cardinalities=None):
    """the evaluator's constants from the pooled real table: (feature cards, K, mean, sd)"""
    pooled = np.concatenate([train, test], axis=0)
    cat = [j for j, k in enumerate(kinds) if k != CONT]
    cards = {j: 1 + int(pooled[:, j].max()) for j in cat}
    if cardinalities is not None:
        for j, c in zip(cat, cardinalities):
            cards[j] = max(cards[j], int(c))
    cont = [j for j, k in enumerate(kinds) if k == CONT]
    mean = pooled[:, cont].mean(axis=0) if cont else np.zeros(0)
    sd = pooled[:, cont].std(axis=0) if cont else np.zeros(0)
    sd = np.where(sd > 0, sd, 1.0)
    K = cards[kinds.index(TARGET)]
    return [cards[j] for j, k in enumerate(kinds) if k == CAT], K, mean, sd


def features(table, kinds, cards, K, mean, sd):
    """(F [n, D] with its one-hot blocks, y with K for a value that is no code)"""
    table = np.asarray(table, dtype=np.float64)
    n = table.shape[0]
    cont = [j for j, k in enumerate(kinds) if k == CONT]
    blocks = [(table[:, cont] - mean[None, :]) / sd[None, :]]
    it = iter(cards)
    for j, k in enumerate(kinds):
        if k == CAT:
            Kc = next(it)
            oh = np.zeros((n, Kc + 1))
            oh[np.arange(n), codes_of(table[:, j], Kc)] = 1.0
            blocks.append(oh)
    blocks.append(np.ones((n, 1)))
    return np.concatenate(blocks, axis=1), codes_of(table[:, kinds.index(TARGET)], K)


def sample_weights(y, K):
    counts = np.bincount(y, minlength=K + 1)[:K]
    nv, present = int(counts.sum()), int((counts > 0).sum())
    s = np.zeros(len(y))
    for i, c in enumerate(y):
        if c < K:
            s[i] = nv / (present * counts[c])
    S = float(s.sum())
    return counts, s, (S if S > 0 else 1.0), nv, present


def _sum_rows(fn, n, chunk):
    """sum of fn(lo, hi) over the whole table (chunk None) or over row groups, in group order"""
    if chunk is None:
        return fn(0, n)
    acc = None
    for lo in range(0, n, chunk):
        v = fn(lo, min(n, lo + chunk))
        acc = v if acc is None else acc + v
    return acc


def gradient(F, s, y, present, P, S, chunk=None):
    """(grad f(P), f(P), R, Z) by dense products"""
    n, D = F.shape
    K = P.shape[1]
    Z = F @ P
    R = np.zeros((n, K))
    rows = np.zeros(n)
    for i in range(n):
        if s[i] > 0:
            z = Z[i, present]
            mx = z.max()
            e = np.exp(z - mx)
            p = np.zeros(K)
            p[present] = e / e.sum()
            rows[i] = s[i] * (math.log(e.sum()) + mx - Z[i, y[i]])
            p[y[i]] -= 1.0
            R[i] = s[i] * p
    g = _sum_rows(lambda lo, hi: F[lo:hi].T @ R[lo:hi], n, chunk)
    reg = np.ones((D, 1))
    reg[D - 1] = 0.0
    loss = (_sum_rows(lambda lo, hi: rows[lo:hi].sum(), n, chunk) + 0.5 * float((reg * P * P).sum())) / S
    return (g + reg * P) / S, loss, R, Z


def fit(F, y, K, iters, checkpoints=(), chunk=None):
    """the solver of the contract; returns a dict of everything the tests compare"""
    n, D = F.shape
    counts, s, S, nv, present_n = sample_weights(y, K)
    present = counts > 0
    reg = np.ones(D)
    reg[D - 1] = 0.0
    gram = _sum_rows(lambda lo, hi: F[lo:hi].T @ (s[lo:hi, None] * F[lo:hi]), n, chunk)
    M = (0.5 * gram + np.diag(reg)) / S
    A = M + np.eye(D) * (1e-10 * np.trace(M) / D)
    Minv = np.linalg.inv(A)
    Minv = 0.5 * (Minv + Minv.T)
    W, V = np.zeros((D, K)), np.zeros((D, K))
    betas = momentum_table(iters)
    out = dict(counts=counts, s=s, S=S, n_valid=nv, present=present, M=M, A=A, Minv=Minv, W_at={}, F=F, y=y)
    g0, _, R0, _ = gradient(F, s, y, present, V, S, chunk)
    out["G0"], out["R0"] = g0, R0
    for k in range(iters):
        g, _, _, _ = gradient(F, s, y, present, V, S, chunk)
        wn = V - Minv @ g
        V = wn + betas[k] * (wn - W)
        W = wn
        if k + 1 in checkpoints:
            out["W_at"][k + 1] = W.copy()
    g, loss, _, _ = gradient(F, s, y, present, W, S, chunk)
    out.update(W=W, G=g, loss=loss, grad=float(np.abs(g).max()))
    return out


def predict(F, W, present):
    """(predictions, logits): the largest logit over the present classes, the lowest class on a tie, class 0 with no
    class present"""
    Z = F @ W
    pred = np.zeros(F.shape[0], dtype=np.int64)
    for i in range(F.shape[0]):
        best = -1
        for c in range(W.shape[1]):
            if present[c] and (best < 0 or Z[i, c] > Z[i, best]):
                best = c
        pred[i] = max(best, 0)
    return pred, Z


def confusion(y, pred, K, rows=None):
    conf = np.zeros((K, K), dtype=np.int64)
    for i in (range(len(y)) if rows is None else rows):
        if y[i] < K:
            conf[y[i], pred[i]] += 1
    return conf


def conf_scores(conf):
    """(weighted F1, accuracy)"""
    total = int(conf.sum())
    if total == 0:
        return 0.0, 0.0
    f1 = 0.0
    for c in range(conf.shape[0]):
        tp, rs, cs = int(conf[c, c]), int(conf[c].sum()), int(conf[:, c].sum())
        if rs + cs > 0:
            f1 += rs * (2.0 * tp / (rs + cs))
    return f1 / total, float(np.trace(conf)) / total


def expected(train, test, fake, kinds, iters, checkpoints=(), cardinalities=None, chunk=None):
    """the whole contract by brute force"""
    cards, K, mean, sd = setup(train, test, kinds, cardinalities)
    Ft, yt = features(test, kinds, cards, K, mean, sd)
    out = {}
    for side, table in (("real", train), ("fake", fake)):
        F, y = features(table, kinds, cards, K, mean, sd)
        f = fit(F, y, K, iters, checkpoints, chunk)
        f["pred"], f["Zt"] = predict(Ft, f["W"], f["present"])
        f["conf"] = confusion(yt, f["pred"], K)
        f["f1"], f["acc"] = conf_scores(f["conf"])
        out[side] = f
    r, k = out["real"], out["fake"]
    out["scores"] = dict(zip(KEYS, [k["f1"], k["acc"], r["f1"], r["acc"], r["f1"] - k["f1"], r["acc"] - k["acc"],
                                    k["loss"], k["grad"]]))
    out.update(cards=cards, K=K, mean=mean, sd=sd, yt=yt, Ft=Ft)
    return out


# ----------------------------------------------------------------------------- the derived bounds
def bounds(f):
    """entrywise / scalar bounds of one brute-force fit (see the module docstring)"""
    F, s, S = np.abs(f["F"]), f["s"], f["S"]
    n, D = F.shape
    K = f["W"].shape[1]
    reg = np.ones(D)
    reg[D - 1] = 0.0
    tol_M = 2 * gamma(n) * (0.5 * F.T @ (s[:, None] * F) + np.diag(reg)) / S
    inv2 = np.linalg.norm(f["Minv"], 2)
    tol_Minv = 2 * inv2 * inv2 * (np.linalg.norm(tol_M) + 32 * D * EPS * np.linalg.norm(f["A"], 2))
    tol_G = 2 * gamma(n + K) * (F.T @ np.abs(f["R0"])) / S + 4 * EPS
    aminv, ag0 = np.abs(f["Minv"]), np.abs(f["G0"])
    tol_W1 = tol_Minv * ag0.sum(axis=0)[None, :] + aminv @ tol_G + gamma(D) * (aminv @ ag0)
    tol_loss = float(np.abs(f["G"]).sum()) * W_TOL + 2 * gamma(n + K) * f["loss"]
    tol_grad = np.linalg.norm(f["M"], 2) * math.sqrt(D * K) * W_TOL + float(tol_G.max())
    return dict(M=tol_M, Minv=tol_Minv, G0=tol_G, W1=tol_W1, loss=tol_loss, grad=tol_grad)


# ----------------------------------------------------------------------------- tables
def make_kinds(n_cont, n_cat, seed=0):
    kinds = np.array([CONT] * n_cont + [CAT] * n_cat + [TARGET])
    np.random.default_rng(seed).shuffle(kinds)
    return kinds.tolist()


def random_table(n, kinds, seed, cards, K, sep=1.0, present=None):
    """a coded table: the target is drawn first (from ``present`` classes, default all K), every feature leans on it
    with noise, so the classes overlap and the optimum is finite"""
    g = np.random.default_rng(seed)
    classes = np.arange(K) if present is None else np.asarray(present)
    y = classes[g.integers(0, len(classes), n)]
    colrng = np.random.default_rng(12345)         # the columns' dependence on the class: the same for every table
    t = np.zeros((n, len(kinds)))
    s = 0
    for j, k in enumerate(kinds):
        if k == TARGET:
            t[:, j] = y
        elif k == CAT:
            Kc = cards[s]
            s += 1
            shift = colrng.integers(0, Kc, K)
            t[:, j] = np.where(g.random(n) < 0.6, shift[y] % Kc, g.integers(0, Kc, n))
        else:
            mu = colrng.normal(size=K) * sep
            t[:, j] = mu[y] + g.normal(size=n) + 3.0 * colrng.normal()
    return t


def coded_evaluator(train, test, kinds, dev="cpu", ops=None, **kw):
    """DeviceUtility on already coded real tables with the given column kinds"""
    meta = {"columns": [{"column_name": f"c{j}", "type": "continuous" if k == CONT else "categorical"}
                        for j, k in enumerate(kinds)], "non_negative_cols": [], "target": f"c{kinds.index(TARGET)}"}
    return DeviceUtility(np.asarray(train, dtype=np.float64), np.asarray(test, dtype=np.float64), meta, [], dev,
                         ops=ops, **kw)


# ----------------------------------------------------------------------------- shared checks (CPU ops / HIP ops)
def run_ops(ops, ev, table, steps, guard=3):
    """pack -> gram -> factor -> ``steps`` steps -> grad -> predict through ``ops`` on the constants of evaluator
    ``ev``, over fresh buffers whose tails carry a guard value that has to survive; returns numpy results"""
    dev = ev.device
    n, D, K = table.shape[0], ev.D, ev.K
    f64 = dict(dtype=torch.float64, device=dev)
    values = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float64)).to(dev)
    tab = UtilityTable(n + guard, ev.n_cont, ev.card, ev.offs, D, K, dev)
    tab.cont.fill_(-7.0)
    tab.cat_t.fill_(-7)
    tab.y.fill_(-7)
    tab.s.fill_(-7.0)
    used = ops.util_part(n, D, K)
    part = torch.full((used + guard,), -7.0, **f64)
    groups = ops.util_groups(n, D * K)
    lossp = torch.full((groups + guard,), -7.0, **f64)

    def mat(r, c):
        full = torch.full((r * c + guard,), -7.0, **f64)
        return full, full[:r * c].view(r, c)

    (m_all, M), (mi_all, Minv), (_, Lt), (_, X) = mat(D, D), mat(D, D), mat(D, D), mat(D, D)
    (w_all, W), (v_all, V), (g_all, G) = mat(D, K), mat(D, K), mat(D, K)
    loss = torch.zeros(1, **f64)
    ops.util_pack(values, ev.kind, ev.slot, ev.mean, ev.sd, tab)
    out = dict(cont=tab.cont[:n].cpu().numpy().copy(), cat_t=tab.cat_t[:, :n].cpu().numpy().copy(),
               y=tab.y[:n].cpu().numpy().copy(), s=tab.s[:n].cpu().numpy().copy(),
               counts=tab.counts.cpu().numpy().copy(), info=tab.info.cpu().numpy().copy())
    ops.util_gram(tab, n, M, part)
    ops.util_factor(M, Lt, X, Minv)
    out["M"], out["Minv"] = M.cpu().numpy().copy(), Minv.cpu().numpy().copy()
    W.zero_()
    V.zero_()
    ops.util_grad(tab, n, V, G, loss, part, lossp)
    out["G0"] = G.cpu().numpy().copy()
    out["W_at"] = {}
    for k, beta in enumerate(momentum_table(max(steps))):
        ops.util_step(tab, n, V, W, Minv, G, loss, part, lossp, beta)
        if k + 1 in steps:
            out["W_at"][k + 1] = W.cpu().numpy().copy()
    ops.util_grad(tab, n, W, G, loss, part, lossp)
    conf_all = torch.full((K * K + guard,), -7, dtype=torch.int32, device=dev)
    conf = conf_all[:K * K].view(K, K)
    sc_all = torch.full((8 + guard,), -7.0, **f64)
    ops.util_predict(ev.test, ev.n_test, tab.counts, W, conf, G, loss, ev.real, sc_all[:8])
    for name, full, size in (("M", m_all, D * D), ("Minv", mi_all, D * D), ("W", w_all, D * K), ("V", v_all, D * K),
                             ("G", g_all, D * K), ("part", part, used), ("lossp", lossp, groups),
                             ("conf", conf_all, K * K), ("scores", sc_all, 8)):
        assert bool((full[size:] == -7).all()), f"{name} guard"
    assert bool((tab.cont[n:] == -7.0).all()) and bool((tab.cat_t[:, n:] == -7).all()), "pack wrote past its rows"
    assert bool((tab.y[n:] == -7).all()) and bool((tab.s[n:] == -7.0).all()), "pack wrote past its rows"
    out.update(W=W.cpu().numpy().copy(), G=G.cpu().numpy().copy(), loss=float(loss[0]),
               conf=conf.cpu().numpy().copy(), scores=sc_all[:8].cpu().numpy().copy())
    return out


def worst(got, want, tol, what):
    """largest |got - want| / tol, printed before it is asserted"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    if got.size == 0:
        return
    err = np.abs(got - want)
    ratio = float((err / np.broadcast_to(tol, err.shape)).max())
    print(f"{what}: worst |diff| = {float(err.max()):.3e}, {ratio:.3g} of its bound")
    assert ratio <= 1.0, (what, float(err.max()), ratio)


def assert_pack(got, f, ev, what):
    """the pack outputs of run_ops against a brute-force fit f: integers equal, fp64 within 4 eps"""
    n, nc = f["F"].shape[0], ev.n_cont
    assert np.array_equal(got["y"], f["y"]), what
    assert np.array_equal(got["counts"], f["counts"]), what
    worst(got["cont"], f["F"][:, :nc], 4 * EPS * np.abs(f["F"][:, :nc]) + 1e-300, what + " cont")
    offs = ev.offs.cpu().tolist()
    for c in range(ev.n_cat):
        block = f["F"][:, nc + offs[c]:nc + offs[c + 1]]
        assert np.array_equal(got["cat_t"][c], block.argmax(axis=1)), (what, c)
    worst(got["s"], f["s"], 4 * EPS * f["s"] + 1e-300, what + " s")
    assert got["info"][0] == f["n_valid"] and got["info"][1] == int(f["present"].sum()), what
    worst(got["info"][2], f["S"], gamma(n) * f["S"], what + " S")


def assert_fit(got, f, what, steps=(1, 5, 20)):
    """M, M^-1, the first gradient and W after each of ``steps`` against a brute-force fit f"""
    b = bounds(f)
    worst(got["M"], f["M"], b["M"] + 1e-300, what + " M")
    worst(got["Minv"], f["Minv"], b["Minv"], what + " Minv")
    worst(got["G0"], f["G0"], b["G0"], what + " G0")
    for k in steps:
        worst(got["W_at"][k], f["W_at"][k], b["W1"] + 1e-300 if k == 1 else W_TOL, f"{what} W after {k}")
    return b


def assert_scores(got, want: dict, b, K, what):
    for i, k in enumerate(KEYS):
        tol = b["loss"] if k == "loss_fake" else b["grad"] if k == "grad_fake" else 8 * K * EPS
        print(f"{what} {k}: got {float(got[i])!r} want {want[k]!r} bound {tol:.3e}")
        assert abs(float(got[i]) - want[k]) <= tol, (what, k, float(got[i]), want[k])


def confident_rows(Z, present, rel=1e-9):
    """rows of logits whose two largest values over the present classes differ by more than rel max |logit|"""
    Zp = np.sort(Z[:, present], axis=1)
    if Zp.shape[1] < 2:
        return np.arange(Z.shape[0])
    return np.nonzero(Zp[:, -1] - Zp[:, -2] > rel * np.abs(Z).max())[0]


def conf_on(ops, ev, rows, train_counts, W):
    """the confusion matrix of ``ops`` over the given rows of the evaluator's test table (packed afresh)"""
    dev = ev.device
    tab = UtilityTable(len(rows), ev.n_cont, ev.card, ev.offs, ev.D, ev.K, dev)
    ops.util_pack(torch.from_numpy(np.ascontiguousarray(ev._test_coded[rows])).to(dev), ev.kind, ev.slot, ev.mean,
                  ev.sd, tab)
    conf = torch.zeros(ev.K, ev.K, dtype=torch.int32, device=dev)
    out = torch.zeros(8, dtype=torch.float64, device=dev)
    G = torch.zeros(ev.D, ev.K, dtype=torch.float64, device=dev)
    ops.util_predict(tab, len(rows), torch.from_numpy(train_counts.astype(np.int32)).to(dev),
                     torch.from_numpy(W).to(dev), conf, G, out[:1].clone(), ev.real, out)
    return conf.cpu().numpy()


# ----------------------------------------------------------------------------- the cases of both test files
# name -> (rows of the generated table, n_cont, cards of the categorical features, K, classes present in it or None)
CASES = {f"rows{n}": (n, 5, [3, 4], 3, None) for n in (1, 63, 64, 65, 2 * CHUNK + 1)}
CASES.update({f"cont{c}": (333, c, [1, 2, 70], 3, None) for c in (0, 1, 16, 17, 33)})
CASES.update({f"classes{K}": (300, 3, [3], K, None) for K in (1, 2, 3, 17, 64)})
CASES["absent"] = (300, 4, [3, 5], 4, [0, 1, 3])
CASES["wide"] = (50, 17, [200] * 5, 3, None)                 # D = 17 + 5 * 201 + 1 = 1023
STEPS = (1, 5, 20)


def build_case(name, n_real=400, n_test=150):
    """(train, test, fake, kinds, cardinalities): cardinalities in column order, the target's included"""
    n, n_cont, cards, K, present = CASES[name]
    kinds = make_kinds(n_cont, len(cards), seed=len(name))
    train = random_table(n_real, kinds, 1, cards, K)
    test = random_table(n_test, kinds, 2, cards, K)
    fake = random_table(n, kinds, 3, cards, K, present=present)
    tcol = kinds.index(TARGET)
    if name == "absent":            # target overflow rows in the generated table, and a feature value that is no code
        fake[::7, tcol] = -1.0
        fake[3::11, tcol] = float("nan")
        fake[5::13, tcol] = float(K)
        fake[::9, kinds.index(CAT)] = 99.0
        test[::10, tcol] = float(K + 2)
    it = iter(cards)
    cardinalities = [K if k == TARGET else next(it) for k in kinds if k != CONT]
    return train, test, fake, kinds, cardinalities


def check_case(ops, dev, name, oracle_ops=None):
    """one case through ``ops``: op by op and end to end against the brute force, and (GPU) against the oracle ops
    on the same device"""
    train, test, fake, kinds, cardinalities = build_case(name)
    want = expected(train, test, fake, kinds, max(STEPS), STEPS, cardinalities)
    f, K = want["fake"], want["K"]
    ev = coded_evaluator(train, test, kinds, dev, ops, iters=max(STEPS), max_rows=len(fake),
                         cardinalities=cardinalities)
    ev._test_coded = np.asarray(test, dtype=np.float64)
    assert (ev.D, ev.K, ev.card_list) == (f["F"].shape[1], K, want["cards"])
    got = run_ops(ops, ev, fake, STEPS)
    assert_pack(got, f, ev, name)
    b = assert_fit(got, f, name, STEPS)
    worst(ev.W_real.cpu().numpy(), want["real"]["W"], W_TOL, name + " W_real")
    s = ev.score(torch.from_numpy(fake).to(dev))
    worst(s.weights().cpu().numpy(), f["W"], W_TOL, name + " score W")
    assert s.weights().cpu().numpy().tobytes() == got["W"].tobytes(), name + ": score() and the ops differ"
    # predictions: on the rows the reference itself is sure of
    yt, present = want["yt"], f["present"]
    rows = confident_rows(want["Ft"] @ f["W"], present)
    print(f"{name}: {len(test) - len(rows)} of {len(test)} test rows left out as ties")
    assert len(rows) >= 0.99 * len(test), name
    if len(rows) == len(test):
        assert np.array_equal(got["conf"], f["conf"]), name
        assert np.array_equal(s.confusion().cpu().numpy(), f["conf"]), name
        assert_scores(got["scores"][:2].tolist() + s.buf.cpu().tolist()[2:], want["scores"], b, K, name)
    else:
        sure = confusion(yt, f["pred"], K, rows)
        assert np.array_equal(conf_on(ops, ev, rows, f["counts"], got["W"]), sure), name
    if oracle_ops is not None:
        ref = run_ops(oracle_ops, ev, fake, STEPS)
        for key in ("y", "counts", "cat_t"):
            assert np.array_equal(got[key], ref[key]), (name, key)
        assert_pack(ref, f, ev, name + " oracle")
        assert_fit(ref, f, name + " oracle", STEPS)
        worst(got["cont"], ref["cont"], 8 * EPS * np.abs(ref["cont"]) + 1e-300, name + " cont vs oracle")
        worst(got["M"], ref["M"], 2 * b["M"] + 1e-300, name + " M vs oracle")
        worst(got["Minv"], ref["Minv"], 2 * b["Minv"], name + " Minv vs oracle")
        for k in STEPS:
            worst(got["W_at"][k], ref["W_at"][k], 2 * (b["W1"] + 1e-300 if k == 1 else W_TOL), f"{name} W{k} vs oracle")
        rows = confident_rows(want["Ft"] @ ref["W"], present)
        assert len(rows) >= 0.99 * len(test), name
        if len(rows) == len(test):
            assert np.array_equal(got["conf"], ref["conf"]), name
        else:
            assert np.array_equal(conf_on(ops, ev, rows, f["counts"], got["W"]),
                                  conf_on(oracle_ops, ev, rows, f["counts"], ref["W"])), name
    return ev, fake, got, want
