"""Shared cases of the MLP-utility tests (test_mlp.py on the CPU, test_hip_mlp.py on the GPU): a plain-numpy brute
force of the whole contract (eval/mlp_device.py), table builders and the bounds.

Nothing here uses TorchOps: the brute force builds the feature matrix F with its one-hot blocks
(utility_cases.features) and works on it with dense numpy products.

Bounds.  eps = 2^-52; gamma(m) = (m + 32) eps as in utility_cases.

* first gradient (derived): an entry of F^T dH is a sum over the batch's rows of products whose factors dH come from
  sums over K classes, which come from sums over H hidden units: 2 gamma(rows + H + K) times the same products taken
  on absolute values, (|F|^T ((|dZ| |W2|^T) . (h > 0)) + alpha |W1|) / m and (|[h | 1]|^T |dZ| + alpha |W2|) / m.
  The ops do not return the gradient; it is read off the first moment after one step, g = m_1 / 0.1, which adds
  4 eps |g|.
* theta after one step (derived): with a = 0.1 and s = sqrt(0.001), the first step is u(g) = lr_1 a g / (s |g| + 1e-8),
  and |du/dg| = lr_1 a 1e-8 / (s |g| + 1e-8)^2, largest at the end of [|g| - tol_g, |g| + tol_g] nearest 0: entrywise
  lr_1 a 1e-8 tol_g / (s max(|g| - tol_g, 0) + 1e-8)^2, plus 8 eps (|theta| + lr) for the step's own roundings.  This
  is up to 1e8 tol_g where |g| < 1e-8.
* theta after 5 and 20 steps: no bound can be derived, Adam divides by sqrt(v).  Measured instead, on the reference
  alone: the brute force summing a batch as a whole against summing it in row blocks of 64, over every table of the two
  test files at 5 and 20 steps.  The largest difference seen was THETA_SPREAD (below); the bound is 16 times that, the
  factor covering a third order, the MFMA's.  The two orders only differ where a batch has more than 64 rows, and what
  dominates the difference is the weight row of a rare one-hot bin: its gradient is alpha theta / m (1e-7) until the
  bin shows up in a batch, sqrt(v) stays near Adam's 1e-8, and a rounding of dH (1e-19 in g) is carried into theta
  times lr / (sqrt(v) + 1e-8), up to 1e5.  The case "wide512" (1,000 such bins, batches of six row blocks) is there
  so that the measurement sees this; it sets the figure.
* scores (derived): f1 and acc come from integers, 8 K eps.  loss: |df| <= sum |grad f| THETA_TOL + 2 gamma(n + H + K)
  f, with grad f the gradient of the objective over the whole table at the last theta.
* confusion matrices are compared on the rows whose two largest logits differ by more than 1e-9 max |z|
  (utility_cases.confident_rows); every case leaves at least 99 % of its test rows.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import utility_cases as uc
from fed_tgan_amd.eval import DeviceMLP
from fed_tgan_amd.eval.mlp_device import KEYS
from fed_tgan_amd.eval.utility_device import UtilityTable
from utility_cases import CAT, CONT, EPS, TARGET, gamma, worst

BLOCK = 64                  # MLP_ROWS: the row block of the blocked summation order
THETA_SPREAD = 7.6e-16      # measured (7.56e-16, measure_spread()): the largest |theta_whole - theta_blocked| at 5 and 20 steps
THETA_TOL = 16 * THETA_SPREAD
STEPS = (1, 5, 20)
LR, ALPHA, SEED = 1e-3, 1e-4, 0
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8


# ----------------------------------------------------------------------------- the brute force
def init_theta(D, H, K, seed):
    g = np.random.default_rng(seed)
    b1, b2 = math.sqrt(6.0 / (D - 1 + H)), math.sqrt(6.0 / (H + K))
    W1 = np.concatenate([g.uniform(-b1, b1, (D - 1, H)), g.uniform(-b1, b1, H)[None, :]], axis=0)
    W2 = np.concatenate([g.uniform(-b2, b2, (H, K)), g.uniform(-b2, b2, K)[None, :]], axis=0)
    return W1, W2


def flat(W1, W2):
    return np.concatenate([W1.reshape(-1), W2.reshape(-1)])


def batch_rows(n, batch, k):
    nb = (n + batch - 1) // batch
    return np.arange(k % nb, n, nb)


def forward(F, W1, W2):
    h = np.maximum(F @ W1, 0.0)
    return h, np.concatenate([h, np.ones((F.shape[0], 1))], axis=1) @ W2


def softmax_rows(Z, y, present):
    """(valid rows, P - Y with zero rows where y is no code, the rows' cross entropies)"""
    n, K = Z.shape
    valid = y < K
    dZ, ce = np.zeros((n, K)), np.zeros(n)
    for i in np.nonzero(valid)[0]:
        z = Z[i, present]
        mx = z.max()
        e = np.exp(z - mx)
        p = np.zeros(K)
        p[present] = e / e.sum()
        ce[i] = math.log(e.sum()) + mx - Z[i, y[i]]
        p[y[i]] -= 1.0
        dZ[i] = p
    return valid, dZ, ce


def objective(F, y, present, W1, W2, alpha, block=None):
    """(g1, g2, loss, parts) of the objective over the rows of F, the sums over rows as a whole or in row blocks"""
    n = F.shape[0]
    h, Z = forward(F, W1, W2)
    valid, dZ, ce = softmax_rows(Z, y, present)
    m = max(int(valid.sum()), 1)
    dH = (dZ @ W2[:-1].T) * (h > 0)
    h1 = np.concatenate([h, np.ones((n, 1))], axis=1)
    r1, r2 = np.ones((W1.shape[0], 1)), np.ones((W2.shape[0], 1))
    r1[-1] = r2[-1] = 0.0
    g1 = (uc._sum_rows(lambda lo, hi: F[lo:hi].T @ dH[lo:hi], n, block) + alpha * r1 * W1) / m
    g2 = (uc._sum_rows(lambda lo, hi: h1[lo:hi].T @ dZ[lo:hi], n, block) + alpha * r2 * W2) / m
    l2 = float((r1 * W1 * W1).sum() + (r2 * W2 * W2).sum())
    loss = (uc._sum_rows(lambda lo, hi: ce[lo:hi].sum(), n, block) + 0.5 * alpha * l2) / m
    return g1, g2, loss, dict(h=h, h1=h1, dZ=dZ, dH=dH, m=m)


def fit(F, y, K, H, steps, batch, checkpoints=(), block=None, lr=LR, alpha=ALPHA, seed=SEED):
    """the solver of the contract; returns a dict of everything the tests compare"""
    n, D = F.shape
    counts = np.bincount(y, minlength=K + 1)[:K]
    present = counts > 0
    W1, W2 = init_theta(D, H, K, seed)
    out = dict(counts=counts, present=present, F=F, y=y, theta0=flat(W1, W2), theta_at={}, H=H, batch=batch)
    theta = flat(W1, W2)
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    for k in range(steps):
        rows = batch_rows(n, batch, k)
        W1, W2 = theta[:D * H].reshape(D, H), theta[D * H:].reshape(H + 1, K)
        g1, g2, _, parts = objective(F[rows], y[rows], present, W1, W2, alpha, block)
        g = flat(g1, g2)
        if k == 0:
            out.update(G0=g, parts0=parts, rows0=rows, W1_0=W1.copy(), W2_0=W2.copy())
        t = k + 1
        m = B1 * m + (1.0 - B1) * g
        v = B2 * v + (1.0 - B2) * g * g
        theta = theta - lr * math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t) * m / (np.sqrt(v) + ADAM_EPS)
        if t in checkpoints:
            out["theta_at"][t] = theta.copy()
    W1, W2 = theta[:D * H].reshape(D, H), theta[D * H:].reshape(H + 1, K)
    g1, g2, loss, _ = objective(F, y, present, W1, W2, alpha, block)
    out.update(theta=theta, W1=W1, W2=W2, loss=loss, G=flat(g1, g2), lr=lr, alpha=alpha)
    return out


def predict(Ft, W1, W2, present):
    """(predictions, logits): the largest logit over the present classes, the lowest class on a tie, class 0 with no
    class present"""
    Z = forward(Ft, W1, W2)[1]
    pred = np.zeros(Ft.shape[0], dtype=np.int64)
    for i in range(Ft.shape[0]):
        best = -1
        for c in range(Z.shape[1]):
            if present[c] and (best < 0 or Z[i, c] > Z[i, best]):
                best = c
        pred[i] = max(best, 0)
    return pred, Z


def expected(train, test, fake, kinds, H, batch, steps, checkpoints=(), cardinalities=None, block=None, seed=SEED):
    """the whole contract by brute force"""
    cards, K, mean, sd = uc.setup(train, test, kinds, cardinalities)
    Ft, yt = uc.features(test, kinds, cards, K, mean, sd)
    out = {}
    for side, table in (("real", train), ("fake", fake)):
        F, y = uc.features(table, kinds, cards, K, mean, sd)
        f = fit(F, y, K, H, steps, batch, checkpoints, block, seed=seed)
        f["pred"], f["Zt"] = predict(Ft, f["W1"], f["W2"], f["present"])
        f["conf"] = uc.confusion(yt, f["pred"], K)
        f["f1"], f["acc"] = uc.conf_scores(f["conf"])
        out[side] = f
    r, k = out["real"], out["fake"]
    out["scores"] = dict(zip(KEYS, [k["f1"], k["acc"], r["f1"], r["acc"], r["f1"] - k["f1"], r["acc"] - k["acc"],
                                    k["loss"]]))
    out.update(cards=cards, K=K, mean=mean, sd=sd, yt=yt, Ft=Ft)
    return out


# ----------------------------------------------------------------------------- the derived bounds
def bounds(f):
    """entrywise / scalar bounds of one brute-force fit (see the module docstring)"""
    F, y, H = f["F"], f["y"], f["H"]
    n, D = F.shape
    K = f["W2"].shape[1]
    p, W1, W2 = f["parts0"], f["W1_0"], f["W2_0"]
    rows = len(f["rows0"])
    Fb = np.abs(F[f["rows0"]])
    r1, r2 = np.ones((D, 1)), np.ones((H + 1, 1))
    r1[-1] = r2[-1] = 0.0
    adH = (np.abs(p["dZ"]) @ np.abs(W2[:-1]).T) * (p["h"] > 0)
    t1 = (Fb.T @ adH + f["alpha"] * r1 * np.abs(W1)) / p["m"]
    t2 = (np.abs(p["h1"]).T @ np.abs(p["dZ"]) + f["alpha"] * r2 * np.abs(W2)) / p["m"]
    tol_G = 2 * gamma(rows + H + K) * flat(t1, t2) + 4 * EPS * np.abs(f["G0"]) + 1e-300
    a, s = 1.0 - B1, math.sqrt(1.0 - B2)
    lr1 = f["lr"] * s / a
    g_lo = np.maximum(np.abs(f["G0"]) - tol_G, 0.0)
    tol_T1 = lr1 * a * ADAM_EPS * tol_G / (s * g_lo + ADAM_EPS) ** 2 + 8 * EPS * (np.abs(f["theta0"]) + f["lr"])
    tol_loss = float(np.abs(f["G"]).sum()) * THETA_TOL + 2 * gamma(n + H + K) * f["loss"]
    return dict(G0=tol_G, T1=tol_T1, loss=tol_loss)


# ----------------------------------------------------------------------------- the cases of both test files
# name -> rows of the generated table, n_cont, cards of the categorical features, K, H, batch; "uc": the tables of
# that case of utility_cases
def _case(n=131, n_cont=5, cards=(3, 4), K=3, H=17, batch=64, **kw):
    return dict(n=n, n_cont=n_cont, cards=list(cards), K=K, H=H, batch=batch, **kw)


CASES = {f"rows{n}": _case(n=n) for n in (1, 63, 64, 65, 131)}      # 65 = batch + 1; 131 = 2 batch + 3: unequal
CASES["batch1"] = _case(n=40, batch=1)                              # batches, and b wraps within 20 steps
CASES["batch65"] = _case(batch=65)
CASES["batch512"] = _case(n=700, batch=512)
CASES.update({f"hidden{H}": _case(H=H) for H in (1, 15, 16, 17, 100, 128)})
CASES.update({f"classes{K}": _case(K=K) for K in (1, 2, 17, 64)})
CASES.update({f"cont{c}": _case(n_cont=c) for c in (0, 1, 4, 5, 17)})
CASES["absent"] = _case(uc="absent")                                # absent classes, NaN / negative / too-large
CASES["novalid"] = _case(novalid=1)                                 # targets, a feature value that is no code
CASES["wide"] = _case(uc="wide", H=128)                             # D = 1023, n = 50
CASES["wide512"] = _case(n=700, n_cont=17, cards=[200] * 5, H=128, batch=512)   # D = 1023 over batches of 6 row blocks


def build_case(name, n_real=400, n_test=150):
    """(train, test, fake, kinds, cardinalities): cardinalities in column order, the target's included"""
    c = CASES[name]
    if "uc" in c:
        return uc.build_case(c["uc"], n_real, n_test)
    kinds = uc.make_kinds(c["n_cont"], len(c["cards"]), seed=len(name))
    train = uc.random_table(n_real, kinds, 1, c["cards"], c["K"])
    test = uc.random_table(n_test, kinds, 2, c["cards"], c["K"])
    fake = uc.random_table(c["n"], kinds, 3, c["cards"], c["K"])
    if "novalid" in c:              # batch b = 1 of nb = 3 holds the rows 1, 4, 7, ...: none of them valid
        nb = (c["n"] + c["batch"] - 1) // c["batch"]
        assert nb == 3
        fake[c["novalid"]::nb, kinds.index(TARGET)] = -1.0
    it = iter(c["cards"])
    cardinalities = [c["K"] if k == TARGET else next(it) for k in kinds if k != CONT]
    return train, test, fake, kinds, cardinalities


def coded_evaluator(train, test, kinds, dev="cpu", ops=None, **kw):
    """DeviceMLP on already coded real tables with the given column kinds"""
    meta = {"columns": [{"column_name": f"c{j}", "type": "continuous" if k == CONT else "categorical"}
                        for j, k in enumerate(kinds)], "non_negative_cols": [], "target": f"c{kinds.index(TARGET)}"}
    return DeviceMLP(np.asarray(train, dtype=np.float64), np.asarray(test, dtype=np.float64), meta, [], dev,
                     ops=ops, **kw)


def intrusion_like(n, seed):
    """(kinds, cards, table) of the determinism test: 22 continuous and 8 categorical features, 5 classes"""
    kinds = uc.make_kinds(22, 8, seed=0)
    cards = [2 + (5 * s) % 9 for s in range(8)]
    return kinds, cards, uc.random_table(n, kinds, seed, cards, 5)


def generated_tables(device="cpu", backend="torch", n=1000):
    """the end-to-end test's tables: (real training frame, test frame, meta, vocabs, engine, generated [n, n_cols])"""
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.samplers import CondTables
    _, df, _, meta, vocabs, _, tr, X = uc.small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), device, backend=backend, seed=3)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    return df.iloc[:500], df.iloc[500:700], meta, vocabs, eng, eng.generate_decoded(n)


def measure_spread():
    """THETA_SPREAD: the largest |theta_whole - theta_blocked| at 5 and 20 steps over every table of the two test
    files (the cases, the determinism test's tables, the end-to-end test's); prints it per table"""
    from fed_tgan_amd.eval.privacy import code_real_table
    jobs = []
    for name, c in CASES.items():
        train, test, fake, kinds, cardinalities = build_case(name)
        jobs.append((name, train, test, fake, kinds, c["H"], c["batch"], cardinalities))
    kinds, _, real = intrusion_like(700, 1)
    test = intrusion_like(200, 2)[2]
    for i, n in ((10, 333), (11, 333), (20, 70)):
        jobs.append((f"intrusion{i}", real, test, intrusion_like(n, i)[2], kinds, 100, 512, None))
    train, test, meta, vocabs, _, vals = generated_tables()
    kinds = [TARGET if c["column_name"] == meta["target"] else CAT if c["type"] == "categorical" else CONT
             for c in meta["columns"]]
    jobs.append(("generated", code_real_table(train, meta, vocabs), code_real_table(test, meta, vocabs),
                 vals.numpy(), kinds, 100, 512, [len(v) for v in vocabs]))
    top = 0.0
    for name, train, test, fake, kinds, H, batch, cardinalities in jobs:
        a = expected(train, test, fake, kinds, H, batch, 20, (5, 20), cardinalities)
        b = expected(train, test, fake, kinds, H, batch, 20, (5, 20), cardinalities, block=BLOCK)
        d = max(float(np.abs(a[s]["theta_at"][k] - b[s]["theta_at"][k]).max()) for s in ("real", "fake") for k in (5, 20))
        print(f"{name}: {d:.3e}")
        top = max(top, d)
    print(f"THETA_SPREAD measured: {top:.3e}")
    return top


_EXPECTED = {}


def case_expected(name):
    """the tables of a case and its brute force, computed once and shared (read-only) by the tests"""
    if name not in _EXPECTED:
        train, test, fake, kinds, cardinalities = build_case(name)
        c = CASES[name]
        want = expected(train, test, fake, kinds, c["H"], c["batch"], max(STEPS), STEPS, cardinalities)
        _EXPECTED[name] = (train, test, fake, kinds, cardinalities, want)
    return _EXPECTED[name]


# ----------------------------------------------------------------------------- shared checks (CPU ops / HIP ops)
def run_ops(ops, ev, table, steps, guard=3):
    """pack -> ``steps`` steps -> loss -> predict through ``ops`` on the constants of evaluator ``ev``, over fresh
    buffers whose tails carry a guard value that has to survive; returns numpy results"""
    dev = ev.device
    n, D, K, H, R = table.shape[0], ev.D, ev.K, ev.hidden, int(ops.MLP_ROWS)
    f64 = dict(dtype=torch.float64, device=dev)
    values = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float64)).to(dev)
    tab = UtilityTable(n + guard, ev.n_cont, ev.card, ev.offs, D, K, dev)
    tab.cont.fill_(-7.0)
    tab.cat_t.fill_(-7)
    tab.y.fill_(-7)
    ops.util_pack(values, ev.kind, ev.slot, ev.mean, ev.sd, tab)
    P = D * H + (H + 1) * K
    nb = (n + ev.batch - 1) // ev.batch
    rows = (n + nb - 1) // nb                                     # the largest batch
    blocks = (rows + R - 1) // R

    def buf(size, **kw):
        full = torch.full((size + guard,), -7, **kw)
        return full, full[:size]

    (th_all, theta), (m_all, m), (v_all, v) = buf(P, **f64), buf(P, **f64), buf(P, **f64)
    (h_all, h), (dh_all, dh), (dz_all, dz) = buf(rows * H, **f64), buf(rows * H, **f64), buf(rows * K, **f64)
    cnt_all, cnt = buf(blocks, dtype=torch.int32, device=dev)
    loss_all, loss = buf(1 + (n + R - 1) // R, **f64)
    conf_all, conf = buf(K * K, dtype=torch.int32, device=dev)
    sc_all, sc = buf(len(KEYS), **f64)
    theta.copy_(ev.theta0)
    m.zero_()
    v.zero_()
    out = dict(y=tab.y[:n].cpu().numpy().copy(), counts=tab.counts.cpu().numpy().copy(), theta_at={})
    from fed_tgan_amd.eval.mlp_device import step_sizes
    for k, lr_t in enumerate(step_sizes(max(steps), ev.lr)):
        ops.mlp_step(tab, n, k % nb, nb, theta, m, v, h, dz, dh, cnt, H, ev.alpha, lr_t)
        if k == 0:
            out["G0"] = m.cpu().numpy() / (1.0 - B1)
            out["cnt0"] = cnt.cpu().numpy().copy()
        if k + 1 in steps:
            out["theta_at"][k + 1] = theta.cpu().numpy().copy()
    ops.mlp_loss(tab, n, theta, H, ev.alpha, loss)
    ops.mlp_predict(ev.test, ev.n_test, tab.counts, theta, H, conf.view(K, K), loss, ev.real, sc)
    for name, full, size in (("theta", th_all, P), ("m", m_all, P), ("v", v_all, P), ("h", h_all, rows * H),
                             ("dh", dh_all, rows * H), ("dz", dz_all, rows * K), ("cnt", cnt_all, blocks),
                             ("loss", loss_all, loss.numel()), ("conf", conf_all, K * K),
                             ("scores", sc_all, len(KEYS))):
        assert bool((full[size:] == -7).all()), f"{name} guard"
    assert bool((tab.cont[n:] == -7.0).all()) and bool((tab.cat_t[:, n:] == -7).all()), "pack wrote past its rows"
    assert bool((tab.y[n:] == -7).all()), "pack wrote past its rows"
    out.update(theta=theta.cpu().numpy().copy(), loss=float(loss[0]), conf=conf.view(K, K).cpu().numpy().copy(),
               scores=sc.cpu().numpy().copy())
    return out


def assert_fit(got, f, what, steps=STEPS, factor=1.0):
    """the first gradient and theta after each of ``steps`` against a brute-force fit f"""
    b = bounds(f)
    worst(got["G0"], f["G0"], factor * b["G0"], what + " G0")
    for k in steps:
        worst(got["theta_at"][k], f["theta_at"][k], factor * (b["T1"] if k == 1 else THETA_TOL),
              f"{what} theta after {k}")
    return b


def assert_scores(got, want: dict, b, K, what, factor=1.0):
    for i, k in enumerate(KEYS):
        tol = factor * (b["loss"] if k == "mlp_loss_fake" else 8 * K * EPS)
        print(f"{what} {k}: got {float(got[i])!r} want {want[k]!r} bound {tol:.3e}")
        assert abs(float(got[i]) - want[k]) <= tol, (what, k, float(got[i]), want[k])


def conf_on(ops, ev, test, rows, train_counts, theta):
    """the confusion matrix of ``ops`` over the given rows of the test table (packed afresh)"""
    dev = ev.device
    tab = UtilityTable(len(rows), ev.n_cont, ev.card, ev.offs, ev.D, ev.K, dev)
    ops.util_pack(torch.from_numpy(np.ascontiguousarray(test[rows])).to(dev), ev.kind, ev.slot, ev.mean, ev.sd, tab)
    conf = torch.zeros(ev.K, ev.K, dtype=torch.int32, device=dev)
    out = torch.zeros(len(KEYS), dtype=torch.float64, device=dev)
    ops.mlp_predict(tab, len(rows), torch.from_numpy(train_counts.astype(np.int32)).to(dev),
                    torch.from_numpy(theta).to(dev), ev.hidden, conf, out[:1].clone(), ev.real, out)
    return conf.cpu().numpy()


def check_case(ops, dev, name, oracle_ops=None, factor=1.0):
    """one case through ``ops``: op by op and end to end against the brute force at ``factor`` times the bounds, and
    (GPU) against the oracle ops on the same device at twice the bounds"""
    train, test, fake, kinds, cardinalities, want = case_expected(name)
    test = np.asarray(test, dtype=np.float64)
    c, f, K = CASES[name], want["fake"], want["K"]
    ev = coded_evaluator(train, test, kinds, dev, ops, hidden=c["H"], batch=c["batch"], steps=max(STEPS),
                         max_rows=len(fake), cardinalities=cardinalities)
    assert (ev.D, ev.K, ev.card_list) == (f["F"].shape[1], K, want["cards"])
    assert np.array_equal(ev.theta0.cpu().numpy(), f["theta0"]), name + ": theta0"
    got = run_ops(ops, ev, fake, STEPS)
    assert np.array_equal(got["y"], f["y"]) and np.array_equal(got["counts"], f["counts"]), name
    R = int(ops.MLP_ROWS)
    valid0 = (f["y"][f["rows0"]] < K).astype(np.int64)
    assert got["cnt0"].tolist() == [int(valid0[i:i + R].sum()) for i in range(0, len(valid0), R)], name
    b = assert_fit(got, f, name, STEPS, factor)
    worst(ev.theta_real.cpu().numpy(), want["real"]["theta"], factor * THETA_TOL, name + " theta_real")
    s = ev.score(torch.from_numpy(fake).to(dev))
    W1, W2 = s.weights()
    theta = np.concatenate([W1.cpu().numpy().reshape(-1), W2.cpu().numpy().reshape(-1)])
    worst(theta, f["theta"], factor * THETA_TOL, name + " score theta")
    assert theta.tobytes() == got["theta"].tobytes(), name + ": score() and the ops differ"
    # predictions: on the rows the reference itself is sure of
    yt, present = want["yt"], f["present"]
    rows = uc.confident_rows(f["Zt"], present)
    print(f"{name}: {len(test) - len(rows)} of {len(test)} test rows left out as ties")
    assert len(rows) >= 0.99 * len(test), name
    if len(rows) == len(test):
        assert np.array_equal(got["conf"], f["conf"]), name
        assert np.array_equal(s.confusion().cpu().numpy(), f["conf"]), name
        assert_scores(got["scores"][:2].tolist() + s.buf.cpu().tolist()[2:], want["scores"], b, K, name, factor)
    else:
        sure = uc.confusion(yt, f["pred"], K, rows)
        assert np.array_equal(conf_on(ops, ev, test, rows, f["counts"], got["theta"]), sure), name
    worst(got["loss"], f["loss"], factor * b["loss"], name + " loss")
    if oracle_ops is not None:
        ref = run_ops(oracle_ops, ev, fake, STEPS)
        assert np.array_equal(got["y"], ref["y"]) and np.array_equal(got["counts"], ref["counts"]), name
        assert np.array_equal(got["cnt0"], ref["cnt0"]), name
        assert_fit(ref, f, name + " oracle", STEPS)
        worst(got["G0"], ref["G0"], 2 * b["G0"], name + " G0 vs oracle")
        for k in STEPS:
            worst(got["theta_at"][k], ref["theta_at"][k], 2 * (b["T1"] if k == 1 else THETA_TOL),
                  f"{name} theta{k} vs oracle")
        worst(got["loss"], ref["loss"], 2 * b["loss"], name + " loss vs oracle")
        if len(rows) == len(test):
            assert np.array_equal(got["conf"], ref["conf"]), name
        else:
            assert np.array_equal(conf_on(ops, ev, test, rows, f["counts"], got["theta"]),
                                  conf_on(oracle_ops, ev, test, rows, f["counts"], ref["theta"])), name
    return ev, fake, got, want
