"""Cost of the on-device tree-utility evaluator (TSTR decision tree and random forest) on one GPU, by model, by op and
by level (profiles/forest_r10.md).

The table: n rows of the synthetic 42-column Intrusion schema as the "generated" table, an m-row draw as the real
table, split by index % 5 == 4 into training and held-out rows (tools/utility_probe.py's tables).  Arms, interleaved
rep by rep, device time from HIP events around each call, median and min .. max over the repetitions after a warm-up:

  * dt_graph / rf_graph   eval/forest_device.py DeviceForest.score (csrc/kernels/forest.hip) with one model, as a
                          hipGraph replay: pack, bootstrap, grow, predict, scores; dt_score / rf_score: the same, eager
  * pack, dt_grow, rf_bootstrap, rf_grow, dt_predict, rf_predict   the pass's ops one by one
  * rf_grow_d / dt_grow_d   growth limited to depth d = 0 .. max_depth: a level's cost is the difference of two
  * torch                 the same pass through TorchOps on the same device, with ``--torch-trees`` trees (wall time,
                          one repetition)

and, on the host, sklearn's DecisionTreeClassifier / RandomForestClassifier(n_jobs=16) at the same depth on the same
coded table, as wall time.

    python tools/forest_probe.py [--rows 40000] [--real 40000] [--trees 100] [--depth 12] [--reps 7] [--no-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def _timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def _summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=40000)
    ap.add_argument("--real", type=int, default=40000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-trees", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="skip the sklearn arms")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from fed_tgan_amd.data.demo import small_table
    from fed_tgan_amd.data.synthetic import generate_intrusion
    from fed_tgan_amd.eval.forest_device import DeviceForest
    from fed_tgan_amd.eval.privacy import code_real_table
    from fed_tgan_amd.ops.hip import HipOps
    from fed_tgan_amd.ops.ref import TorchOps
    if not torch.cuda.is_available():
        raise SystemExit("forest_probe: needs a GPU (a CPU timing says nothing about the device)")
    dev = torch.device("cuda:0")
    n, T, depth = args.rows, args.trees, args.depth
    _, _, _, meta, vocabs, _, _, _ = small_table()
    real = generate_intrusion(args.real, 7)
    held = np.arange(len(real)) % 5 == 4
    train, test = real[~held].reset_index(drop=True), real[held].reset_index(drop=True)
    fake = code_real_table(generate_intrusion(n, 9), meta, vocabs)
    vals = torch.from_numpy(fake).to(dev)
    ops = HipOps(dev)
    kw = dict(trees=T, max_depth=depth, max_rows=n)
    t0 = time.perf_counter()
    both = DeviceForest(train, test, meta, vocabs, dev, ops=ops, **kw)
    torch.cuda.synchronize(dev)
    construct_s = time.perf_counter() - t0
    ev = {m: DeviceForest(train, test, meta, vocabs, dev, ops=ops, models=(m,), **kw) for m in ("dt", "rf")}
    gr = {m: DeviceForest(train, test, meta, vocabs, dev, ops=ops, models=(m,), graph=True, **kw) for m in ("dt", "rf")}
    e = both
    dt, rf, tab = e.models["dt"], e.models["rf"], e.train
    arms = {
        "dt_score": lambda: ev["dt"].score(vals),
        "rf_score": lambda: ev["rf"].score(vals),
        "dt_graph": lambda: gr["dt"].score(vals),
        "rf_graph": lambda: gr["rf"].score(vals),
        "pack": lambda: ops.tree_pack(vals, e.kind, e.slot, tab),
        "dt_grow": lambda: ops.tree_grow(tab, n, dt, depth, e.min_leaf, e.F, e.seed),
        "rf_bootstrap": lambda: ops.tree_bootstrap(rf.mult, n, True, e.seed),
        "rf_grow": lambda: ops.tree_grow(tab, n, rf, depth, e.min_leaf, e.m_feat, e.seed),
        "dt_predict": lambda: ops.tree_predict(e.test, e.n_test, tab.cw, dt, False, e.conf["dt"]),
        "rf_predict": lambda: ops.tree_predict(e.test, e.n_test, tab.cw, rf, True, e.conf["rf"]),
    }
    for d in range(depth):
        arms[f"dt_grow_d{d}"] = (lambda d=d: ops.tree_grow(tab, n, dt, d, e.min_leaf, e.F, e.seed))
        arms[f"rf_grow_d{d}"] = (lambda d=d: ops.tree_grow(tab, n, rf, d, e.min_leaf, e.m_feat, e.seed))
    got = both.score(vals)
    ops.tree_bootstrap(dt.mult, n, False, e.seed)
    for fn in arms.values():          # warm-up: code objects, the graph capture
        fn()
        fn()
    times = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, fn in arms.items():
            times[k].append(_timed(fn, dev))
    arms["rf_grow"]()
    arms["dt_grow"]()
    nodes = {m: [int(x) for x in both.models[m].level[:, 2].cpu().tolist()] for m in ("dt", "rf")}
    res = {"rows": n, "train_rows": len(train), "test_rows": len(test), "columns": e.n_cols, "F": e.F, "K": e.K,
           "max_bins": e.max_bins, "trees": T, "max_depth": depth, "device": torch.cuda.get_device_name(0),
           "construct_s": construct_s, "scores": got.floats(), "dt_nodes": nodes["dt"][0],
           "rf_nodes_mean": sum(nodes["rf"]) / len(nodes["rf"])}
    for k, ms in times.items():
        res[k] = _summary(ms)
    print("hip arms done", {k: round(statistics.median(v), 3) for k, v in times.items()}, flush=True)
    if not args.no_torch:
        tt = args.torch_trees
        slow = DeviceForest(train, test, meta, vocabs, dev, ops=TorchOps(), trees=tt, max_depth=depth, max_rows=n)
        fast = DeviceForest(train, test, meta, vocabs, dev, ops=ops, trees=tt, max_depth=depth, max_rows=n)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ref = slow.score(vals)
        torch.cuda.synchronize(dev)
        torch_s = time.perf_counter() - t0
        same = bool(torch.equal(ref.buf.view(torch.int64), fast.score(vals).buf.view(torch.int64)))
        res["torch"] = {"wall_s": torch_s, "trees": tt, "reps": 1, "hip_same_trees_ms": _timed(lambda: fast.score(vals), dev),
                        "buf_bitwise_equal": same}
        print("torch", res["torch"], flush=True)
    if not args.no_host:
        from sklearn.ensemble import RandomForestClassifier
        from sklearn.tree import DecisionTreeClassifier
        names = [c["column_name"] for c in meta["columns"]]
        tcol = names.index(e.target)
        feat = [j for j in range(len(names)) if j != tcol]
        te = code_real_table(test, meta, vocabs)
        X, y = fake[:, feat], fake[:, tcol]
        t0 = time.perf_counter()
        sk = DecisionTreeClassifier(class_weight="balanced", max_depth=depth, random_state=0).fit(X, y)
        res["sklearn_dt"] = {"wall_s": time.perf_counter() - t0, "acc": float((sk.predict(te[:, feat]) == te[:, tcol]).mean())}
        t0 = time.perf_counter()
        sk = RandomForestClassifier(n_estimators=T, class_weight="balanced", max_depth=depth, n_jobs=16,
                                    random_state=0).fit(X, y)
        res["sklearn_rf"] = {"wall_s": time.perf_counter() - t0, "n_jobs": 16,
                             "acc": float((sk.predict(te[:, feat]) == te[:, tcol]).mean())}
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
