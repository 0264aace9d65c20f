"""Cost and quality of the on-device utility evaluator (TSTR logistic regression) on one GPU, by arm and by launch
(profiles/utility_r9.md).

The table: n rows of the synthetic 42-column Intrusion schema as the "generated" table (a fresh draw of the same
generator of rows: the fit is a meaningful one), an m-row draw as the real table, split by index % 5 == 4 into
training and held-out rows.  Arms, interleaved rep by rep, device time from HIP events around each call, median and
min .. max over the repetitions after a warm-up:

  * score / graph   eval/utility_device.py DeviceUtility.score (csrc/kernels/utility.hip), eager and as a hipGraph
                    replay: pack, gram, factor, ``iters`` steps, the final gradient, predict
  * pack, gram, factor, step, grad, predict   the pass's ops one by one; step and gram with the flops they imply
  * torch           the same pass through TorchOps on the same device in the same process, with ``--torch-iters``
                    iterations only (wall time, one repetition): its index_add_ calls are contended fp64 atomics

and, on the host, for scale: sklearn's LogisticRegression run to convergence on the same feature matrix (its F1 on
the held-out rows against the evaluator's), and eval/utility.py ``real_res`` (the reference's four classifiers
through sklearn on the frames), both as wall time.

    python tools/utility_probe.py [--rows 40000] [--real 40000] [--iters 200] [--reps 5]
                                  [--no-host | --host-only] [--lr-tol 1e-10]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

FP64_PEAK = 78.6e12     # MI355X fp64 matrix peak, AMD's published figure (flop / s)
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


def _weighted_f1(y, pred, K):
    conf = np.zeros((K, K), dtype=np.int64)
    np.add.at(conf, (y, pred), 1)
    rs, cs, tp = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
    den = rs + cs
    f = np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)
    return float((rs * f).sum() / max(conf.sum(), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=40000)
    ap.add_argument("--real", type=int, default=40000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-iters", type=int, default=5)
    ap.add_argument("--lr-tol", type=float, default=1e-10, help="tol of the sklearn LogisticRegression arm")
    ap.add_argument("--no-host", action="store_true", help="skip the sklearn arms")
    ap.add_argument("--host-only", action="store_true", help="only the sklearn arms (needs no GPU)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from fed_tgan_amd.data.demo import small_table
    from fed_tgan_amd.data.synthetic import generate_intrusion
    from fed_tgan_amd.eval.privacy import code_real_table
    from fed_tgan_amd.eval.utility_device import DeviceUtility
    from fed_tgan_amd.ops.hip import HipOps
    from fed_tgan_amd.ops.ref import TorchOps
    if not args.host_only and not torch.cuda.is_available():
        raise SystemExit("utility_probe: needs a GPU (a CPU timing says nothing about the device)")
    dev = torch.device("cpu" if args.host_only else "cuda:0")
    n, iters = args.rows, args.iters
    spec, _, _, meta, vocabs, _, _, _ = small_table()
    real = generate_intrusion(args.real, 7)
    held = np.arange(len(real)) % 5 == 4
    train, test = real[~held].reset_index(drop=True), real[held].reset_index(drop=True)
    fake_frame = generate_intrusion(n, 9)
    fake = code_real_table(fake_frame, meta, vocabs)
    vals = torch.from_numpy(fake).to(dev)
    if args.host_only:
        e = DeviceUtility(train, test, meta, vocabs, dev, ops=TorchOps(), iters=0, max_rows=1)
        K = e.K
        res = {"rows": n, "train_rows": len(train), "test_rows": len(test), "D": e.D, "K": K, "host_only": True}
    else:
        ops = HipOps(dev)
        t0 = time.perf_counter()
        eager = DeviceUtility(train, test, meta, vocabs, dev, ops=ops, iters=iters, max_rows=n)
        torch.cuda.synchronize(dev)
        construct_s = time.perf_counter() - t0
        graph = DeviceUtility(train, test, meta, vocabs, dev, ops=ops, iters=iters, max_rows=n, graph=True)
        e = eager
        D, K = e.D, e.K
        arms = {
            "score": lambda: eager.score(vals),
            "graph": lambda: graph.score(vals),
            "pack": lambda: ops.util_pack(vals, e.kind, e.slot, e.mean, e.sd, e.train),
            "gram": lambda: ops.util_gram(e.train, n, e.M, e.part),
            "factor": lambda: ops.util_factor(e.M, e.Lt, e.X, e.Minv),
            "step": lambda: ops.util_step(e.train, n, e.V, e.W, e.Minv, e.G, e.loss, e.part, e.lossp, 0.5),
            "grad": lambda: ops.util_grad(e.train, n, e.W, e.G, e.loss, e.part, e.lossp),
            "predict": lambda: ops.util_predict(e.test, e.n_test, e.train.counts, e.W, e.conf, e.G, e.loss, e.real,
                                                e.scores),
        }
        for fn in arms.values():          # warm-up: code objects, the graph capture
            fn()
            fn()
        times = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, fn in arms.items():
                times[k].append(_timed(fn, dev))
        got = eager.score(vals)
        print("hip arms done", {k: statistics.median(v) for k, v in times.items()}, flush=True)
        short = DeviceUtility(train, test, meta, vocabs, dev, ops=ops, iters=args.torch_iters, max_rows=n)
        slow = DeviceUtility(train, test, meta, vocabs, dev, ops=TorchOps(), iters=args.torch_iters, max_rows=n)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ref_scores = slow.score(vals)
        torch.cuda.synchronize(dev)
        torch_s = time.perf_counter() - t0
        err = float((short.score(vals).weights() - ref_scores.weights()).abs().max())
        hip_short_ms = _timed(lambda: short.score(vals), dev)
        res = {"rows": n, "train_rows": len(train), "test_rows": len(test), "columns": e.n_cols, "n_cont": e.n_cont,
               "n_cat": e.n_cat, "D": D, "K": K, "iters": iters, "row_groups_step": ops.util_groups(n, D * K),
               "row_groups_gram": ops.util_groups(n, D * D), "device": torch.cuda.get_device_name(0),
               "construct_s": construct_s, "hip_vs_torch_W_max_abs_err": err, "scores": got.floats(),
               "torch": {"wall_s": torch_s, "iters": args.torch_iters, "reps": 1, "hip_same_iters_ms": hip_short_ms}}
        for k, ms in times.items():
            res[k] = _summary(ms)
        sec = lambda k: res[k]["median_ms"] * 1e-3      # noqa: E731
        res["gram"]["flops"] = 2.0 * n * D * D / sec("gram")
        res["step"]["flops"] = (4.0 * n * D * K + 2.0 * D * D * K) / sec("step")
        res["step"]["share_of_fp64_peak"] = res["step"]["flops"] / FP64_PEAK
        res["torch_over_hip_same_iters"] = torch_s * 1e3 / hip_short_ms
    if not args.no_host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import utility_cases as uc
        from sklearn.linear_model import LogisticRegression
        from fed_tgan_amd.eval.utility import real_res
        kinds = list(e.kinds)
        tr_c, te_c = code_real_table(train, meta, vocabs), code_real_table(test, meta, vocabs)
        mean, sd = e.mean.cpu().numpy(), e.sd.cpu().numpy()
        def feats(table):        # rows whose target is no code carry no weight in the contract: left out here
            F, y = uc.features(table, kinds, e.card_list, K, mean, sd)
            return F[y < K], y[y < K]

        F, y = feats(fake)
        Ft, yt = feats(te_c)
        t0 = time.perf_counter()
        lr = LogisticRegression(C=1.0, class_weight="balanced", tol=args.lr_tol, max_iter=10000).fit(F, y)
        res["sklearn_lr"] = {"wall_s": time.perf_counter() - t0, "iterations": int(np.max(lr.n_iter_)), "tol": args.lr_tol,
                             "f1": _weighted_f1(yt, lr.predict(Ft), K)}
        Fr, yr = feats(tr_c)
        lr = LogisticRegression(C=1.0, class_weight="balanced", tol=args.lr_tol, max_iter=10000).fit(Fr, yr)
        res["sklearn_lr"]["f1_real"] = _weighted_f1(yt, lr.predict(Ft), K)
        t0 = time.perf_counter()
        import pandas as pd
        print("sklearn_lr", res["sklearn_lr"], flush=True)
        rr = real_res(pd.concat([real, fake_frame]), fake_frame, test, spec.target_column, spec.categorical_list,
                      verbose=False)
        res["sklearn_real_res"] = {"wall_s": time.perf_counter() - t0, "f1_lr": float(np.asarray(rr)[0][-1])}
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
