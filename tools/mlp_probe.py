"""Cost and quality of the on-device MLP-utility evaluator (TSTR one-hidden-layer network) on one GPU, by arm and by
launch (profiles/mlp_r11.md).

The table: n rows of the synthetic 42-column Intrusion schema as the "generated" table (a fresh draw of the same
generator of rows: the fit is a meaningful one), an m-row draw as the real table, split by index % 5 == 4 into
training and held-out rows.  Arms, interleaved rep by rep, device time from HIP events around each call, median and
min .. max over the repetitions after a warm-up:

  * score / graph   eval/mlp_device.py DeviceMLP.score (csrc/kernels/mlp.hip), eager and as a hipGraph replay: pack,
                    ``steps`` steps, the loss, predict
  * pack, step, loss, predict   the pass's ops one by one; the step's two launches apart, from the profiler's kernel
                    records of ``--trace-steps`` steps
  * torch           the same pass through TorchOps on the same device in the same process, with ``--torch-steps``
                    steps only (wall time, one repetition)

and, on the host, for scale: sklearn's MLPClassifier(random_state=69) on the same feature matrix (its F1 on the
held-out rows against the evaluator's) as wall time.  ``--csv PATH --host-only`` instead fits the defaults through
TorchOps on the CPU on a real CSV of the Intrusion schema (rows with index % 5 == 4 held out) next to sklearn's.

    python tools/mlp_probe.py [--rows 40000] [--real 40000] [--steps 1000] [--reps 5] [--no-host | --host-only]
                              [--csv data/raw/Intrusion_test.csv]
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


def _scores(y, pred, K):
    conf = np.zeros((K, K), dtype=np.int64)
    np.add.at(conf, (y, pred), 1)
    rs, cs, tp = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
    den = rs + cs
    f = np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)
    return float((rs * f).sum() / max(conf.sum(), 1)), float(tp.sum() / max(conf.sum(), 1))


def _kernel_shares(step, n_steps, dev):
    """device time per kernel name over n_steps steps, from the profiler's kernel records"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize(dev)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(n_steps):
            step()
        torch.cuda.synchronize(dev)
    out = {}
    for ev in prof.key_averages():
        if "mlp_" in ev.key:
            name = "forward" if "mlp_forward" in ev.key else "grad_adam" if "mlp_grad_adam" in ev.key else ev.key
            total = getattr(ev, "device_time_total", None)
            if total is None:
                total = ev.cuda_time_total
            out[name] = {"us_per_step": total / n_steps, "calls": ev.count}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=40000)
    ap.add_argument("--real", type=int, default=40000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--hidden", type=int, default=100)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=50)
    ap.add_argument("--trace-steps", type=int, default=50)
    ap.add_argument("--no-host", action="store_true", help="skip the sklearn arm")
    ap.add_argument("--host-only", action="store_true", help="only the CPU arms (needs no GPU)")
    ap.add_argument("--csv", default=None, help="a real table of the Intrusion schema instead of the synthetic draws")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from fed_tgan_amd.data.demo import small_table
    from fed_tgan_amd.data.synthetic import generate_intrusion
    from fed_tgan_amd.eval.mlp_device import DeviceMLP
    from fed_tgan_amd.eval.privacy import code_real_table
    from fed_tgan_amd.ops.ref import TorchOps
    if not args.host_only and not torch.cuda.is_available():
        raise SystemExit("mlp_probe: needs a GPU (a CPU timing says nothing about the device)")
    dev = torch.device("cpu" if args.host_only else "cuda:0")
    n, steps = args.rows, args.steps
    kw = dict(hidden=args.hidden, batch=args.batch)
    if args.csv:
        import pandas as pd
        from fed_tgan_amd.data.schema import intrusion_spec
        from fed_tgan_amd.data.table import TablePreprocessor
        from fed_tgan_amd.fed.stats import merge_categorical_metas
        spec, real = intrusion_spec(), pd.read_csv(args.csv)
        tp = TablePreprocessor(real, "Intrusion", spec.problem_type, spec.target_column, spec.categorical_list,
                               spec.nonnegative_list)
        meta, vocabs, _ = merge_categorical_metas([tp.local_meta()])
    else:
        _, _, _, meta, vocabs, _, _, _ = small_table()
        real = generate_intrusion(args.real, 7)
    held = np.arange(len(real)) % 5 == 4
    train, test = real[~held].reset_index(drop=True), real[held].reset_index(drop=True)
    fake = code_real_table(train if args.csv else generate_intrusion(n, 9), meta, vocabs)
    n = len(fake)
    vals = torch.from_numpy(fake).to(dev)
    if args.host_only:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        t0 = time.perf_counter()
        e = DeviceMLP(train, test, meta, vocabs, dev, ops=TorchOps(), steps=steps, max_rows=n, **kw)
        got = e.score(vals).floats()
        res = {"rows": n, "train_rows": len(train), "test_rows": len(test), "D": e.D, "K": e.K, "host_only": True,
               "steps": steps, "classes_present": int((e.train.counts > 0).sum()), "scores": got,
               "torch_cpu_wall_s": time.perf_counter() - t0, "csv": args.csv}
    else:
        from fed_tgan_amd.ops.hip import HipOps
        ops = HipOps(dev)
        t0 = time.perf_counter()
        eager = DeviceMLP(train, test, meta, vocabs, dev, ops=ops, steps=steps, max_rows=n, **kw)
        torch.cuda.synchronize(dev)
        construct_s = time.perf_counter() - t0
        graph = DeviceMLP(train, test, meta, vocabs, dev, ops=ops, steps=steps, max_rows=n, graph=True, **kw)
        e = eager
        nb = (n + e.batch - 1) // e.batch

        def step():
            ops.mlp_step(e.train, n, 1 % nb, nb, e.theta, e.m, e.v, e.h, e.dz, e.dh, e.cnt, e.hidden, e.alpha, 1e-3)

        arms = {
            "score": lambda: eager.score(vals),
            "graph": lambda: graph.score(vals),
            "pack": lambda: ops.util_pack(vals, e.kind, e.slot, e.mean, e.sd, e.train),
            "step": step,
            "loss": lambda: ops.mlp_loss(e.train, n, e.theta, e.hidden, e.alpha, e.loss),
            "predict": lambda: ops.mlp_predict(e.test, e.n_test, e.train.counts, e.theta, e.hidden, e.conf, e.loss,
                                               e.real, e.scores),
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
        try:
            launches = _kernel_shares(step, args.trace_steps, dev)
        except Exception as err:          # a torch build without kernel records: the arms above still stand
            launches = {"unavailable": repr(err)}
        short = DeviceMLP(train, test, meta, vocabs, dev, ops=ops, steps=args.torch_steps, max_rows=n, **kw)
        slow = DeviceMLP(train, test, meta, vocabs, dev, ops=TorchOps(), steps=args.torch_steps, max_rows=n, **kw)
        slow.score(vals)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ref_scores = slow.score(vals)
        torch.cuda.synchronize(dev)
        torch_s = time.perf_counter() - t0
        err = max(float((a - b).abs().max()) for a, b in zip(short.score(vals).weights(), ref_scores.weights()))
        hip_short_ms = _timed(lambda: short.score(vals), dev)
        res = {"rows": n, "train_rows": len(train), "test_rows": len(test), "columns": e.n_cols, "n_cont": e.n_cont,
               "n_cat": e.n_cat, "D": e.D, "K": e.K, "hidden": e.hidden, "batch": e.batch, "steps": steps,
               "device": torch.cuda.get_device_name(0), "construct_s": construct_s,
               "hip_vs_torch_theta_max_abs_err": err, "scores": got.floats(), "step_launches": launches,
               "torch": {"wall_s": torch_s, "steps": args.torch_steps, "reps": 1, "hip_same_steps_ms": hip_short_ms}}
        for k, ms in times.items():
            res[k] = _summary(ms)
        res["score"]["ms_per_step"] = (res["score"]["median_ms"] - res["pack"]["median_ms"] - res["loss"]["median_ms"]
                                       - res["predict"]["median_ms"]) / max(steps, 1)
        res["torch_over_hip_same_steps"] = torch_s * 1e3 / hip_short_ms
    if not args.no_host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import utility_cases as uc
        from sklearn.neural_network import MLPClassifier
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        K, mean, sd = e.K, e.mean.cpu().numpy(), e.sd.cpu().numpy()

        def feats(table):        # rows whose target is no code carry no weight in the contract: left out here
            F, y = uc.features(table, list(e.kinds), e.card_list, K, mean, sd)
            return F[y < K, :-1], y[y < K]          # (sklearn has its own intercept)

        Ft, yt = feats(code_real_table(test, meta, vocabs))
        res["sklearn_mlp"] = {}
        for side, table in (("fake", fake), ("real", code_real_table(train, meta, vocabs))):
            F, y = feats(table)
            t0 = time.perf_counter()
            clf = MLPClassifier(random_state=69).fit(F, y)
            wall = time.perf_counter() - t0
            pred = clf.classes_[np.argmax(clf.predict_proba(Ft), axis=1)]
            f1, acc = _scores(yt, pred, K)
            res["sklearn_mlp"][side] = {"wall_s": wall, "epochs": int(clf.n_iter_), "f1": f1, "acc": acc}
            print("sklearn_mlp", side, res["sklearn_mlp"][side], flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
