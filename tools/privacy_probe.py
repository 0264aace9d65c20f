"""Cost of the privacy evaluator (DCR / NNDR) on one GPU, by arm (profiles/privacy_r7.md).

The Intrusion shape: n generated rows (an untrained generator of the 42-column schema: the values do not change the
work) against an m-row synthetic Intrusion real table.  Arms, interleaved rep by rep, device time from HIP events
around each call, median and min .. max over the repetitions after a warm-up:

  * score / graph   eval/privacy.py DevicePrivacy.score (csrc/kernels/privacy.hip), eager and as a hipGraph replay
  * top2            HipOps.nn_top2 alone, with the implied pair rate
  * torch top2      TorchOps.nn_top2 on the same device in the same process: what torch ops give today
  * host            the round trip: copy both packed tables to the host, one-hot the codes (weight 1 / sqrt 2, so
                    the squared Euclidean distance is the same d2) and scikit-learn's brute-force 2-NN on
                    --threads threads, at --host-rows queries

    python tools/privacy_probe.py [--rows 40000] [--real 40000] [--reps 10] [--torch-reps 3] [--json PATH]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=4000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from fed_tgan_amd.data.demo import small_table
    from fed_tgan_amd.data.synthetic import generate_intrusion
    from fed_tgan_amd.eval.privacy import DevicePrivacy
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.samplers import CondTables
    from fed_tgan_amd.ops.ref import TorchOps
    if not torch.cuda.is_available():
        raise SystemExit("privacy_probe: needs a GPU (a CPU timing says nothing about the device)")
    dev = torch.device("cuda:0")
    _, _, _, meta, vocabs, _, tr, X = small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=500), dev, backend="hip", seed=1)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    real = generate_intrusion(args.real, 7)
    n = args.rows
    vals = eng.generate_decoded(n)
    t0 = time.perf_counter()
    eager = DevicePrivacy(real, meta, vocabs, dev, ops=eng.ops, max_rows=n)
    torch.cuda.synchronize(dev)
    construct_s = time.perf_counter() - t0
    graph = DevicePrivacy(real, meta, vocabs, dev, ops=eng.ops, max_rows=n, graph=True)
    ref = TorchOps()
    q_cont, q_cat = eager.q_cont[:n], eager.q_cat[:n]
    t_d1, t_d2 = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    t_i1 = torch.zeros(n, dtype=torch.int32, device=dev)
    arms = {
        "score": lambda: eager.score(vals),
        "graph": lambda: graph.score(vals),
        "top2": lambda: eng.ops.nn_top2(q_cont, q_cat, eager.r_cont, eager.r_cat, False, eager.d1, eager.d2, eager.i1,
                                        eager.scratch),
    }
    torch_top2 = lambda: ref.nn_top2(q_cont, q_cat, eager.r_cont, eager.r_cat, False, t_d1, t_d2, t_i1)      # noqa: E731
    for fn in arms.values():          # warm-up: code objects, the graph capture
        fn()
        fn()
    torch_top2()
    torch.cuda.synchronize(dev)
    # the two formulations agree on this table (the tests' bound)
    err = ((eager.d1[:n] - t_d1).abs() / t_d1.clamp_min(1.0)).max().item()
    times = {k: [] for k in arms}
    times["torch_top2"] = []
    for rep in range(args.reps):
        for k, fn in arms.items():
            times[k].append(_timed(fn, dev))
        if rep < args.torch_reps:
            times["torch_top2"].append(_timed(torch_top2, dev))
    res = {"rows": n, "real_rows": args.real, "columns": len(meta["columns"]), "n_cont": eager.n_cont,
           "n_cat": eager.n_cat, "device": torch.cuda.get_device_name(0), "construct_s": construct_s,
           "hip_vs_torch_d1_max_rel_err": err, "scores": eager.score(vals).floats()}
    for k, ms in times.items():
        res[k] = _summary(ms)
    pairs = float(n) * float(args.real)
    res["top2"]["pairs_per_s"] = pairs / (res["top2"]["median_ms"] * 1e-3)
    res["torch_top2"]["pairs_per_s"] = pairs / (res["torch_top2"]["median_ms"] * 1e-3)
    res["torch_over_hip"] = res["torch_top2"]["median_ms"] / res["top2"]["median_ms"]

    # the round trip: device -> host copy, then scikit-learn's brute force on the host
    from sklearn.neighbors import NearestNeighbors
    hq = min(args.host_rows, n)
    t0 = time.perf_counter()
    host = [t.cpu().numpy() for t in (q_cont[:hq], q_cat[:hq], eager.r_cont, eager.r_cat)]
    copy_s = time.perf_counter() - t0
    width = int(max(host[1].max(), host[3].max())) + 1

    def embed(cont, cat):
        hot = np.zeros((cat.shape[0], cat.shape[1], width), dtype=np.float64)
        np.put_along_axis(hot, cat[:, :, None].astype(np.int64), np.sqrt(0.5), axis=2)
        return np.concatenate([cont, hot.reshape(cat.shape[0], -1)], axis=1)

    t0 = time.perf_counter()
    nn = NearestNeighbors(n_neighbors=2, algorithm="brute", n_jobs=args.threads).fit(embed(host[2], host[3]))
    dist, _ = nn.kneighbors(embed(host[0], host[1]))
    host_s = time.perf_counter() - t0
    res["host"] = {"query_rows": hq, "threads": args.threads, "copy_s": copy_s, "knn_s": host_s,
                   "pairs_per_s": float(hq) * args.real / host_s,
                   "dcr_max_abs_diff": float(np.abs(dist[:, 0] - eager.score(vals).rows()[0][:hq].cpu().numpy()).max())}
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
