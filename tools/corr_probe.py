"""Cost of the correlation evaluator (Diff. Corr.) on one GPU, by arm and by launch (profiles/correlation_r8.md).

Two shapes.  ``intrusion``: n generated rows (an untrained generator of the 42-column schema: the values do not
change the work) against an m-row synthetic Intrusion real table.  ``wide``: a random coded n x 512 table, half of its
columns categorical with 2..31 values.  Arms, interleaved rep by rep, device time from HIP events around each call,
median and min .. max over the repetitions after a warm-up:

  * score / graph   eval/correlation.py DeviceCorrelation.score (csrc/kernels/correlation.hip), eager and as a
                    hipGraph replay
  * pack, moments, counts, matrix, diff   the pass's launches one by one, with the rates they imply: moments as the
                    2 n W n_cont flops of G = F^T Xc, counts as LDS atomics
  * torch           the same pass through TorchOps on the same device in the same process: what torch ops give today

    python tools/corr_probe.py [--shape intrusion|wide] [--rows 40000] [--real 40000] [--reps 10] [--torch-reps 2]
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


def _wide(n, m, cols, seed):
    g = np.random.default_rng(seed)
    kinds = [j % 2 for j in range(cols)]
    cards = [2 + (7 * s) % 30 for s in range(cols // 2)]
    meta = {"columns": [{"column_name": f"c{j}", "type": "categorical" if k else "continuous"}
                        for j, k in enumerate(kinds)], "non_negative_cols": []}

    def table(rows):
        hidden = g.random(rows)
        t = np.empty((rows, cols))
        s = 0
        for j, k in enumerate(kinds):
            if k:
                t[:, j] = np.minimum(np.floor((0.6 * hidden + 0.4 * g.random(rows)) * cards[s]), cards[s] - 1)
                s += 1
            else:
                t[:, j] = g.normal() * hidden + g.normal(size=rows)
        return t

    return meta, table(m), table(n), cards


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="intrusion", choices=["intrusion", "wide"])
    ap.add_argument("--rows", type=int, default=40000)
    ap.add_argument("--real", type=int, default=40000)
    ap.add_argument("--cols", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from fed_tgan_amd.eval.correlation import DeviceCorrelation
    from fed_tgan_amd.ops.hip import HipOps
    from fed_tgan_amd.ops.ref import TorchOps
    if not torch.cuda.is_available():
        raise SystemExit("corr_probe: needs a GPU (a CPU timing says nothing about the device)")
    dev = torch.device("cuda:0")
    n = args.rows
    if args.shape == "intrusion":
        from fed_tgan_amd.data.demo import small_table
        from fed_tgan_amd.data.synthetic import generate_intrusion
        from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
        from fed_tgan_amd.models.samplers import CondTables
        _, _, _, meta, vocabs, _, tr, X = small_table()
        eng = CTGANEngine(tr.layout, EngineConfig(batch_size=500), dev, backend="hip", seed=1)
        eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
        ops, real, kw = eng.ops, generate_intrusion(args.real, 7), {}
        vals = eng.generate_decoded(n)
    else:
        meta, real, fake, cards = _wide(n, args.real, args.cols, 3)
        ops, vocabs, kw = HipOps(dev), [], {"cardinalities": cards}
        vals = torch.from_numpy(fake).to(dev)
    t0 = time.perf_counter()
    eager = DeviceCorrelation(real, meta, vocabs, dev, ops=ops, max_rows=n, **kw)
    torch.cuda.synchronize(dev)
    construct_s = time.perf_counter() - t0
    graph = DeviceCorrelation(real, meta, vocabs, dev, ops=ops, max_rows=n, graph=True, **kw)
    slow = DeviceCorrelation(real, meta, vocabs, dev, ops=TorchOps(), max_rows=n, baseline=False, **kw)
    e = eager
    arms = {
        "score": lambda: eager.score(vals),
        "graph": lambda: graph.score(vals),
        "pack": lambda: ops.corr_pack(vals, e.kind, e.slot, e.card, e.cont, e.cat_t, e.mean, e.part),
        "moments": lambda: ops.corr_moments(e.cont, e.cat_t, n, e.mean, e.card, e.offs, e.G, e.part),
        "counts": lambda: ops.corr_counts(e.cat_t, n, e.pairs_t, e.poff, e.counts, e.lds_bins),
        "matrix": lambda: ops.corr_matrix(e.G, e.counts, e.poff, e.kind, e.slot, e.card, e.offs, n, e.A),
        "diff": lambda: ops.corr_diff(e.A_real, e.A, e.scores),
    }
    torch_pass = lambda: slow.score(vals)      # noqa: E731
    for fn in arms.values():          # warm-up: code objects, the graph capture
        fn()
        fn()
    ref_scores = torch_pass()
    torch.cuda.synchronize(dev)
    got = eager.score(vals)
    err = float((got.matrix() - ref_scores.matrix()).abs().max())
    times = {k: [] for k in arms}
    times["torch"] = []
    for rep in range(args.reps):
        for k, fn in arms.items():
            times[k].append(_timed(fn, dev))
        if rep < args.torch_reps:
            times["torch"].append(_timed(torch_pass, dev))
    res = {"shape": args.shape, "rows": n, "real_rows": args.real, "columns": e.n_cols, "n_cont": e.n_cont,
           "n_cat": e.n_cat, "W": e.W, "pairs": int(e.pairs_t.shape[0]), "tables_bytes": e.scratch_bytes,
           "global_pairs": len(e.global_pairs), "row_groups": ops.corr_groups(n, e.W, e.n_cont),
           "device": torch.cuda.get_device_name(0), "construct_s": construct_s,
           "hip_vs_torch_A_max_abs_err": err, "scores": got.floats()}
    for k, ms in times.items():
        res[k] = _summary(ms)
    sec = lambda k: res[k]["median_ms"] * 1e-3      # noqa: E731
    if e.n_cont:
        res["moments"]["flops"] = 2.0 * n * e.W * e.n_cont / sec("moments")
        res["moments"]["share_of_fp64_peak"] = res["moments"]["flops"] / FP64_PEAK
    if e.n_cat:
        res["counts"]["lds_atomics_per_s"] = float(n) * int(e.pairs_t.shape[0]) / sec("counts")
    res["torch_over_hip_graph"] = res["torch"]["median_ms"] / res["graph"]["median_ms"]
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
