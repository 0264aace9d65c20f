"""Cost of scoring a generated table (Avg_JSD / Avg_WD) on one GPU, by arm (profiles/similarity_r7.md).

The Intrusion shape: the shipped split's 8,078 training rows (tools/real_quality.py's 80 / 20 split, seed 2024) as
the real table, 42 columns; a one-round federation on them gives the generator, which then produces n rows.
Arms, interleaved rep by rep:

  * graph / eager   eval/device.py DeviceSimilarity.score (csrc/kernels/similarity.hip) as a hipGraph replay and as
                    eager launches; device time from HIP events around the call, and host wall time to the
                    synchronised result
  * torch           the torch-op formulation on the same device: the reference ops' table pass (bincount for the
                    counts), fed/stats.py wasserstein_1d_rows for W1 (it sorts the fake rows itself and takes whole
                    rows: tables in which a column has blank fields are not its domain, the time is the same) and
                    the reference JSD
  * stat_sim        eval/similarity.py on the written CSV, with and without read_csv (host wall time)

    python tools/similarity_bench.py [--sizes 40000 200000] [--reps 20] [--out-dir /tmp/simbench] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
DATA = os.path.join(ROOT, "data", "raw", "Intrusion_test.csv")


def _timed(fn, dev):
    """(device ms between two events around fn, host ms until the device is idle)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[40000, 200000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out-dir", default="/tmp/simbench")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from fed_tgan_amd.data.schema import intrusion_spec
    from fed_tgan_amd.eval.device import DeviceSimilarity
    from fed_tgan_amd.eval.similarity import stat_sim
    from fed_tgan_amd.fed.runtime import FedConfig, FedRuntime
    from fed_tgan_amd.fed.stats import wasserstein_1d_rows
    from fed_tgan_amd.models.generator_io import load_generator
    from fed_tgan_amd.ops.ref import TorchOps
    from fed_tgan_amd.parallel.comm import Comm
    if not torch.cuda.is_available():
        raise SystemExit("similarity_bench.py measures on a GPU; none found")
    dev = torch.device("cuda:0")
    spec = intrusion_spec()
    os.makedirs(args.out_dir, exist_ok=True)
    df = pd.read_csv(DATA)
    perm = np.random.default_rng(2024).permutation(len(df))
    train_path = os.path.join(args.out_dir, "train.csv")
    df.iloc[perm[:int(round(0.8 * len(df)))]].reset_index(drop=True).to_csv(train_path, index=False)
    real = pd.read_csv(train_path)
    cfg = FedConfig(spec=spec, epochs=1, datapath=train_path, n_sample=1000, out_dir=args.out_dir, backend="hip",
                    gmm_backend="torch", verbose=False)
    rt = FedRuntime(cfg, Comm(0, 1, [0], "gloo", device=dev), dev)
    rt.initialize()
    rt.fit()
    rt.close()
    gen = load_generator(os.path.join(args.out_dir, "models", f"{spec.name}_generator.pt"), dev, backend="hip")
    ref = TorchOps()
    results = []
    for n in args.sizes:
        vals = gen.device_table(n)
        torch.cuda.synchronize(dev)
        sims = {"graph": DeviceSimilarity(real, gen.meta, gen.vocabs, dev, ops=gen.engine.ops, max_rows=n, graph=True),
                "eager": DeviceSimilarity(real, gen.meta, gen.vocabs, dev, ops=gen.engine.ops, max_rows=n)}
        s0 = sims["eager"]
        lo, hi = s0.real_keys[:, :1], s0.real_keys.gather(1, (s0.n_real.long() - 1).clamp_min(0).view(-1, 1))
        scale = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
        real_scaled = (s0.real_keys - lo) / scale          # (every real column of the split parses fully)
        keys, valid = torch.empty_like(s0.keys), torch.empty_like(s0.valid)
        counts, out = torch.empty_like(s0.counts), torch.empty_like(s0.scores)

        def torch_arm():
            ref.sim_prepare(vals, s0.kind, s0.slot, s0.vocab, keys, valid, counts)
            wd = wasserstein_1d_rows(real_scaled, (keys[:, :n] - lo) / scale, u_sorted=True)
            ref.sim_jsd(s0.real_counts, counts, out[2:2 + s0.n_cat])
            return torch.stack([out[2:2 + s0.n_cat].mean(), wd.mean()])

        arms = {"graph": lambda: sims["graph"].score(vals).buf[:2], "eager": lambda: sims["eager"].score(vals).buf[:2],
                "torch": torch_arm}
        path = os.path.join(args.out_dir, f"fake_{n}.csv")
        gen._write_values(path, gen._to_host(vals))
        times = {k: [] for k in arms}
        values = {}
        for rep in range(args.reps + 2):                       # two warm-up reps (code objects, graph capture)
            for k, fn in arms.items():
                d, h, o = _timed(fn, dev)
                values[k] = [float(x) for x in o.cpu().tolist()]
                if rep >= 2:
                    times[k].append((d, h))
        cpu = {"read_csv": [], "stat_sim": []}
        for _ in range(3):
            t0 = time.perf_counter()
            fake = pd.read_csv(path)
            t1 = time.perf_counter()
            values["stat_sim"] = list(stat_sim(real, fake, spec.categorical_list))
            cpu["read_csv"].append((t1 - t0) * 1e3)
            cpu["stat_sim"].append((time.perf_counter() - t1) * 1e3)
        rec = {"rows": n, "real_rows": len(real), "columns": len(real.columns), "reps": args.reps, "scores": values,
               "launches_per_score": 7 + max(0, int(np.ceil(np.log2(max(1, -(-n // gen.engine.ops.SIM_SORT_TILE)))))),
               "cpu_ms": {k: {"median": statistics.median(v), "min": min(v)} for k, v in cpu.items()}}
        for k, v in times.items():
            dv, hv = [x[0] for x in v], [x[1] for x in v]
            rec[k] = {"device_ms": {"median": statistics.median(dv), "min": min(dv), "max": max(dv)},
                      "host_ms": {"median": statistics.median(hv), "min": min(hv), "max": max(hv)}}
        results.append(rec)
        print(json.dumps(rec), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
