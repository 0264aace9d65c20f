"""Cost of the privacy guard on one GPU (profiles/guard_r12.md).

(1) The radius test against the top-2 search on the same packed buffers: --rows generated rows (an untrained generator
of the 42-column Intrusion schema) against a --real row synthetic Intrusion table.  Arms, alternated rep by rep in
one process, device time from HIP events, median and min .. max after a warm-up of every arm:

  * top2            HipOps.nn_top2 (the privacy evaluator's search, the yardstick)
  * within T=0      HipOps.nn_within at t2 = 0
  * within p5       ... at T = the real table's own dcr_rr_p5
  * within inf      ... at t2 = +inf (every query has its hit in the first tile)

(2) End to end: LoadedGenerator.write_csv(n, min_dcr=0) against the unguarded call, alternated, wall time; the
guarded pass replayed alone and its search (nn_pack + nn_within) alone, device time.

    python tools/guard_probe.py [--rows 65536] [--real 40000] [--n 40000] [--reps 10] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

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


def _wall(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def _summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--real", type=int, default=40000)
    ap.add_argument("--n", type=int, default=40000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from fed_tgan_amd.data.demo import small_table
    from fed_tgan_amd.data.synthetic import generate_intrusion
    from fed_tgan_amd.eval.privacy import DevicePrivacy
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.generator_io import LoadedGenerator
    from fed_tgan_amd.models.samplers import CondTables
    if not torch.cuda.is_available():
        raise SystemExit("guard_probe: needs a GPU (a CPU timing says nothing about the device)")
    dev = torch.device("cuda:0")
    _, _, _, meta, vocabs, _, tr, X = small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=500), dev, backend="hip", seed=1)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    real = generate_intrusion(args.real, 7)
    ops, nq = eng.ops, args.rows
    ev = DevicePrivacy(real, meta, vocabs, dev, ops=ops, max_rows=nq)
    base = ev.scores.tolist()
    vals = eng.generate_decoded(nq)
    ops.nn_pack(vals, ev.kind, ev.slot, ev.lo, ev.scale, ev.q_cont, ev.q_cat)
    q_cont, q_cat = ev.q_cont[:nq], ev.q_cat[:nq]
    near = torch.zeros(nq, dtype=torch.int32, device=dev)
    t2s = {"within_T0": 0.0, "within_p5": float(base[4]) ** 2, "within_inf": float("inf")}
    t2d = {k: torch.tensor([v], dtype=torch.float64, device=dev) for k, v in t2s.items()}
    arms = {"top2": lambda: ops.nn_top2(q_cont, q_cat, ev.r_cont, ev.r_cat, False, ev.d1, ev.d2, ev.i1, ev.scratch)}
    for k in t2s:
        arms[k] = (lambda t: lambda: ops.nn_within(q_cont, q_cat, ev.r_cont, ev.r_cat, t, near, ev.scratch))(t2d[k])
    res = {"rows": nq, "real_rows": args.real, "n_cont": ev.n_cont, "n_cat": ev.n_cat,
           "device": torch.cuda.get_device_name(0), "dcr_rr_p5": base[4], "flagged": {}, "agrees_with_top2": {}}
    for k, fn in arms.items():          # warm-up of every arm, and the two searches agree on every row
        fn()
        fn()
        if k != "top2":
            res["flagged"][k] = int((near >= 0).sum())
            res["agrees_with_top2"][k] = bool(torch.equal(near >= 0, ev.d1[:nq] <= t2d[k]))
    times = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, fn in arms.items():
            times[k].append(_timed(fn, dev))
    for k, ms in times.items():
        res[k] = _summary(ms)

    # (2) end to end
    gen = LoadedGenerator("Intrusion", eng, tr, meta, vocabs)
    n = args.n
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "s.csv")
        calls = {"write_csv": lambda: gen.write_csv(path, n),
                 "write_csv_guarded": lambda: gen.write_csv(path, n, min_dcr=0.0, guard_real=real)}
        for fn in calls.values():
            fn()
            fn()
        wall = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                wall[k].append(_wall(fn, dev))
    for k, ms in wall.items():
        res[k] = _summary(ms)
    lg = eng.last_guard
    res["guard"] = dict(lg, rejected_share=lg["rejected"] / max(lg["generated"], 1))
    (key, ent), = eng._guard_ent.items()
    m, guard = key[0], ent["guard"]
    plain = eng._gen_graphs[n]
    parts = {"guarded_pass": ent["graph"].replay, "search": lambda: guard.launch(ent["out"], *ent["gbufs"]),
             "plain_pass": plain.graph.replay}
    ctr = ops.ctr.clone()
    for fn in parts.values():
        fn()
    dev_ms = {k: [] for k in parts}
    for _ in range(args.reps):
        for k, fn in parts.items():
            dev_ms[k].append(_timed(fn, dev))
    ops.ctr.copy_(ctr)
    for k, ms in dev_ms.items():
        res[k] = _summary(ms)
    res["pass_rows"] = m
    res["search_share_of_pass"] = res["search"]["median_ms"] / res["guarded_pass"]["median_ms"]
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    eng.release()


if __name__ == "__main__":
    main()
