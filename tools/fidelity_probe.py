"""Cost of the fidelity evaluator on one GPU (profiles/fidelity_r13.md).

--rows generated rows (an untrained generator of the 42-column Intrusion schema) against a --real row synthetic
Intrusion table, k = --k.  Arms, alternated rep by rep in one process after a warm-up of every arm, device time from
HIP events, median and min .. max:

  * top2            HipOps.nn_top2 on the same packed buffers (the privacy evaluator's search, the yardstick)
  * topk_self       HipOps.nn_topk, the generated rows against themselves (ff)
  * ball_fake       HipOps.nn_ball, generated queries against the real balls (cntA)
  * ball_real       HipOps.nn_ball, real queries against the generated balls (cntB, dminB)
  * reduce          HipOps.prdc_reduce
  * score           DeviceFidelity.score, eager
  * score_graph     DeviceFidelity.score as a hipGraph replay
  * score_torch     DeviceFidelity.score on the reference ops (ops/ref.py) on the same GPU, --torch_reps times

    python tools/fidelity_probe.py [--rows 40000] [--real 40000] [--k 5] [--reps 10] [--torch_reps 3] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

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
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch_reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from fed_tgan_amd.data.demo import small_table
    from fed_tgan_amd.data.synthetic import generate_intrusion
    from fed_tgan_amd.eval.fidelity import DeviceFidelity
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.samplers import CondTables
    from fed_tgan_amd.ops.ref import TorchOps
    if not torch.cuda.is_available():
        raise SystemExit("fidelity_probe: needs a GPU (a CPU timing says nothing about the device)")
    dev = torch.device("cuda:0")
    _, _, _, meta, vocabs, _, tr, X = small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=500), dev, backend="hip", seed=1)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    real = generate_intrusion(args.real, 7)
    ops, n, m, k = eng.ops, args.rows, args.real, args.k
    ev = DeviceFidelity(real, meta, vocabs, dev, ops=ops, k=k, max_rows=n)
    evg = DeviceFidelity(real, meta, vocabs, dev, ops=ops, k=k, max_rows=n, graph=True, baseline=False)
    evt = DeviceFidelity(real, meta, vocabs, dev, ops=TorchOps(), k=k, max_rows=n, baseline=False)
    vals = eng.generate_decoded(n).clone()
    ops.nn_pack(vals, ev.kind, ev.slot, ev.lo, ev.scale, ev.q_cont, ev.q_cat)
    q_cont, q_cat = ev.q_cont[:n], ev.q_cat[:n]
    f64 = dict(dtype=torch.float64, device=dev)
    d1, d2 = torch.zeros(n, **f64), torch.zeros(n, **f64)
    i1 = torch.zeros(n, dtype=torch.int32, device=dev)
    top2_scratch = torch.zeros(ops.nn_scratch(n, m), **f64)
    arms = {
        "top2": lambda: ops.nn_top2(q_cont, q_cat, ev.r_cont, ev.r_cat, False, d1, d2, i1, top2_scratch),
        "topk_self": lambda: ops.nn_topk(q_cont, q_cat, q_cont, q_cat, True, k, ev.ff, ev.scratch),
        "ball_fake": lambda: ops.nn_ball(q_cont, q_cat, ev.r_cont, ev.r_cat, ev.rr, ev.cnt_a, ev.dmin_a, ev.scratch),
        "ball_real": lambda: ops.nn_ball(ev.r_cont, ev.r_cat, q_cont, q_cat, ev.ff, ev.cnt_b, ev.dmin_b, ev.scratch),
        "reduce": lambda: ops.prdc_reduce(ev.cnt_a, ev.cnt_b, ev.dmin_b, ev.rr, n, m, k, ev.scores),
        "score": lambda: ev.score(vals),
        "score_graph": lambda: evg.score(vals),
    }
    res = {"rows": n, "real_rows": m, "k": k, "n_cont": ev.n_cont, "n_cat": ev.n_cat,
           "device": torch.cuda.get_device_name(0)}
    for fn in arms.values():            # warm-up of every arm (the first replay captures the graph)
        fn()
        fn()
    res["scores"] = ev.score(vals).floats()
    res["scores_graph_equal"] = bool(torch.equal(evg.score(vals).buf[:4], ev.score(vals).buf[:4]))
    # the nearest-neighbour distance of the ball pass is the top-2 search's d1 within rounding
    ops.nn_ball(q_cont, q_cat, ev.r_cont, ev.r_cat, ev.rr, ev.cnt_a, ev.dmin_a, ev.scratch)
    res["dmin_vs_top2_d1_max_abs"] = float((ev.dmin_a[:n] - d1).abs().max())
    times = {key: [] for key in arms}
    for _ in range(args.reps):
        for key, fn in arms.items():
            times[key].append(_timed(fn, dev))
    for key, ms in times.items():
        res[key] = _summary(ms)
    if args.torch_reps > 0:
        evt.score(vals)
        res["scores_torch"] = evt.score(vals).floats()
        res["score_torch"] = _summary([_timed(lambda: evt.score(vals), dev) for _ in range(args.torch_reps)])
        res["torch_over_hip"] = res["score_torch"]["median_ms"] / res["score"]["median_ms"]
    for key in ("topk_self", "ball_fake", "ball_real", "score", "score_graph"):
        res[key + "_over_top2"] = res[key]["median_ms"] / res["top2"]["median_ms"]
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    eng.release()


if __name__ == "__main__":
    main()
