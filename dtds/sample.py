"""``python -m dtds.sample`` -- generate rows from a trained federated generator.

    python -m dtds.sample -model models/Intrusion_generator.pt -n 40000 -out Intrusion_synthetic.csv

The federator writes ``models/{name}_generator.pt`` after the last round (see
:mod:`fed_tgan_amd.models.generator_io`); the reference only had an unused ``save_model``
(`Server/dtds/distributed.py:560-563`).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m dtds.sample")
    p.add_argument("-model", required=True, help="models/{name}_generator.pt written by the federator")
    p.add_argument("-n", type=int, default=40000, help="rows to generate")
    p.add_argument("-out", default=None, help="CSV path (default {name}_synthetic.csv)")
    p.add_argument("-backend", default="auto", choices=["auto", "hip", "torch"])
    p.add_argument("-seed", type=int, default=0)
    p.add_argument("-where", action="append", default=[], metavar="COL=VALUE",
                   help="only rows whose categorical column COL is VALUE (repeatable)")
    p.add_argument("-where_json", default=None,
                   help="the same as JSON; one column may map values to weights, e.g. "
                        "'{\"class\": {\"back.\": 1, \"satan.\": 1}, \"protocol_type\": \"tcp\"}' (-n rows split by weight); "
                        "a list of values means any of them, {\"min\": a, \"max\": b} a range on a continuous column")
    p.add_argument("-where_range", action="append", default=[], metavar="COL=LO:HI",
                   help="only rows whose continuous column COL lies in [LO, HI], in the units the CSV prints "
                        "(repeatable; either side may be empty for an open bound)")
    p.add_argument("-max_passes", type=int, default=64, help="generation passes a conditional request may take")
    p.add_argument("-min_dcr", type=float, default=None, metavar="T",
                   help="privacy guard: write only rows farther than T from every real record, in the metric of "
                        "-privacy_against (0 keeps out exact copies); still exactly -n rows")
    p.add_argument("-guard_against", default=None, metavar="REAL.csv",
                   help="the real table of -min_dcr (default: the table of -privacy_against)")
    p.add_argument("-known", default=None, metavar="PARTIAL.csv",
                   help="complete a partial table: a CSV with (some of) the model's columns whose blank cells are to be "
                        "filled; the output has its rows, in its order, with the known cells kept and the others taken "
                        "from the closest of -known_tries generated candidates (-n is ignored)")
    p.add_argument("-known_tries", type=int, default=64, help="candidates generated per row of -known (1..1024)")
    p.add_argument("-known_retries", type=int, default=2,
                   help="further rounds of candidates for rows of -known that still miss a known category")
    p.add_argument("-known_tol", type=float, default=None, metavar="T",
                   help="also retry rows of -known whose known numeric cells lie farther than T from the candidate")
    p.add_argument("-score_against", default=None, metavar="REAL.csv",
                   help="also print Avg_JSD / Avg_WD of the generated rows against this table, scored on the device")
    p.add_argument("-privacy_against", default=None, metavar="REAL.csv",
                   help="also print one JSON line with DCR / NNDR of the generated rows against this table (5th "
                        "percentiles, minimum, share of exact copies, and the real table's own baseline)")
    p.add_argument("-corr_against", default=None, metavar="REAL.csv",
                   help="also print one JSON line with Diff. Corr. of the generated rows against this table (the "
                        "distance between the two tables' association matrices, its mean and maximum per column "
                        "pair, and the real table's own even / odd row baseline)")
    p.add_argument("-fidelity_against", default=None, metavar="REAL.csv",
                   help="also print one JSON line, after all other output, with precision / recall / density / "
                        "coverage of the generated rows against this table (k-nearest-neighbour manifold metrics) and "
                        "the real table's own even / odd row baseline")
    p.add_argument("-fidelity_k", type=int, default=5, help="the k of -fidelity_against (1..8)")
    p.add_argument("-utility_against", default=None, metavar="REAL.csv",
                   help="also print one JSON line with the ML utility of the generated rows: weighted F1 and accuracy "
                        "on held-out real rows of a logistic regression fitted on them on the device, the same for "
                        "the real training rows, and the gaps (real - generated)")
    p.add_argument("-utility_test", default=None, metavar="TEST.csv",
                   help="the held-out real rows of -utility_against (default: its rows with index %% 5 == 4)")
    p.add_argument("-utility_iters", type=int, default=200, help="solver iterations of -utility_against")
    p.add_argument("-utility_models", default="lr", metavar="lr,dt,rf,mlp",
                   help="the classifiers of -utility_against: lr (logistic regression), dt (histogram decision tree), "
                        "rf (random forest), mlp (one hidden layer); the trees' and the network's scores join the same "
                        "JSON line as dt_* / rf_* / mlp_* keys")
    p.add_argument("-utility_trees", type=int, default=100, help="trees of the random forest of -utility_models")
    p.add_argument("-utility_depth", type=int, default=12, help="depth limit of the trees of -utility_models")
    p.add_argument("-utility_hidden", type=int, default=100, help="hidden units of the mlp of -utility_models")
    p.add_argument("-utility_steps", type=int, default=1000, help="Adam steps of the mlp of -utility_models")
    p.add_argument("-utility_batch", type=int, default=512, help="rows per batch of the mlp of -utility_models")
    args = p.parse_args(argv)
    if (args.utility_test or args.utility_iters != 200) and not args.utility_against:
        p.error("-utility_test / -utility_iters need -utility_against")
    utility_models = tuple(m for m in args.utility_models.split(",") if m)
    if not utility_models or set(utility_models) - {"lr", "dt", "rf", "mlp"}:
        p.error("-utility_models is a comma-separated subset of lr,dt,rf,mlp")
    if (utility_models != ("lr",) or args.utility_trees != 100 or args.utility_depth != 12) and not args.utility_against:
        p.error("-utility_models / -utility_trees / -utility_depth need -utility_against")
    if (args.utility_hidden != 100 or args.utility_steps != 1000 or args.utility_batch != 512) and \
            not args.utility_against:
        p.error("-utility_hidden / -utility_steps / -utility_batch need -utility_against")
    if args.fidelity_k != 5 and not args.fidelity_against:
        p.error("-fidelity_k needs -fidelity_against")
    if not 1 <= args.fidelity_k <= 8:
        p.error("-fidelity_k is 1..8")
    guard_real = args.guard_against or args.privacy_against
    if args.min_dcr is not None and guard_real is None:
        p.error("-min_dcr needs a real table: -guard_against or -privacy_against")
    if args.min_dcr is not None and not (args.min_dcr >= 0 and args.min_dcr != float("inf")):
        p.error("-min_dcr is a finite number >= 0")
    if args.guard_against and args.min_dcr is None:
        p.error("-guard_against needs -min_dcr")
    if args.known is not None:
        clash = [f for f, v in (("-where", args.where), ("-where_json", args.where_json),
                                ("-where_range", args.where_range), ("-min_dcr", args.min_dcr is not None),
                                ("-guard_against", args.guard_against), ("-score_against", args.score_against),
                                ("-privacy_against", args.privacy_against), ("-corr_against", args.corr_against),
                                ("-fidelity_against", args.fidelity_against),
                                ("-utility_against", args.utility_against)) if v]
        if clash:
            p.error(f"-known does not combine with {', '.join(clash)}")
        if not 1 <= args.known_tries <= 1024:
            p.error("-known_tries is 1..1024")
        if args.known_retries < 0:
            p.error("-known_retries is >= 0")
        if args.known_tol is not None and not args.known_tol >= 0:
            p.error("-known_tol is a number >= 0")
    elif args.known_tries != 64 or args.known_retries != 2 or args.known_tol is not None:
        p.error("-known_tries / -known_retries / -known_tol need -known")
    import torch
    from fed_tgan_amd.models.conditional import parse_where
    from fed_tgan_amd.models.generator_io import load_generator
    try:
        where = parse_where(args.where, args.where_json, args.where_range)
    except ValueError as e:
        p.error(str(e))
    dev = torch.device("cuda", 0) if (torch.cuda.is_available() and args.backend != "torch") else torch.device("cpu")
    gen = load_generator(args.model, dev, backend=args.backend, seed=args.seed)
    out = args.out or f"{gen.name}_synthetic.csv"
    t0 = time.time()
    scores = privacy = corr = utility = fidelity = None
    if args.known is not None:
        try:
            gen.write_csv(out, known=args.known, tries=args.known_tries, retries=args.known_retries,
                          tol=args.known_tol)
        except ValueError as e:
            p.error(str(e))
        lk = gen.engine.last_known
        print(f"{lk['rows']} rows -> {out} ({time.time() - t0:.3f} s, {gen.engine.ops.name} on {dev}, completed from "
              f"{args.known}: {lk['sweeps']} sweeps, {lk['generated']} candidates generated, "
              f"{100.0 * lk['exact_categorical']:.1f} % of rows with every known category matched, "
              f"d_p95 {lk['d_p95']:.4g})", flush=True)
        return out
    if args.score_against or args.privacy_against or args.corr_against or args.utility_against or \
            args.fidelity_against:
        scores, privacy, corr, utility, *more = gen.write_csv_all(
            out, args.n, score_real=args.score_against, privacy_real=args.privacy_against,
            corr_real=args.corr_against, where=where or None, max_passes=args.max_passes,
            utility_real=args.utility_against, utility_test=args.utility_test, utility_iters=args.utility_iters,
            utility_models=utility_models, utility_trees=args.utility_trees, utility_depth=args.utility_depth,
            utility_hidden=args.utility_hidden, utility_steps=args.utility_steps, utility_batch=args.utility_batch,
            min_dcr=args.min_dcr, guard_real=guard_real if args.min_dcr is not None else None,
            fidelity_real=args.fidelity_against, fidelity_k=args.fidelity_k)
        fidelity = more[0] if more else None
    elif args.min_dcr is not None:
        gen.write_csv(out, args.n, where=where or None, max_passes=args.max_passes, min_dcr=args.min_dcr,
                      guard_real=guard_real)
    else:
        gen.write_csv(out, args.n, where=where or None, max_passes=args.max_passes)
    cond = ""
    if where:
        lc = gen.engine.last_conditional
        cond = f", {lc['passes']} passes, {lc['kept']} of {lc['generated']} generated rows accepted"
        for pr in lc.get("predicates") or ():
            cond += (f", {pr['predicate']} rejected {100.0 * pr['rejected'] / max(pr['tested'], 1):.1f} % of "
                     f"{pr['tested']} rows")
    if args.min_dcr is not None:
        lg = gen.engine.last_guard
        cond += (f", guard min_dcr {args.min_dcr!r}: {lg['passes']} passes, {lg['rejected']} of {lg['generated']} "
                 "generated rows rejected")
    print(f"{args.n} rows -> {out} ({time.time() - t0:.3f} s, {gen.engine.ops.name} on {dev}{cond})", flush=True)
    if scores is not None:
        print(f"Avg_JSD {scores[0]!r} Avg_WD {scores[1]!r} (against {args.score_against})", flush=True)
    if privacy is not None:
        print(json.dumps(privacy), flush=True)
    if corr is not None:
        print(json.dumps(corr), flush=True)
    if utility is not None:
        print(json.dumps(utility), flush=True)
    if fidelity is not None:
        print(json.dumps(dict(fidelity, k=args.fidelity_k)), flush=True)
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
