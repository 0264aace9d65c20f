"""Conditional generation measured (profiles/cond_sample_r7.md):

(a) the cost of one conditional pass (sample_gen -> cond_request -> G -> sample_decode -> cond_partition) against the
    plain generation pass at the same row count, both as hipGraph replays, alternating;
(b) on a model trained for a few dozen epochs: rows kept per rows generated for requested ``class`` values, with the
    value in the conditional vector (generate_decoded_where) and by filtering plain generate_decoded output.

    python tools/cond_probe.py [--rows 40960] [--epochs 40 400] [--seeds 1 2] [--out FILE]

``--pred`` measures the range / set predicates instead (profiles/cond_pred_r14.md):

(c) one predicate-driven pass (sample_gen -> pred_request -> G -> sample_decode -> pred_mark -> cond_partition,
    ``serror_rate`` in [0.9, 1.0]) against the one-value conditional pass of (a) at the same row count, both as
    hipGraph replays with the generator wired to obey its condition, alternating;
(d) on a generator trained on ``--csv`` (the shipped Intrusion split): rows generated per row kept for that range when
    it drives (modes drawn by rows x Gaussian share) against the same range as a filter behind the unconditional
    sampler -- the same code with the driver table set to the span's plain counts.

    python tools/cond_probe.py --pred [--pred_rows 65536] [--csv data/raw/Intrusion_test.csv] [--epochs 300]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def replay_us(fn, dev, reps):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) / reps * 1e6


def wire(eng, tr, continuous):
    """The output layer copies the conditional vector onto the logits of its span (weight 60 beats the Gumbel noise):
    the categorical one-hots, with ``continuous`` the mode indicators too."""
    lay = tr.layout
    with torch.no_grad():
        W = eng.p["G.out.W"]
        W.zero_()
        eng.p["G.out.b"].zero_()
        for c, mt in enumerate(tr.meta):
            if continuous or mt["type"] != "continuous":
                for k in range(int(lay.cond_width[c])):
                    W[int(lay.cond_start[c]) + k, W.shape[1] - lay.n_opt + int(lay.cond_offset[c]) + k] = 60.0


def csv_table(path, dev):
    """(meta, vocabs, transformer, encoded matrix) of a CSV of the Intrusion schema, fitted on the device."""
    import numpy as np
    import pandas as pd
    from fed_tgan_amd.data.schema import intrusion_spec
    from fed_tgan_amd.data.table import TablePreprocessor
    from fed_tgan_amd.features.transformer import VGMTransformer
    from fed_tgan_amd.fed.stats import merge_categorical_metas
    spec, real = intrusion_spec(), pd.read_csv(path)
    tp = TablePreprocessor(real, "Intrusion", spec.problem_type, spec.target_column, spec.categorical_list,
                           spec.nonnegative_list)
    meta, vocabs, _ = merge_categorical_metas([tp.local_meta()])
    enc = tp.encode(vocabs)
    cat = tp.categorical_indices()
    tr = VGMTransformer().fit(enc, cat, (), seed=0, backend="torch", device=str(dev))
    tr.refit(enc, meta, vocabs, cat, (), tr.bank, tr.components)
    return meta, vocabs, tr, tr.transform(enc, np.random.default_rng(0))


def pred_probe(args, dev, say):
    from fed_tgan_amd.data.demo import small_table
    from fed_tgan_amd.models.conditional import build_request, driver_table, mode_tables
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.samplers import CondTables
    where = {"serror_rate": {"min": 0.9, "max": 1.0}}
    m = args.pred_rows

    # ---------------------------------------------------------------- (c) pass cost
    _, df, _, meta, vocabs, _, tr, X = small_table(args.table_rows, 0)
    names = [c["column_name"] for c in meta["columns"]]
    cond = CondTables.from_encoded(X, tr.layout)
    eng = CTGANEngine(tr.layout, EngineConfig(gen_chunk=max(m, 40960)), dev, backend="hip", seed=1)
    eng.set_training_data(X)
    eng.set_generation_tables(cond, tr)
    wire(eng, tr, continuous=True)
    common = str(df["class"].value_counts().index[0])
    one = build_request(tr, meta, vocabs, {"class": common}, m, dev)
    eng.generate_decoded_where(m, one, chunk=m)
    lc1 = dict(eng.last_conditional)
    rng = build_request(tr, meta, vocabs, where, m, dev, counts=cond.counts)
    eng.generate_decoded_where(m, rng, chunk=m)
    lc2 = dict(eng.last_conditional)
    e1 = eng._cond_ent[(m, 1, 0)]
    e2 = eng._cond_ent[(m, 1, 0) + eng._pred_shape(rng)]

    def replay(ent):
        def fn():               # the quota reopened before every replay: each pass writes every row it keeps
            ent["req"]["filled"].zero_()
            ent["graph"].replay()
        return fn
    say(f"(c) one pass of {m} rows of small_table({args.table_rows}, 0), hipGraph replays, {args.reps} per window, "
        f"alternating; wired output layer: class={common!r} keeps {lc1['kept']}/{lc1['generated']}, serror_rate in "
        f"[0.9, 1.0] keeps {lc2['kept']}/{lc2['generated']} (driver table {rng['drv_opt'].tolist()} / "
        f"{[round(x, 6) for x in rng['drv_cum'].tolist()]})")
    for rnd in range(4):
        a = replay_us(replay(e1), dev, args.reps)
        b = replay_us(replay(e2), dev, args.reps)
        say(f"    round {rnd}: one-value pass {a:7.1f} us   predicate-driven pass {b:7.1f} us   added {b - a:6.1f} us = "
            f"{100 * (b - a) / a:5.1f} %")
    eng.release()

    # ---------------------------------------------------------------- (d) generated rows per kept row, trained model
    meta, vocabs, tr, X = csv_table(args.csv, dev)
    names = [c["column_name"] for c in meta["columns"]]
    js = names.index("serror_rate")
    cond = CondTables.from_encoded(X, tr.layout)
    mu, sd = mode_tables(tr, js)
    say(f"(d) {args.csv}: {X.shape[0]} rows; serror_rate modes (mean, sd, rows): "
        f"{[(round(float(a), 4), round(float(b), 4), int(c)) for a, b, c in zip(mu, sd, cond.counts[js])]}")
    want = args.pred_want
    for seed in args.seeds:
        eng = CTGANEngine(tr.layout, EngineConfig(), dev, backend="hip", seed=seed)
        eng.set_training_data(X)
        eng.set_generation_tables(cond, tr)
        done = 0
        for epochs in sorted(args.epochs):
            for _ in range(epochs - done):
                eng.train_epoch()
            done = epochs
            torch.cuda.synchronize(dev)
            big = eng.generate_decoded(200000)
            share = float(((big[:, js] >= 0.9) & (big[:, js] <= 1.0)).double().mean())
            drive = build_request(tr, meta, vocabs, where, want, dev, counts=cond.counts)
            filt = build_request(tr, meta, vocabs, where, want, dev, counts=cond.counts)
            width = int(tr.layout.cond_width[js])
            opt, cum = driver_table(range(width), cond.counts[js][:width])      # the unconditional sampler's draw
            filt["drv_opt"] = torch.tensor(opt, dtype=torch.int32, device=dev)
            filt["drv_cum"] = torch.tensor(cum, dtype=torch.float64, device=dev)
            res = []
            for label, req in (("drives", drive), ("filters", filt)):
                try:
                    eng.generate_decoded_where(want, req, max_passes=4096)
                    lc = eng.last_conditional
                    res.append(f"{label}: {lc['generated']}/{lc['kept']} = {lc['generated'] / max(lc['kept'], 1):.2f} "
                               f"generated per kept row ({lc['passes']} passes)")
                except RuntimeError as e:
                    res.append(f"{label}: {type(e).__name__}: {e}")
            say(f"    seed {seed}, {epochs} epochs x {eng.steps_per_epoch} steps, {want} rows: " + ";  ".join(res) +
                f";  generate_decoded(200000) holds {share:.4f} inside")
        eng.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pred", action="store_true", help="measure the range / set predicates: (c) and (d)")
    ap.add_argument("--pred_rows", type=int, default=65536)
    ap.add_argument("--pred_want", type=int, default=20000)
    ap.add_argument("--csv", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "data", "raw",
                                                  "Intrusion_test.csv"))
    ap.add_argument("--rows", type=int, default=40960)
    ap.add_argument("--table_rows", type=int, default=4000)
    ap.add_argument("--epochs", type=int, nargs="+", default=[40, 400], help="report after each of these epoch counts")
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fed_tgan_amd.data.demo import small_table
    from fed_tgan_amd.models.conditional import build_request
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.samplers import CondTables
    if not torch.cuda.is_available():
        raise SystemExit("cond_probe measures on the GPU; none found")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.pred:
        pred_probe(args, dev, say)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    _, df, _, meta, vocabs, _, tr, X = small_table(args.table_rows, 0)
    names = [c["column_name"] for c in meta["columns"]]
    jc = names.index("class")
    counts = df["class"].value_counts()
    say(f"table: small_table({args.table_rows}, 0), {len(names)} columns, data_dim {tr.layout.data_dim}, "
        f"n_opt {tr.layout.n_opt}; class counts {dict((k, int(v)) for k, v in counts.items())}")
    m = args.rows
    n_cols = len(names)

    # ---------------------------------------------------------------- (a) pass cost
    eng = CTGANEngine(tr.layout, EngineConfig(gen_chunk=max(m, 40960)), dev, backend="hip", seed=1)
    eng.set_training_data(X)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    # the output layer copies the conditional vector onto the categorical logits (weight 60 beats the Gumbel noise):
    # every generated row carries the requested value, so the partition moves the whole table -- its full traffic
    wire(eng, tr, continuous=False)
    eng.generate_decoded(m)
    plain = eng._gen_graphs[m].graph
    common = str(counts.index[0])
    req = build_request(tr, meta, vocabs, {"class": common}, m, dev)
    eng.generate_decoded_where(m, req, chunk=m, max_passes=64)
    lc = eng.last_conditional
    ent = eng._cond_ent[(m, 1, 0)]
    filled = ent["req"]["filled"]

    def cond_pass():            # the quota reopened before every replay: each pass writes every row it keeps
        filled.zero_()
        ent["graph"].replay()
    say(f"(a) one pass of {m} rows, hipGraph replays, {args.reps} per window, alternating; bytes of the decoded table "
        f"{m * n_cols * 8 / 1e6:.1f} MB; class={common!r} with the wired output layer keeps "
        f"{lc['kept']}/{lc['generated']} rows")
    for rnd in range(4):
        a = replay_us(plain.replay, dev, args.reps)
        b = replay_us(cond_pass, dev, args.reps)
        z = replay_us(filled.zero_, dev, args.reps)
        say(f"    round {rnd}: plain pass {a:7.1f} us   conditional pass {b:7.1f} us (incl. the counter reset, alone "
            f"{z:5.1f} us)   added {b - a:6.1f} us = {100 * (b - a) / a:5.1f} %")
    eng.release()

    # ---------------------------------------------------------------- (b) acceptance on a trained model
    picks = [str(counts.index[-1]), str(counts.index[len(counts) // 2]), str(counts.index[1])]
    for seed in args.seeds:
        eng = CTGANEngine(tr.layout, EngineConfig(), dev, backend="hip", seed=seed)
        eng.set_training_data(X)
        eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
        done = 0
        for epochs in sorted(args.epochs):
            t0 = time.perf_counter()
            for _ in range(epochs - done):
                eng.train_epoch()
            torch.cuda.synchronize(dev)
            say(f"(b) seed {seed}: {epochs} epochs x {eng.steps_per_epoch} steps (+{epochs - done} in "
                f"{time.perf_counter() - t0:.2f} s), losses {eng.losses()}")
            done = epochs
            big = eng.generate_decoded(200000)
            for label in picks:
                code = float([v for v in vocabs if v.column_name == "class"][0].tolist().index(label))
                plain_rate = float((big[:, jc] == code).double().mean())
                want = 5000
                req = build_request(tr, meta, vocabs, {"class": label}, want, dev)
                try:
                    eng.generate_decoded_where(want, req, max_passes=4096)      # (captures the pass on first use)
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    eng.generate_decoded_where(want, req, max_passes=4096)
                    torch.cuda.synchronize(dev)
                    dt = time.perf_counter() - t0
                    lc = eng.last_conditional
                    rate = lc["kept"] / max(lc["generated"], 1)
                    say(f"    class={label!r} ({int(counts[label])}/{len(df)} training rows): conditioned kept "
                        f"{lc['kept']}/{lc['generated']} = {rate:.4f} ({lc['passes']} passes, {want} rows in "
                        f"{dt * 1e3:.2f} ms);  filtering generate_decoded(200000) keeps {plain_rate:.5f};  "
                        f"ratio {rate / max(plain_rate, 1e-12):.1f}x")
                except RuntimeError as e:
                    say(f"    class={label!r}: {type(e).__name__}: {e};  filtering keeps {plain_rate:.5f}")
        eng.release()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
