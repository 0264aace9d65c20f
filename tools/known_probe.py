"""Completion of partial rows measured (profiles/known.md):

(a) Intrusion schema, ``--rows`` known rows with a random half of the cells blanked, ``--tries`` candidates per row,
    no retry: the whole call, one pass as a hipGraph replay, the pass's ``known_match`` launch alone, the torch-op
    formulation of that launch on the same GPU, and plain ``generate_decoded`` of the same number of rows; device
    events, alternating windows.
(b) on a generator trained on the training rows of the shipped Intrusion split (tools/real_quality.py's 80 / 20
    permutation): the held-out rows with ``class`` blanked, completed -- the share whose filled ``class`` is the true
    one, next to always answering the majority class; and with one continuous column blanked -- the W1 distance
    of filled against true values, next to drawing that column unconditionally.

    python tools/known_probe.py [--rows 40000] [--tries 64] [--epochs 300] [--seeds 1 2] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_us(fn, reps):
    """Device time of ``reps`` calls of fn, per call, from two events on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def med(xs):
    xs = sorted(xs)
    return f"{xs[len(xs) // 2]:9.1f} us ({xs[0]:.1f} - {xs[-1]:.1f})"


def timing(args, dev, say):
    from fed_tgan_amd.data.demo import small_table
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.samplers import CondTables
    from fed_tgan_amd.ops.ref import TorchOps
    _, _, _, meta, _, enc, tr, X = small_table(args.table_rows, 0)
    enc = np.asarray(enc)
    N, R = args.rows, args.tries
    n_cols = enc.shape[1]
    rng = np.random.default_rng(0)
    known = np.ascontiguousarray(enc[np.arange(N) % len(enc)], dtype=np.float64)
    mask = (rng.random(known.shape) < 0.5).astype(np.uint8)
    eng = CTGANEngine(tr.layout, EngineConfig(), dev, backend="hip", seed=1)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    q = int(eng.cfg.gen_chunk) // R
    m = q * R
    say(f"(a) small_table({args.table_rows}, 0): {n_cols} columns; {N} known rows, half of the cells blanked, tries "
        f"{R}, retries 0: {-(-N // q)} passes of {m} rows ({q} slots); one pass's decoded table is "
        f"{m * n_cols * 8 / 1e6:.2f} MB, its known cells and masks {q * n_cols * 9 / 1e3:.1f} KB")
    eng.generate_decoded_known(known, mask, tries=R, retries=0)          # captures the pass
    say(f"    last_known: {eng.last_known}")
    ent = eng._known_ent[(m, R)]
    total = N * R
    eng.generate_decoded(total)                                          # captures the plain generation
    plain = eng._gen_graphs[total].graph
    ent["qidx"].copy_(torch.arange(q, dtype=torch.int32, device=dev))
    st = ent["state"]
    ref = TorchOps()

    def whole():
        eng.generate_decoded_known(known, mask, tries=R, retries=0)

    def match():                 # every query starts open, so every slot writes its row
        st["best"].fill_(float("inf"))
        eng.ops.known_match(ent["known"], ent["mask"], ent["qidx"], R, ent["out"], ent["kind"], ent["scale"], st,
                            ent["dst"])

    def torch_match():
        st["best"].fill_(float("inf"))
        ref.known_match(ent["known"], ent["mask"], ent["qidx"], R, ent["out"], ent["kind"], ent["scale"], st,
                        ent["dst"])
    arms = {"whole call (host prep + passes + report)": (whole, 1), "one pass, hipGraph replay": (ent["graph"].replay, 20),
            "known_match alone (+ the fill of best)": (match, 50), "torch-op known_match, same buffers": (torch_match, 2),
            f"plain generate_decoded({total}), hipGraph replay": (plain.replay, 1),
            "fill of best alone": (lambda: st["best"].fill_(float("inf")), 50)}
    for fn, _ in arms.values():
        fn()
    torch.cuda.synchronize(dev)
    got = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, (fn, reps) in arms.items():
            got[k].append(window_us(fn, reps))
    for k, v in got.items():
        say(f"    {k:55s} {med(v)}")
    t_match = sorted(got["known_match alone (+ the fill of best)"])[args.rounds // 2] - \
        sorted(got["fill of best alone"])[args.rounds // 2]
    t_pass = sorted(got["one pass, hipGraph replay"])[args.rounds // 2]
    say(f"    known_match: {t_match:.1f} us of the pass's {t_pass:.1f} us ({100 * t_match / t_pass:.1f} %); it reads "
        f"{m * n_cols * 8 / 1e6:.2f} MB once: {m * n_cols * 8 / t_match / 1e6:.2f} TB/s")
    eng.release()


def w1(a, b):
    a, b = np.sort(np.asarray(a, dtype=np.float64)), np.sort(np.asarray(b, dtype=np.float64))
    return float(np.abs(a - b).mean())


def quality(args, dev, backend, say):
    import pandas as pd
    from fed_tgan_amd.data.schema import intrusion_spec
    from fed_tgan_amd.data.table import TablePreprocessor
    from fed_tgan_amd.features.transformer import VGMTransformer
    from fed_tgan_amd.fed.stats import merge_categorical_metas
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.known import parse_known
    from fed_tgan_amd.models.samplers import CondTables
    df = pd.read_csv(args.csv)
    if args.max_rows:
        df = df.iloc[:args.max_rows]
    perm = np.random.default_rng(2024).permutation(len(df))
    n_tr = int(round(0.8 * len(df)))
    train, hold = df.iloc[perm[:n_tr]].reset_index(drop=True), df.iloc[perm[n_tr:]].reset_index(drop=True)
    spec = intrusion_spec()
    tp = TablePreprocessor(train, "Intrusion", spec.problem_type, spec.target_column, spec.categorical_list,
                           spec.nonnegative_list)
    meta, vocabs, _ = merge_categorical_metas([tp.local_meta()])
    enc = tp.encode(vocabs)
    cat = tp.categorical_indices()
    tr = VGMTransformer().fit(enc, cat, (), seed=0, backend="torch" if backend == "hip" else "sklearn",
                              **({"device": str(dev)} if backend == "hip" else {}))
    tr.refit(enc, meta, vocabs, cat, (), tr.bank, tr.components)
    X = tr.transform(enc, np.random.default_rng(0))
    names = [c["column_name"] for c in meta["columns"]]
    # held-out rows whose labels the model knows (the others cannot be written as known cells)
    keep = np.ones(len(hold), dtype=bool)
    cursor = 0
    for j, c in enumerate(meta["columns"]):
        if c["type"] == "categorical":
            labels = [str(s) for s in vocabs[cursor].tolist()]
            ok = {labels[int(code)] for code in tr.meta[j]["i2s"]}
            keep &= hold[c["column_name"]].astype(str).isin(ok).to_numpy()
            cursor += 1
    hold = hold[keep].reset_index(drop=True)
    jc, jx = names.index("class"), names.index(args.column)
    full, _ = parse_known(hold.astype(object), meta, vocabs, tr)
    major = float(pd.Series(enc[:, jc]).mode()[0])
    say(f"(b) {os.path.relpath(args.csv, ROOT)}: {len(train)} training rows, {len(hold)} of "
        f"{int((~keep).sum()) + len(hold)} held-out rows with known labels; tries {args.tries}, retries 2; always "
        f"answering the majority class is right on {float((full[:, jc] == major).mean()):.4f} of them")
    for seed in args.seeds:
        eng = CTGANEngine(tr.layout, EngineConfig(), dev, backend=backend, seed=seed)
        eng.set_training_data(X)
        eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
        torch.manual_seed(seed)
        for _ in range(args.epochs):
            eng.train_epoch()
        mask = np.ones(full.shape, dtype=np.uint8)
        mask[:, jc] = 0
        out = eng.generate_decoded_known(full, mask, tries=args.tries).cpu().numpy()
        lk1 = dict(eng.last_known)
        acc = float((out[:, jc] == full[:, jc]).mean())
        mask = np.ones(full.shape, dtype=np.uint8)
        mask[:, jx] = 0
        out = eng.generate_decoded_known(full, mask, tries=args.tries).cpu().numpy()
        lk2 = dict(eng.last_known)
        free = eng.generate_decoded(len(full)).cpu().numpy()
        say(f"    seed {seed}, {args.epochs} epochs x {eng.steps_per_epoch} steps: class blanked: filled == true on "
            f"{acc:.4f} (exact_categorical {lk1['exact_categorical']:.4f}, d_p95 {lk1['d_p95']:.4f}, sweeps "
            f"{lk1['sweeps']});  {args.column} blanked: W1(filled, true) {w1(out[:, jx], full[:, jx]):.4f} against "
            f"W1(unconditional, true) {w1(free[:, jx], full[:, jx]):.4f} in the decoded space (exact_categorical "
            f"{lk2['exact_categorical']:.4f}, d_p95 {lk2['d_p95']:.4f})")
        eng.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=40000)
    ap.add_argument("--tries", type=int, default=64)
    ap.add_argument("--table_rows", type=int, default=4000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--csv", default=os.path.join(ROOT, "data", "raw", "Intrusion_test.csv"))
    ap.add_argument("--column", default="src_bytes", help="the continuous column blanked in (b)")
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--max_rows", type=int, default=0, help="(rehearsal) use only the first rows of the CSV")
    ap.add_argument("--rehearse", action="store_true", help="part (b) alone on the CPU with the torch backend: checks "
                                                            "the code path, measures nothing")
    ap.add_argument("--skip_timing", action="store_true")
    ap.add_argument("--skip_quality", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.rehearse:
        quality(args, torch.device("cpu"), "torch", say)
        return
    if not torch.cuda.is_available():
        raise SystemExit("known_probe measures on the GPU; none found")
    dev = torch.device("cuda:0")
    if not args.skip_timing:
        timing(args, dev, say)
    if not args.skip_quality:
        quality(args, dev, "hip", say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
