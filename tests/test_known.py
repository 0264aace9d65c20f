"""Completion of partial rows on the CPU path (torch backend): parse_known, the per-row driver choice, the reference
known_request / known_match ops on hand-made cases, the engine end to end with the wired generator, and the
saved-generator interface (LoadedGenerator.complete, ``python -m dtds.sample -known``)."""
import copy

import numpy as np
import pandas as pd
import pytest
import torch

import known_cases as kc
from cond_helpers import code as _code, names as _names, wire_generator
from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
from fed_tgan_amd.models.known import build_known, column_scales, parse_known
from fed_tgan_amd.models.samplers import CondTables
from fed_tgan_amd.ops.ref import TorchOps
from helpers import small_table

OPS = TorchOps()


# ----------------------------------------------------------------------------- parse_known
def _frame(n=6):
    _, df, _, meta, vocabs, _, tr, _ = small_table()
    return df.iloc[:n].reset_index(drop=True).copy(), meta, vocabs, tr


def test_parse_known_absent_blank_empty_and_log1p():
    df, meta, vocabs, tr = _frame()
    names = _names(meta)
    jp, jd, jc = names.index("protocol_type"), names.index("src_bytes"), names.index("class")
    assert "src_bytes" in meta["non_negative_cols"]
    part = df.drop(columns=["class"]).astype(object)
    part.loc[1, "protocol_type"] = ""
    part.loc[2, "protocol_type"] = None
    part.loc[3, "src_bytes"] = np.nan
    part.loc[4, "src_bytes"] = 7
    known, mask = parse_known(part, meta, vocabs, tr)
    assert known.shape == mask.shape == (6, len(names)) and mask.dtype == np.uint8 and known.dtype == np.float64
    assert not mask[:, jc].any()                                   # a column the table lacks: unknown for every row
    assert mask[:, jp].tolist() == [1, 0, 0, 1, 1, 1]              # blanks and None
    assert known[0, jp] == _code(vocabs, "protocol_type", df.loc[0, "protocol_type"])
    assert mask[:, jd].tolist() == [1, 1, 1, 0, 1, 1] and known[4, jd] == np.log1p(7.0)
    # any column order, and a CSV read as text gives the same arrays
    k2, m2 = parse_known(part[part.columns[::-1]], meta, vocabs, tr)
    assert np.array_equal(k2, known) and np.array_equal(m2, mask)


def test_parse_known_csv_and_the_empty_category(tmp_path):
    df, meta, vocabs, tr = _frame()
    names = _names(meta)
    jf = names.index("flag")
    voc = [v for v in vocabs if v.column_name == "flag"][0]
    # a vocabulary and a model that know the category the CSV prints as a blank
    voc2 = copy.deepcopy(vocabs)
    tr2 = copy.copy(tr)
    tr2.meta = copy.deepcopy(tr.meta)
    labels = list(voc.tolist())
    if "empty" not in labels:
        v2 = [v for v in voc2 if v.column_name == "flag"][0]
        v2.__init__(labels + ["empty"], "flag")
        tr2.meta[jf]["i2s"] = list(tr2.meta[jf]["i2s"]) + [len(labels)]
        labels = labels + ["empty"]
    part = df[["flag", "src_bytes"]].astype(object)
    part.loc[0, "flag"] = "empty"
    part.loc[1, "flag"] = ""
    path = str(tmp_path / "p.csv")
    part.to_csv(path, index=False)
    known, mask = parse_known(path, meta, voc2, tr2)
    assert mask[:, jf].tolist() == [1, 0, 1, 1, 1, 1] and known[0, jf] == labels.index("empty")


def test_parse_known_errors():
    df, meta, vocabs, tr = _frame()
    part = df.copy().astype(object)
    part.loc[3, "protocol_type"] = "ipx"
    with pytest.raises(ValueError, match=r"column 'protocol_type': value 'ipx' \(row 3\) is not in the vocabulary"):
        parse_known(part, meta, vocabs, tr)
    tr2 = copy.copy(tr)
    tr2.meta = copy.deepcopy(tr.meta)
    jp = _names(meta).index("protocol_type")
    tr2.meta[jp]["i2s"] = [1, 0]                                   # this model never saw udp (code 2)
    part = df.copy().astype(object)
    part.loc[2, "protocol_type"] = "udp"
    part.loc[5, "protocol_type"] = "udp"
    rows = [i for i in range(6) if part.loc[i, "protocol_type"] == "udp"]
    with pytest.raises(ValueError, match=rf"'protocol_type': value 'udp' \(row {rows[0]}\) is not among the model's"):
        parse_known(part, meta, vocabs, tr2)
    part = df.copy().astype(object)
    part.loc[1, "src_bytes"] = -2
    with pytest.raises(ValueError, match=r"'src_bytes' is non-negative; value -2 \(row 1\) is negative"):
        parse_known(part, meta, vocabs, tr)
    part.loc[1, "src_bytes"] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        parse_known(part, meta, vocabs, tr)
    part.loc[1, "src_bytes"] = "abc"
    with pytest.raises(ValueError, match="not a number"):
        parse_known(part, meta, vocabs, tr)
    with pytest.raises(ValueError, match="columns the model does not have"):
        parse_known(df.assign(extra=1), meta, vocabs, tr)
    with pytest.raises(ValueError, match="date columns"):
        parse_known(df, dict(meta, date_info={"when": "YYYY-MM-DD"}), vocabs, tr)


# ----------------------------------------------------------------------------- driver choice
def test_driver_choice():
    _, _, _, meta, vocabs, enc, tr, X = small_table()
    names = _names(meta)
    counts = np.asarray(CondTables.from_encoded(X, tr.layout).counts, dtype=np.float64)
    jp, jc, jd = names.index("protocol_type"), names.index("class"), names.index("src_bytes")
    n_cols = len(names)
    known = np.zeros((5, n_cols))
    mask = np.zeros((5, n_cols), dtype=np.uint8)
    opt_of = lambda j, o: float(tr.meta[j]["i2s"][o])      # noqa: E731
    rare_c = int(np.argmin(counts[jc][:len(tr.meta[jc]["i2s"])]))
    common_p = int(np.argmax(counts[jp][:len(tr.meta[jp]["i2s"])]))
    # row 0: a common protocol and the rarest class -> class drives
    known[0, jp], known[0, jc] = opt_of(jp, common_p), opt_of(jc, rare_c)
    mask[0, [jp, jc]] = 1
    # row 1: only the protocol; a continuous cell beside it changes nothing
    known[1, jp], known[1, jd] = opt_of(jp, common_p), 0.5
    mask[1, [jp, jd]] = 1
    # row 2: only a continuous cell, at the mean of one of its modes
    from fed_tgan_amd.models.conditional import mode_tables
    mu, sd = mode_tables(tr, jd)
    k_far = int(np.argmax(mu))
    known[2, jd] = mu[k_far]
    mask[2, jd] = 1
    # row 3: nothing known; row 4: a continuous cell no mode reaches
    known[4, jd] = float((mu + 4 * sd).max() + 100.0)
    mask[4, jd] = 1
    tab = build_known(tr, counts, known, mask)
    assert tab["drv_span"].tolist()[:2] == [jc, jp] and tab["drv_opt"].tolist()[:2] == [rare_c, common_p]
    z = (mu[k_far] - mu) / sd
    w = np.where(np.abs(z) <= 4, counts[jd][:len(mu)] * np.exp(-0.5 * z * z) / sd, -1.0)
    assert tab["drv_span"][2] == jd and tab["drv_opt"][2] == int(np.argmax(w))
    assert tab["drv_span"].tolist()[3:] == [-1, -1]
    # a tie goes to the lowest column: two categorical cells whose options have equal counts
    c2 = counts.copy()
    c2[jc][rare_c] = c2[jp][common_p]
    tab = build_known(tr, c2, known[:1], mask[:1])
    assert tab["drv_span"].tolist() == [min(jp, jc)]
    kind, scale = column_scales(tr)
    assert kind[jp] == 1 and kind[jd] == 0 and scale[jd] == 1.0 / (tr.meta[jd]["max"] - tr.meta[jd]["min"])
    with pytest.raises(ValueError, match="not among the model's options"):
        bad = known[:1].copy()
        bad[0, jp] = 99.0
        build_known(tr, counts, bad, mask[:1])


# ----------------------------------------------------------------------------- the reference ops
def _hand():
    """2 continuous columns (scales 1, 1/2), 1 categorical; one query knowing all three; 4 candidates."""
    return {"known": torch.tensor([[1.0, 2.0, 5.0]], dtype=torch.float64),
            "mask": torch.ones(1, 3, dtype=torch.uint8), "qidx": torch.tensor([0], dtype=torch.int32), "tries": 4,
            "kind": torch.tensor([0, 0, 1], dtype=torch.int32), "scale": torch.tensor([1.0, 0.5], dtype=torch.float64
                                                                                       ).repeat(2)[:3].contiguous(),
            "cand": torch.tensor([[1.0, 2.0, 6.0],      # d2 = 0 + 1
                                  [2.0, 2.0, 5.0],      # d2 = 1 + 0
                                  [1.0, 4.0, 5.0],      # d2 = (2 * 0.5)^2 = 1
                                  [3.0, 2.0, 5.0]], dtype=torch.float64), "N": 1}


def test_ref_match_argmin_ties_and_bookkeeping():
    case = _hand()
    st, dst = kc.fresh_state(1), kc.fresh_dst(1, 3)
    kc.run_match(OPS, case, st, dst)
    # three candidates at d2 = 1: the lowest index wins, and its parts are recorded
    assert st["best"].tolist() == [1.0] and st["pick"].tolist() == [0] and st["seen"].tolist() == [4]
    assert st["dc"].tolist() == [0.0] and st["miss"].tolist() == [1]
    assert dst.tolist() == [[1.0, 2.0, 5.0]]                      # everything known: the input comes back
    # strict <: a second pass whose best candidate equals the best so far replaces nothing; seen advances
    case2 = dict(case, cand=case["cand"].flip(0).contiguous())
    kc.run_match(OPS, case2, st, dst)
    assert st["pick"].tolist() == [0] and st["seen"].tolist() == [8] and st["miss"].tolist() == [1]
    # a closer candidate in a third pass wins, numbered among all candidates seen
    cand3 = case["cand"].clone()
    cand3[2] = torch.tensor([1.0, 2.0, 5.0])
    kc.run_match(OPS, dict(case, cand=cand3), st, dst)
    assert st["best"].tolist() == [0.0] and st["pick"].tolist() == [8 + 2] and st["seen"].tolist() == [12]
    assert st["miss"].tolist() == [0]


def test_ref_match_reads_only_known_cells():
    case = kc.exact_case(5, 7, 9, "random", "mixed", seed=3)
    st, dst = kc.fresh_state(case["N"]), kc.fresh_dst(case["N"], 9)
    kc.run_match(OPS, case, st, dst)
    # other values in the query's unknown cells, and in candidate columns no live query knows: same winners
    c2 = dict(case)
    unknown = case["mask"] == 0
    c2["known"] = torch.where(unknown, torch.full_like(case["known"], 123.0), case["known"])
    free = (case["mask"][case["qidx"][case["qidx"] >= 0].long()] == 0).all(0)
    cand = case["cand"].clone()
    cand[:, free] += 1000.0
    st2, dst2 = kc.fresh_state(case["N"]), kc.fresh_dst(case["N"], 9)
    kc.run_match(OPS, c2, st2, dst2, cand=cand)
    assert kc.state_equal(st, st2)
    live = case["qidx"][case["qidx"] >= 0].long()
    for s, i in enumerate(case["qidx"].tolist()):
        if i < 0:
            continue
        t = int(st["pick"][i])
        known = case["mask"][i] != 0
        # known cells are the input's bits, the others the winner's
        assert torch.equal(dst[i][known].view(torch.int64), case["known"][i][known].view(torch.int64))
        assert torch.equal(dst[i][~known], case["cand"][s * 7 + t][~known])
        want = min(kc.d2_of(case, i, case["cand"][s * 7 + u]) for u in range(7))
        assert float(st["best"][i]) == want == kc.d2_of(case, i, case["cand"][s * 7 + t])
        assert all(kc.d2_of(case, i, case["cand"][s * 7 + u]) > want for u in range(t))
    # idle slots and queries outside the pass: nothing written
    rest = torch.ones(case["N"], dtype=torch.bool)
    rest[live] = False
    assert bool((dst[rest] == kc.POISON).all()) and bool(torch.isinf(st["best"][rest]).all())
    assert st["seen"][rest].tolist() == [0] * int(rest.sum()) and st["seen"][live].tolist() == [7] * live.numel()


def test_ref_match_nothing_and_everything_known():
    case = kc.exact_case(4, 5, 6, "none", seed=1)
    st, dst = kc.fresh_state(case["N"]), kc.fresh_dst(case["N"], 6)
    kc.run_match(OPS, case, st, dst)
    for s, i in enumerate(case["qidx"].tolist()):
        if i >= 0:       # d2 = 0 everywhere: candidate 0 of the first pass wins, a plain generated row
            assert st["best"][i] == 0 and st["pick"][i] == 0 and torch.equal(dst[i], case["cand"][s * 5])
    case = kc.exact_case(4, 5, 6, "all", seed=2)
    st, dst = kc.fresh_state(case["N"]), kc.fresh_dst(case["N"], 6)
    kc.run_match(OPS, case, st, dst)
    live = case["qidx"][case["qidx"] >= 0].long()
    assert torch.equal(dst[live], case["known"][live])


def test_ref_request():
    case = kc.request_case(5, 3, seed=4)
    col, opt, h = case["col"].clone(), case["opt"].clone(), case["h"].clone()
    OPS.known_request(case["qidx"], case["drv_span"], case["drv_opt"], 3, col, opt, case["cond"], h=h, c_col0=4)
    off = case["cond"]["cond_offset"].long()
    seen_live = seen_kept = 0
    for b in range(15):
        i = int(case["qidx"][b // 3])
        if i >= 0 and int(case["drv_span"][i]) >= 0:
            sp, o = int(case["drv_span"][i]), int(case["drv_opt"][i])
            assert (int(col[b]), int(opt[b])) == (sp, o)
            assert h[b, 4:].sum() == 1.0 and h[b, 4 + int(off[sp]) + o] == 1.0
            seen_live += 1
        else:
            assert int(col[b]) == int(case["col"][b]) and int(opt[b]) == int(case["opt"][b])
            assert torch.equal(h[b], case["h"][b])
            seen_kept += 1
    assert seen_live and seen_kept and bool((h[:, :4] == 0.5).all())
    with pytest.raises(ValueError, match="tries"):
        OPS.known_request(case["qidx"], case["drv_span"], case["drv_opt"], 1025, col, opt, case["cond"])
    assert OPS.KNOWN_MAX_TRIES == 1024


# ----------------------------------------------------------------------------- the engine
def _engine(seed=3, wired=True, **cfg):
    _, _, _, _, _, _, tr, X = small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200, **cfg), "cpu", backend="torch", seed=seed)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    if wired:
        wire_generator(eng, tr)
    return eng, tr


def _partial(n, seed, p_known=0.5):
    """Rows of the small table's coded form with a random share of the cells known."""
    _, _, _, meta, _, enc, _, _ = small_table()
    rng = np.random.default_rng(seed)
    known = np.ascontiguousarray(np.asarray(enc)[:n], dtype=np.float64)
    return known, (rng.random(known.shape) < p_known).astype(np.uint8), meta


def test_engine_wired_generator_matches_the_driver():
    eng, tr = _engine()
    known, mask, meta = _partial(90, 0)
    mask[0] = 0                                      # nothing known
    mask[1] = 1                                      # everything known
    cat = [j for j, m in enumerate(tr.meta) if m["type"] != "continuous"]
    for r in range(2, 12):                           # rows that know exactly one category: their driver
        mask[r, cat] = 0
        mask[r, cat[r % len(cat)]] = 1
    torch.manual_seed(5)
    out = eng.generate_decoded_known(known, mask, tries=4, retries=1, chunk=64).numpy()
    lk = eng.last_known
    assert out.shape == known.shape and lk["rows"] == 90 and lk["tries"] == 4
    on = mask != 0
    assert np.array_equal(out[on].view(np.int64), known[on].view(np.int64))       # known cells: the input's bits
    assert np.array_equal(out[1], known[1])
    tab = build_known(tr, eng.gen_counts, known, mask)
    has = tab["drv_span"] >= 0
    drove = np.isin(tab["drv_span"], cat)
    assert drove.sum() > 50
    # the wired generator obeys its condition: every candidate of a row carries the driving column's value, so a
    # row whose only known category is its driver misses none, and no row misses all of its known categories
    ent = next(iter(eng._known_ent.values()))
    st = ent["state"]
    n_cat = on[:, cat].sum(1)
    miss = st["miss"][:90].numpy()
    assert (n_cat == 1).sum() > 0 and (miss[n_cat == 1] == 0).all()
    assert (miss[drove] < n_cat[drove]).all()
    assert lk["generated"] == sum(-(-n // 16) for n in [90] + lk["open"][:-1]) * 64
    assert lk["sweeps"] == len(lk["open"]) <= 2 and lk["open"][0] <= 90
    assert has.sum() >= drove.sum() and np.isfinite(lk["d_p50"]) and lk["d_p50"] <= lk["d_p95"] <= lk["d_max"]
    assert lk["exact_categorical"] == float((st["miss"][:90] == 0).double().mean())


def test_engine_one_categorical_column_is_exact_without_retry():
    """A schema with one categorical column, all of whose cells are known: the wired generator answers every
    condition, so sweep 0 leaves no row open and no retry runs."""
    from fed_tgan_amd.features.transformer import VGMTransformer
    rng = np.random.default_rng(0)
    data = np.stack([rng.normal(size=600), rng.integers(0, 4, 600).astype(float), rng.normal(size=600) * 3], 1)
    tr = VGMTransformer().fit(data, (1,), (), seed=0, backend="sklearn")
    X = tr.transform(data, np.random.default_rng(0))
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=100, gen_dims=(32,), dis_dims=(32,), embedding_dim=16), "cpu",
                      backend="torch", seed=1)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    wire_generator(eng, tr)
    known = data[:70].copy()
    mask = np.zeros((70, 3), dtype=np.uint8)
    mask[:, 1] = 1
    mask[::3, 0] = 1
    torch.manual_seed(2)
    out = eng.generate_decoded_known(known, mask, tries=8, retries=2, chunk=200).numpy()
    lk = eng.last_known
    assert (out[:, 1] == known[:, 1]).all() and lk["exact_categorical"] == 1.0
    assert lk["open"] == [0] and lk["sweeps"] == 1 and lk["generated"] == 3 * 200      # q = 25 slots: 3 passes of 70 rows
    assert np.array_equal(out[::3, 0], known[::3, 0])


def test_engine_unknown_rows_are_plain_generation_and_runs_repeat():
    known, mask, _ = _partial(10, 1)
    mask[:] = 0
    tabs = []
    for _ in range(2):
        eng, _ = _engine(wired=False, seed=7)
        torch.manual_seed(9)
        tabs.append(eng.generate_decoded_known(known, mask, tries=3, retries=2, chunk=30))
        assert eng.last_known["open"] == [0] and eng.last_known["d_max"] == 0.0
    assert torch.equal(tabs[0], tabs[1])
    eng, _ = _engine(wired=False, seed=7)
    torch.manual_seed(9)
    plain = eng.generate_decoded(30)
    assert torch.equal(tabs[0], plain[::3])          # candidate 0 of each slot: the row plain generation puts there
    # equal states, partly known rows: bit-identical again
    known, mask, _ = _partial(40, 2)
    outs = []
    for _ in range(2):
        eng, _ = _engine(wired=False, seed=7)
        torch.manual_seed(9)
        outs.append((eng.generate_decoded_known(known, mask, tries=5, chunk=64), copy.deepcopy(eng.last_known)))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]


def test_engine_edges_and_retries_only_lower_best():
    eng, tr = _engine(wired=False, seed=4)
    known, mask, _ = _partial(30, 3)
    assert eng.generate_decoded_known(known[:0], mask[:0]).shape == (0, known.shape[1])
    assert eng.last_known["rows"] == 0 and eng.last_known["generated"] == 0
    with pytest.raises(ValueError, match="tries"):
        eng.generate_decoded_known(known, mask, tries=0)
    with pytest.raises(ValueError, match="tries"):
        eng.generate_decoded_known(known, mask, tries=1025)
    torch.manual_seed(3)
    out1 = eng.generate_decoded_known(known, mask, tries=1, retries=0, chunk=8)
    assert out1.shape == (30, known.shape[1]) and eng.last_known["generated"] == 32 and eng.last_known["sweeps"] == 1
    ent = eng._known_ent[(8, 1)]
    assert ent["state"]["pick"][:30].tolist() == [0] * 30 and ent["state"]["seen"][:30].tolist() == [1] * 30
    # equal states: the run with retries starts with the same sweep 0, and no row ends farther than without them
    best = []
    for retries in (0, 3):
        eng, _ = _engine(wired=False, seed=4)
        torch.manual_seed(3)
        eng.generate_decoded_known(known, mask, tries=2, retries=retries, tol=0.0, chunk=16)
        best.append(eng._known_ent[(16, 2)]["state"]["best"][:30].clone())
        assert eng.last_known["sweeps"] == retries + 1
    assert bool((best[1] <= best[0]).all()) and bool((best[1] < best[0]).any())


def test_synthesizer_sample_remaining_columns():
    from fed_tgan_amd.models.synthesizer import CTGANSynthesizer
    rng = np.random.default_rng(0)
    data = np.stack([rng.normal(size=400), rng.integers(0, 3, 400).astype(float)], 1)
    syn = CTGANSynthesizer(embedding_dim=16, gen_dim=(32,), dis_dim=(32,), batch_size=100, epochs=1, device="cpu",
                           backend="torch", seed=0, verbose=False).fit(data, categorical_columns=(1,))
    known = np.full((12, 2), np.nan)
    known[:6, 0] = data[:6, 0]
    known[6:, 1] = 2.0
    out = syn.sample_remaining_columns(known, tries=8)
    assert out.shape == (12, 2) and np.array_equal(out[:6, 0], data[:6, 0]) and (out[6:, 1] == 2.0).all()
    assert np.isfinite(out).all() and syn.engine.last_known["rows"] == 12


# ----------------------------------------------------------------------------- the saved generator
def test_saved_generator_complete_and_cli(tmp_path, capsys):
    from fed_tgan_amd.models.generator_io import export_generator, load_generator
    import dtds.sample
    _, df, _, meta, vocabs, _, tr, X = small_table()
    eng, _ = _engine(wired=False, seed=5)
    path = str(tmp_path / "g.pt")
    export_generator(path, eng, tr, CondTables.from_encoded(X, tr.layout), meta, vocabs, "Intrusion")
    gen = load_generator(path, torch.device("cpu"), backend="torch", seed=0)
    part = df.iloc[:25].reset_index(drop=True).astype(object)
    rng = np.random.default_rng(0)
    hole = rng.random(part.shape) < 0.5
    part = part.mask(hole, "")
    part["class"] = ""
    vals = gen.complete(part, tries=4)
    known, mask = parse_known(part, meta, vocabs, tr)
    assert vals.shape == known.shape and np.array_equal(vals[mask != 0], known[mask != 0])
    frame = gen.complete_frame(part, tries=4)
    assert list(frame.columns) == _names(meta) and len(frame) == 25
    for name in ("protocol_type", "src_bytes"):
        on = ~hole[:, list(part.columns).index(name)]
        assert frame[name].to_numpy(dtype=object)[on].tolist() == part[name].to_numpy(dtype=object)[on].tolist()
    assert set(frame["class"]) <= set(vocabs[-1].tolist()) | {" "}
    src, out = str(tmp_path / "partial.csv"), str(tmp_path / "full.csv")
    part.to_csv(src, index=False)
    dtds.sample.main(["-model", path, "-known", src, "-known_tries", "4", "-backend", "torch", "-out", out])
    got = pd.read_csv(out, dtype=str, keep_default_na=False)
    assert len(got) == 25 and list(got.columns) == _names(meta)
    on = ~hole[:, list(part.columns).index("protocol_type")]
    assert got["protocol_type"].to_numpy()[on].tolist() == part["protocol_type"].to_numpy()[on].tolist()   # row order
    line = capsys.readouterr().out
    assert "sweeps" in line and "candidates generated" in line and "d_p95" in line
    for extra in (["-where", "protocol_type=udp"], ["-min_dcr", "0", "-guard_against", src], ["-score_against", src],
                  ["-privacy_against", src], ["-where_range", "src_bytes=0:1"]):
        with pytest.raises(SystemExit):
            dtds.sample.main(["-model", path, "-known", src, "-backend", "torch", "-out", out] + extra)
    with pytest.raises(SystemExit):
        dtds.sample.main(["-model", path, "-known_tries", "4", "-backend", "torch", "-out", out])
