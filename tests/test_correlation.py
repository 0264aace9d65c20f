"""The correlation evaluator's contract on the CPU: the reference ops (ops/ref.py TorchOps corr_*) and the front end
(eval/correlation.py DeviceCorrelation, LoadedGenerator.correlation, ``dtds.sample -corr_against``) against the
plain-numpy brute force of correlation_cases.py.  Bounds: correlation_cases.TOL (derived there)."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

import correlation_cases as cc
from fed_tgan_amd.eval import DeviceCorrelation
from fed_tgan_amd.eval.privacy import code_real_table
from fed_tgan_amd.ops.ref import TorchOps

REF = TorchOps()
CONT, CAT = cc.CONT, cc.CAT


def _score(real, fake, kinds, **kw):
    ev = cc.coded_evaluator(real, kinds, "cpu", REF, max_rows=len(fake), **kw)
    return ev, ev.score(torch.from_numpy(np.ascontiguousarray(fake, dtype=np.float64)))


# ----------------------------------------------------------------------------- TorchOps against the brute force
@pytest.mark.parametrize("n", [1, 2, 65, 300])
@pytest.mark.parametrize("layout", list(cc.LAYOUTS))
def test_reference_matches_brute_force(layout, n):
    cc.check_layout(REF, "cpu", layout, n, seed=n)


def test_baseline_is_the_even_odd_split():
    kinds = cc.layout_kinds(4, 3)
    real = cc.random_table(301, kinds, 1)
    fake = cc.random_table(50, kinds, 2)
    ev, s = _score(real, fake, kinds)
    cards = cc.cards_of(real, kinds)
    want = cc.diff_scores(cc.association(real[0::2], kinds, cards), cc.association(real[1::2], kinds, cards))[0]
    assert abs(s.floats()["corr_diff_rr"] - want) <= 2 * cc.TOL and want > 0.0
    assert np.isnan(_score(real, fake, kinds, baseline=False)[1].floats()["corr_diff_rr"])
    assert np.isnan(_score(real[:1], fake, kinds)[1].floats()["corr_diff_rr"])       # fewer than two real rows


# ----------------------------------------------------------------------------- degenerate columns
def test_constant_columns():
    g = np.random.default_rng(0)
    n = 200
    kinds = [CONT, CONT, CAT, CAT]
    t = np.stack([np.full(n, 3.5), g.normal(size=n), np.full(n, 2.0), g.integers(0, 3, n).astype(float)], axis=1)
    ev, s = _score(t, t, kinds)
    A = s.matrix().numpy()
    cc.assert_matrix(A, cc.association(t, kinds, cc.cards_of(t, kinds)), "constant")
    assert (A[0, 1:] == 0.0).all() and (A[1:, 0] == 0.0).all()      # a constant continuous column: r = eta = 0
    assert A[2, 3] == 1.0 and 0.0 <= A[3, 2] <= 1e-12                 # U(const | .) = 1, U(. | const) = 0
    assert 0.0 <= A[2, 1] <= 1e-12 and A[1, 2] == A[2, 1]             # eta of a constant category (a rounded mean)
    assert s.floats()["corr_diff"] == 0.0


def test_identical_and_negated_columns():
    g = np.random.default_rng(1)
    n = 500
    a = g.integers(0, 5, n).astype(float)
    x = g.normal(size=n) * 3.0 + 7.0
    kinds = [CAT, CAT, CONT, CONT, CONT]
    t = np.stack([a, a, x, x, -x], axis=1)
    A = _score(t, t, kinds)[1].matrix().numpy()
    assert abs(A[0, 1] - 1.0) <= 1e-12 and abs(A[1, 0] - 1.0) <= 1e-12
    assert abs(A[2, 3] - 1.0) <= 1e-12 and abs(A[3, 2] - 1.0) <= 1e-12
    assert abs(A[2, 4] + 1.0) <= 1e-12 and abs(A[4, 3] + 1.0) <= 1e-12
    assert (np.abs(A) <= 1.0).all() and (A[:2] >= 0.0).all()


def test_overflow_bin_takes_what_is_no_code():
    g = np.random.default_rng(2)
    kinds = [CAT, CONT, CAT]
    real = np.stack([g.integers(0, 4, 300).astype(float), g.normal(size=300), g.integers(0, 3, 300).astype(float)], 1)
    fake = real[:120].copy()
    fake[::7, 0] = 4.0            # one past the last code
    fake[1::7, 0] = -1.0
    fake[2::7, 0] = np.nan
    fake[3::7, 2] = 1e12
    fake[4::7, 2] = -np.inf
    want = cc.expected(real, fake, kinds)
    ev, s = _score(real, fake, kinds)
    cc.assert_matrix(s.matrix().numpy(), want["A_fake"], "overflow")
    cc.assert_scores(s.floats(), want, 3, "overflow")
    _, _, counts = cc.run_matrix(REF, ev, fake)
    assert counts[4] == len(fake[::7]) + len(fake[1::7]) + len(fake[2::7])       # the margin's overflow bin
    clean = cc.expected(real, real[:120], kinds)
    assert abs(want["corr_diff"] - clean["corr_diff"]) > 1e-3                     # the bin behaves like a category


def test_real_category_outside_the_vocabulary():
    _, df, _, meta, vocabs, enc, _, _ = cc.small_table()
    names = [c["column_name"] for c in meta["columns"]]
    cat = next(c["column_name"] for c in meta["columns"] if c["type"] == "categorical")
    j = names.index(cat)
    real = df.iloc[:300].copy()
    real.loc[real.index[:60], cat] = "only_in_real"
    ev = DeviceCorrelation(real, meta, vocabs, "cpu", max_rows=200)
    assert ev.card_list[0] == len(vocabs[0]) + 1
    coded = code_real_table(real, meta, vocabs)
    kinds = [CAT if c["type"] == "categorical" else CONT for c in meta["columns"]]
    cards = [len(v) for v in vocabs]
    fake = np.ascontiguousarray(np.asarray(enc)[300:500], dtype=np.float64)
    want = cc.expected(coded, fake, kinds, cardinalities=cards, check_entropy=False)
    assert want["cards"][0] == len(vocabs[0]) + 1 and coded[:60, j].min() >= len(vocabs[0])
    s = ev.score(torch.from_numpy(fake))
    cc.assert_scores(s.floats(), want, len(kinds), "unseen")


# ----------------------------------------------------------------------------- construction and API
def test_frame_and_coded_array_give_identical_scores():
    _, df, _, meta, vocabs, enc, _, _ = cc.small_table()
    enc = np.ascontiguousarray(np.asarray(enc), dtype=np.float64)
    fake = torch.from_numpy(enc[900:1300] + 0.0)
    a = DeviceCorrelation(df.iloc[:600], meta, vocabs, "cpu", max_rows=400).score(fake)
    b = DeviceCorrelation(enc[:600], meta, vocabs, "cpu", max_rows=400).score(fake)
    c = DeviceCorrelation(enc[:600], meta, [], "cpu", max_rows=400, cardinalities=[len(v) for v in vocabs]).score(fake)
    assert torch.equal(a.buf.view(torch.int64), b.buf.view(torch.int64))
    assert torch.equal(a.buf.view(torch.int64), c.buf.view(torch.int64))
    assert torch.equal(a.matrix(), b.matrix())
    p = a.pairs(5)
    assert list(p.columns) == ["column_i", "column_j", "kind", "real", "fake", "abs_diff"] and len(p) == 5
    names = [col["column_name"] for col in meta["columns"]]
    assert set(p["column_i"]) <= set(names) and set(p["column_j"]) <= set(names)
    assert set(p["kind"]) <= {"pearson", "theils_u", "correlation_ratio"}
    assert p["abs_diff"].is_monotonic_decreasing and abs(p["abs_diff"][0] - a.floats()["corr_max_abs"]) == 0.0


def test_date_tables_and_non_finite_values_are_refused():
    _, df, _, meta, vocabs, enc, _, _ = cc.small_table()
    with pytest.raises(ValueError, match="date"):
        DeviceCorrelation(df.iloc[:50], dict(meta, date_info={"when": "%Y"}), vocabs, "cpu")
    cont = next(c["column_name"] for c in meta["columns"] if c["type"] != "categorical")
    for bad in (np.nan, np.inf):
        real = df.iloc[:50].copy()
        real[cont] = real[cont].astype(np.float64)
        real.loc[real.index[7], cont] = bad
        with pytest.raises(ValueError, match=cont):
            DeviceCorrelation(real, meta, vocabs, "cpu")
    coded = np.asarray(enc)[:50].astype(np.float64).copy()
    coded[3, [c["column_name"] for c in meta["columns"]].index(cont)] = np.nan
    with pytest.raises(ValueError, match=cont):
        DeviceCorrelation(coded, meta, vocabs, "cpu")
    with pytest.raises(ValueError, match="coded"):
        DeviceCorrelation(coded[:, :-1], meta, vocabs, "cpu")


def test_score_checks_its_input():
    _, df, _, meta, vocabs, enc, _, _ = cc.small_table()
    ev = DeviceCorrelation(df.iloc[:50], meta, vocabs, "cpu", max_rows=10, baseline=False)
    ok = torch.from_numpy(np.asarray(enc)[:10].astype(np.float64).copy())
    assert np.isnan(ev.score(ok).floats()["corr_diff_rr"])
    with pytest.raises(ValueError, match="expected a float64"):
        ev.score(ok.float())
    with pytest.raises(ValueError, match="expected a float64"):
        ev.score(ok[:, :-1])
    with pytest.raises(ValueError, match="buffers hold 1..10"):
        ev.score(torch.cat([ok, ok]))
    with pytest.raises(ValueError, match="the evaluator on"):
        ev.score(ok.to("meta"))


def test_scratch_limit_names_the_columns():
    kinds = [CAT, CONT, CAT]
    real = np.zeros((10, 3))
    real[0, 0], real[0, 2] = 999.0, 1999.0
    with pytest.raises(ValueError, match=r"'c2' \(2000\).*'c0' \(1000\)"):
        cc.coded_evaluator(real, kinds, max_scratch_bytes=1 << 20)
    ev = cc.coded_evaluator(real, kinds)
    assert ev.global_pairs == [(0, 1)] and ev.scratch_bytes == 4 * (1001 + 2001 + 1001 * 2001)


# ----------------------------------------------------------------------------- planted dependence
def test_planted_dependence_is_seen():
    real, kinds = cc.planted(4000, 0)
    fresh, _ = cc.planted(4000, 1)
    ev, s = _score(real, fresh, kinds)
    u_ba = float(ev.A_real[1, 0])
    print("U(b|a)", u_ba, s.floats())
    assert abs(u_ba - 0.75) <= 0.05
    assert s.floats()["corr_max_abs"] <= 0.1
    g = np.random.default_rng(5)
    shuffled = np.stack([g.permutation(real[:, j]) for j in range(3)], axis=1)
    f = ev.score(torch.from_numpy(shuffled)).floats()
    print("shuffled", f)
    assert f["corr_max_abs"] >= 0.5 and f["corr_diff"] > 10 * f["corr_diff_rr"]


# ----------------------------------------------------------------------------- front ends
def test_loaded_generator_and_sample_cli(tmp_path, capsys):
    import dtds.sample
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.generator_io import export_generator, load_generator
    from fed_tgan_amd.models.samplers import CondTables
    _, df, _, meta, vocabs, _, tr, X = cc.small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), "cpu", backend="torch", seed=5)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    path, real_csv, out = str(tmp_path / "g.pt"), str(tmp_path / "real.csv"), str(tmp_path / "s.csv")
    export_generator(path, eng, tr, CondTables.from_encoded(X, tr.layout), meta, vocabs, "Intrusion")
    df.iloc[:400].to_csv(real_csv, index=False)
    real = pd.read_csv(real_csv)
    gen = load_generator(path, torch.device("cpu"), backend="torch", seed=0)
    torch.manual_seed(11)
    want = DeviceCorrelation(real, meta, vocabs, "cpu", max_rows=150).score(gen.device_table(150)).floats()
    torch.manual_seed(11)
    got = load_generator(path, torch.device("cpu"), backend="torch", seed=0).correlation(real, n=150)
    assert got == want and tuple(got) == cc.KEYS and want["corr_diff"] > 0.0
    # all three evaluators at once: the existing lines keep their order, the correlation line is last
    torch.manual_seed(11)
    dtds.sample.main(["-model", path, "-n", "150", "-backend", "torch", "-seed", "0", "-out", out, "-corr_against",
                      real_csv, "-privacy_against", real_csv, "-score_against", real_csv])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-4].startswith("150 rows -> ") and lines[-3].startswith("Avg_JSD ")
    assert tuple(json.loads(lines[-2])) == ("dcr_p5", "nndr_p5", "dcr_min", "copies", "dcr_rr_p5", "nndr_rr_p5")
    line = json.loads(lines[-1])
    assert tuple(line) == cc.KEYS and line == want
    assert len(pd.read_csv(out)) == 150
    # alone
    torch.manual_seed(11)
    dtds.sample.main(["-model", path, "-n", "150", "-backend", "torch", "-seed", "0", "-out", out, "-corr_against",
                      real_csv])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-2].startswith("150 rows -> ") and json.loads(lines[-1]) == want
    # without the flag nothing new is printed
    dtds.sample.main(["-model", path, "-n", "20", "-backend", "torch", "-out", out])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("20 rows -> ")
    # with -where: the scored rows are the conditional request's
    dtds.sample.main(["-model", path, "-n", "60", "-backend", "torch", "-out", out, "-corr_against", real_csv,
                      "-where", "protocol_type=udp"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert tuple(line) == cc.KEYS and line["corr_diff_rr"] == want["corr_diff_rr"] and line["corr_diff"] > 0.0
    # write_csv_evaluated keeps its two-tuple
    res = gen.write_csv_evaluated(out, 30, privacy_real=real)
    assert len(res) == 2 and res[0] is None and tuple(res[1])[:1] == ("dcr_p5",)
