"""The privacy evaluator's contract on the CPU: the reference ops (ops/ref.py TorchOps nn_*) and the front end
(eval/privacy.py DevicePrivacy, LoadedGenerator.privacy, ``dtds.sample -privacy_against``) against the plain-numpy
brute force of privacy_cases.py.  Bounds: privacy_cases.TOL (derived there)."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

import privacy_cases as pc
from fed_tgan_amd.eval import DevicePrivacy
from fed_tgan_amd.eval.privacy import code_real_table
from fed_tgan_amd.ops.ref import TorchOps

REF = TorchOps()


# ----------------------------------------------------------------------------- TorchOps against the brute force
@pytest.mark.parametrize("nq,nr", [(1, 1), (1, 2), (7, 3), (300, 257)])
@pytest.mark.parametrize("layout", ["cont", "cat", "small", "intrusion", "wide"])
def test_reference_top2_matches_brute_force(nq, nr, layout):
    n_cont, n_cat = pc.LAYOUTS[layout]
    for same in (False, True):
        q_cont, q_cat, r_cont, r_cat = pc.random_packed(nq, nr, n_cont, n_cat, seed=nq * 1000 + nr, same=same)
        w1, w2, wi, _ = pc.top2(q_cont, q_cat, r_cont, r_cat, exclude_self=same)
        d1, d2, i1 = pc.run_top2(REF, "cpu", q_cont, q_cat, r_cont, r_cat, same)
        pc.assert_top2(d1, d2, i1, w1, w2, q_cont, q_cat, r_cont, r_cat, same, f"{layout} {nq}x{nr} same={same}")
        if n_cont == 0:       # integer distances: the tie-break is exact
            assert np.array_equal(i1, wi)


@pytest.mark.parametrize("nq,nr", [(1, 1), (1, 2), (7, 3), (300, 257)])
def test_reference_scores_match_brute_force(nq, nr):
    g = np.random.default_rng(nq + nr)
    kinds = [pc.CONT, pc.CAT, pc.CONT, pc.CAT, pc.CONT, pc.CONT, pc.CAT]
    def table(n):       # noqa: E306
        t = g.normal(size=(n, len(kinds))) * 3.0 + 1.0
        for j, k in enumerate(kinds):
            if k == pc.CAT:
                t[:, j] = g.integers(0, 3, n)
        return t
    real, fake = table(nr), table(nq)
    fake[::3] = real[g.integers(0, nr, len(fake[::3]))]           # copied records
    want = pc.expected(real, fake, kinds)
    ev = pc.coded_evaluator(real, kinds, max_rows=nq)
    s = ev.score(torch.from_numpy(fake))
    pc.assert_scores(s.floats(), want, f"{nq}x{nr}")
    dcr, nndr, i1 = s.rows()
    assert np.abs(dcr.numpy() - want["dcr"]).max() <= pc.TOL and np.abs(nndr.numpy() - want["nndr"]).max() <= pc.TOL
    assert i1.dtype == torch.int32 and bool((dcr[::3] == 0.0).all())
    assert want["copies"] >= 1.0 / 3.0 and s.floats()["copies"] == want["copies"]


# ----------------------------------------------------------------------------- exact cases (privacy_cases.py)
def test_exact_cases():
    pc.check_exact_cases(REF, "cpu", 40, [(3, 30), (5, 6)])


def test_single_reference_row():
    pc.check_single_reference_row(REF, "cpu")


def test_constant_real_column_has_scale_one():
    kinds = [pc.CONT, pc.CONT, pc.CAT]
    real = np.array([[5.0, 0.0, 0.0], [5.0, 4.0, 1.0], [5.0, 2.0, 1.0]])
    fake = np.array([[7.0, 1.0, 1.0], [5.0, 4.0, 1.0]])
    ev = pc.coded_evaluator(real, kinds, max_rows=2)
    assert ev.scale.tolist() == [1.0, 0.25] and ev.lo.tolist() == [5.0, 0.0]
    s = ev.score(torch.from_numpy(fake))
    assert s.rows()[0].tolist() == [(4.0 + 0.0625) ** 0.5, 0.0] and s.rows()[2].tolist() == [2, 1]
    pc.assert_scores(s.floats(), pc.expected(real, fake, kinds))


# ----------------------------------------------------------------------------- construction and API
def test_real_category_outside_the_vocabulary_never_matches():
    _, df, _, meta, vocabs, enc, _, _ = pc.small_table()
    names = [c["column_name"] for c in meta["columns"]]
    cat = next(c["column_name"] for c in meta["columns"] if c["type"] == "categorical")
    j = names.index(cat)
    real = df.iloc[:200].copy()
    real.loc[real.index[:50], cat] = "only_in_real"
    coded = code_real_table(real, meta, vocabs)
    assert (coded[:50, j] >= len(vocabs[0])).all() and np.array_equal(coded[50:], np.asarray(enc)[50:200])
    fake = np.ascontiguousarray(np.asarray(enc)[:200], dtype=np.float64)     # the same rows with their true category
    kinds = [pc.CAT if c["type"] == "categorical" else pc.CONT for c in meta["columns"]]
    want = pc.expected(coded, fake, kinds)
    s = DevicePrivacy(real, meta, vocabs, "cpu", max_rows=200).score(torch.from_numpy(fake))
    pc.assert_scores(s.floats(), want)
    d1 = s.rows()[0].numpy() ** 2
    assert (d1[:50] > 0.0).all() and (d1[50:] == 0.0).all()       # their own record is a full mismatch away now
    assert float(s.buf[3]) == 0.75


def test_date_tables_and_non_finite_values_are_refused():
    _, df, _, meta, vocabs, enc, _, _ = pc.small_table()
    with pytest.raises(ValueError, match="date"):
        DevicePrivacy(df.iloc[:50], dict(meta, date_info={"when": "%Y"}), vocabs, "cpu")
    cont = next(c["column_name"] for c in meta["columns"] if c["type"] != "categorical")
    for bad in (np.nan, np.inf):
        real = df.iloc[:50].copy()
        real[cont] = real[cont].astype(np.float64)
        real.loc[real.index[7], cont] = bad
        with pytest.raises(ValueError, match=cont):
            DevicePrivacy(real, meta, vocabs, "cpu")
    coded = np.asarray(enc)[:50].astype(np.float64).copy()
    coded[3, [c["column_name"] for c in meta["columns"]].index(cont)] = np.nan
    with pytest.raises(ValueError, match=cont):
        DevicePrivacy(coded, meta, vocabs, "cpu")


def test_score_checks_its_input():
    _, df, _, meta, vocabs, enc, _, _ = pc.small_table()
    ev = DevicePrivacy(df.iloc[:50], meta, vocabs, "cpu", max_rows=10, baseline=False)
    ok = torch.from_numpy(np.asarray(enc)[:10].astype(np.float64).copy())
    assert np.isnan(ev.score(ok).floats()["dcr_rr_p5"])
    with pytest.raises(ValueError, match="expected a float64"):
        ev.score(ok.float())
    with pytest.raises(ValueError, match="expected a float64"):
        ev.score(ok[:, :-1])
    with pytest.raises(ValueError, match="buffers hold 1..10"):
        ev.score(torch.cat([ok, ok]))


def test_frame_and_coded_array_give_identical_scores():
    _, df, _, meta, vocabs, enc, _, _ = pc.small_table()
    enc = np.ascontiguousarray(np.asarray(enc), dtype=np.float64)
    assert np.array_equal(code_real_table(df, meta, vocabs), enc)          # the matrix the clients train on
    fake = torch.from_numpy(enc[900:1300] + 0.0)
    a = DevicePrivacy(df.iloc[:600], meta, vocabs, "cpu", max_rows=400).score(fake)
    b = DevicePrivacy(enc[:600], meta, vocabs, "cpu", max_rows=400).score(fake)
    assert torch.equal(a.buf.view(torch.int64), b.buf.view(torch.int64))
    kinds = [pc.CAT if c["type"] == "categorical" else pc.CONT for c in meta["columns"]]
    pc.assert_scores(a.floats(), pc.expected(enc[:600], enc[900:1300], kinds), "small_table")


def test_loaded_generator_and_sample_cli(tmp_path, capsys):
    import dtds.sample
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.generator_io import export_generator, load_generator
    from fed_tgan_amd.models.samplers import CondTables
    _, df, _, meta, vocabs, _, tr, X = pc.small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), "cpu", backend="torch", seed=5)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    path, real_csv, out = str(tmp_path / "g.pt"), str(tmp_path / "real.csv"), str(tmp_path / "s.csv")
    export_generator(path, eng, tr, CondTables.from_encoded(X, tr.layout), meta, vocabs, "Intrusion")
    df.iloc[:400].to_csv(real_csv, index=False)
    real = pd.read_csv(real_csv)
    # the table a fresh generator with this seed produces first, scored by hand
    # (the torch backend draws from torch's global generator)
    gen = load_generator(path, torch.device("cpu"), backend="torch", seed=0)
    torch.manual_seed(11)
    want = DevicePrivacy(real, meta, vocabs, "cpu", max_rows=150).score(gen.device_table(150)).floats()
    torch.manual_seed(11)
    got = load_generator(path, torch.device("cpu"), backend="torch", seed=0).privacy(real, n=150)
    assert got == want and tuple(got) == pc.KEYS
    torch.manual_seed(11)
    dtds.sample.main(["-model", path, "-n", "150", "-backend", "torch", "-seed", "0", "-out", out, "-privacy_against",
                      real_csv, "-score_against", real_csv])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-2].startswith("Avg_JSD ") and lines[-3].startswith("150 rows -> ")
    line = json.loads(lines[-1])
    assert tuple(line) == pc.KEYS and line == want
    assert len(pd.read_csv(out)) == 150
    # with -where: the scored rows are the conditional request's
    dtds.sample.main(["-model", path, "-n", "60", "-backend", "torch", "-out", out, "-privacy_against", real_csv,
                      "-where", "protocol_type=udp"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert tuple(line) == pc.KEYS and line["dcr_rr_p5"] == want["dcr_rr_p5"] and line["dcr_p5"] >= 0.0
