"""The fidelity evaluator (eval/fidelity.py) on the CPU: the reference ops (ops/ref.py nn_topk / nn_ball / prdc_reduce)
and DeviceFidelity end to end against the plain-numpy brute force of fidelity_cases.py.  Both accumulate a distance
without contraction in column order, so everything is compared bit for bit."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

import fidelity_cases as fc
import privacy_cases as pc
from fed_tgan_amd.eval import DeviceFidelity, FidelityScores
from fed_tgan_amd.eval.fidelity import FID_MAX_K, KEYS
from fed_tgan_amd.ops.ref import TorchOps

REF = TorchOps()
KS = (1, 2, 5, 8)


def test_constants_agree():
    assert FID_MAX_K == TorchOps.FID_MAX_K == 8 and KEYS == fc.KEYS


@pytest.mark.parametrize("layout", ["cont", "cat", "small", "intrusion"])
def test_reference_ops_match_brute_force_on_a_table_against_itself(layout):
    n_cont, n_cat = pc.LAYOUTS[layout]
    for k in KS:
        for nr in (k, k + 1, 17, 300):        # nr = k: fewer than k other rows, every radius +inf
            t = pc.random_packed(nr, nr, n_cont, n_cat, seed=nr + k, same=True)
            fc.check_exact(REF, "cpu", *t, (k,), True, f"{layout} self {nr}")
            if nr == k:
                assert np.isinf(fc.run_topk(REF, "cpu", *t, k, True)).all()


@pytest.mark.parametrize("layout", ["cont", "cat", "small", "intrusion"])
@pytest.mark.parametrize("nq,nr", [(1, 1), (7, 3), (300, 257)])
def test_reference_ops_match_brute_force(layout, nq, nr):
    n_cont, n_cat = pc.LAYOUTS[layout]
    fc.check_exact(REF, "cpu", *pc.random_packed(nq, nr, n_cont, n_cat, seed=nq + nr), KS, False, f"{layout} random")
    fc.check_exact(REF, "cpu", *fc.lattice_packed(nq, nr, n_cont, n_cat, seed=nq + nr), KS, False, f"{layout} lattice")


@pytest.mark.parametrize("layout", ["cont", "cat", "small", "intrusion", "wide"])
def test_lattice_dist2_is_dist2(layout):
    n_cont, n_cat = pc.LAYOUTS[layout]
    for same in (False, True):
        t = fc.lattice_packed(40, 70, n_cont, n_cat, seed=n_cont, same=same)
        assert np.array_equal(fc.lattice_dist2(*t), pc.dist2(*t))


def test_reference_ops_work_in_query_blocks():
    t = pc.random_packed(300, 257, 5, 4, seed=9)
    small = TorchOps()
    small.NN_PAIRS = 257 * 64        # five blocks of queries
    for same in (False, True):
        u = (t[2], t[3], t[2], t[3]) if same else t
        assert np.array_equal(fc.run_topk(small, "cpu", *u, 5, same), fc.run_topk(REF, "cpu", *u, 5, same))
    rad = fc.topk(t[2], t[3], t[2], t[3], 5, True)
    for a, b in zip(fc.run_ball(small, "cpu", *t, rad), fc.run_ball(REF, "cpu", *t, rad)):
        assert np.array_equal(a, b)


def test_nan_distance_is_inside_no_ball_and_never_a_minimum():
    q_cont = np.array([[0.0], [np.nan], [0.5]])
    r_cont = np.array([[0.0], [1.0]])
    none = np.zeros((3, 0), dtype=np.int32)
    cnt, dmin = fc.run_ball(REF, "cpu", q_cont, none, r_cont, none[:2], np.array([np.inf, 0.25]))
    assert cnt.tolist() == [1, 0, 2] and dmin.tolist() == [0.0, fc.INF, 0.25]        # <= is inclusive
    got = fc.run_topk(REF, "cpu", q_cont, none, q_cont, none, 1, True)
    assert got.tolist() == [0.25, fc.INF, 0.25]
    with pytest.raises(ValueError, match="k is 1..8"):
        fc.run_topk(REF, "cpu", q_cont, none, q_cont, none, 9, True)


# ----------------------------------------------------------------------------- the evaluator
def _small(n_real=400):
    _, df, _, meta, vocabs, enc, _, _ = pc.small_table()
    enc = np.ascontiguousarray(np.asarray(enc), dtype=np.float64)
    kinds = [pc.CAT if c["type"] == "categorical" else pc.CONT for c in meta["columns"]]
    return df, meta, vocabs, enc, kinds


@pytest.mark.parametrize("k", [1, 5, 8])
def test_evaluator_matches_brute_force_end_to_end(k):
    df, meta, vocabs, enc, kinds = _small()
    fake = enc[900:1200] + 0.0
    fake[::3, [j for j, c in enumerate(kinds) if c == pc.CONT]] *= 1.01       # two thirds stay copies of real rows
    want = fc.expected(enc[:401], fake, kinds, k)
    for real in (df.iloc[:401], enc[:401]):             # a frame and the coded array: the same evaluator
        s = DeviceFidelity(real, meta, vocabs, "cpu", k=k, max_rows=300).score(torch.from_numpy(fake))
        assert isinstance(s, FidelityScores) and s.buf.shape == (8,) and s.buf.dtype == torch.float64
        fc.assert_scores_equal(s.floats(), want, f"small_table k={k}")
        fc.assert_rows_equal(s, want)
    assert all(0.0 <= want[key] <= 1.0 for key in ("precision", "recall", "coverage"))
    assert all(np.isfinite(want[key]) for key in KEYS)


def test_lattice_table_and_the_copy_identity():
    real, fake, kinds = fc.lattice_table(300, 120, seed=1)
    ev = fc.coded_evaluator(real, kinds, k=5, max_rows=300)
    assert (ev.lo == 0).all() and (ev.scale == 1).all()
    s = ev.score(torch.from_numpy(fake))
    want = fc.expected(real, fake, kinds, 5)
    fc.assert_scores_equal(s.floats(), want, "lattice")
    fc.assert_rows_equal(s, want)
    # a row-permuted copy of a continuous real table: everything is reached, and every ball holds its own row's
    # copy and the copies of the k rows its radius was taken from
    g = np.random.default_rng(3)
    real = np.concatenate([g.random((200, 6)), g.integers(0, 4, (200, 3)).astype(np.float64)], axis=1)
    kinds = [pc.CONT] * 6 + [pc.CAT] * 3
    for k in (1, 5, 8):
        f = fc.coded_evaluator(real, kinds, k=k, max_rows=200).score(torch.from_numpy(real[g.permutation(200)]))
        f = f.floats()
        assert (f["precision"], f["recall"], f["coverage"]) == (1.0, 1.0, 1.0) and f["density"] == (k + 1) / k


def test_baseline_keys():
    df, meta, vocabs, enc, kinds = _small()
    fake = torch.from_numpy(enc[500:540] + 0.0)
    on = DeviceFidelity(enc[:101], meta, vocabs, "cpu", k=3, max_rows=40).score(fake).floats()
    off = DeviceFidelity(enc[:101], meta, vocabs, "cpu", k=3, max_rows=40, baseline=False).score(fake).floats()
    assert tuple(on) == tuple(off) == KEYS
    assert [on[key] for key in KEYS[:4]] == [off[key] for key in KEYS[:4]]
    assert all(np.isnan(off[key]) for key in KEYS[4:])
    # the even rows (51) as the real table, the odd rows (50) scored against them, in the whole table's scaling
    want = fc.expected(enc[:101], enc[500:540], kinds, 3)
    assert [on[key] for key in KEYS[4:]] == [want[key] for key in KEYS[4:]]
    assert all(np.isfinite(on[key]) for key in KEYS[4:])
    # an even half of k rows has no k-th neighbour: 2k real rows give NaN, 2k + 1 give numbers
    few = DeviceFidelity(enc[:6], meta, vocabs, "cpu", k=3, max_rows=40).score(fake).floats()
    assert all(np.isnan(few[key]) for key in KEYS[4:]) and np.isfinite(few["precision"])
    more = DeviceFidelity(enc[:7], meta, vocabs, "cpu", k=3, max_rows=40).score(fake).floats()
    fc.assert_scores_equal(more, fc.expected(enc[:7], enc[500:540], kinds, 3), "seven real rows")
    assert all(np.isfinite(more[key]) for key in KEYS[4:])


def test_refusals():
    df, meta, vocabs, enc, _ = _small()
    with pytest.raises(ValueError, match="date"):
        DeviceFidelity(df.iloc[:50], dict(meta, date_info={"when": "%Y"}), vocabs, "cpu")
    cont = next(c["column_name"] for c in meta["columns"] if c["type"] != "categorical")
    for bad in (np.nan, np.inf):
        real = df.iloc[:50].copy()
        real[cont] = real[cont].astype(np.float64)
        real.loc[real.index[7], cont] = bad
        with pytest.raises(ValueError, match=cont):
            DeviceFidelity(real, meta, vocabs, "cpu")
    coded = enc[:50].copy()
    coded[3, [c["column_name"] for c in meta["columns"]].index(cont)] = np.nan
    with pytest.raises(ValueError, match=cont):
        DeviceFidelity(coded, meta, vocabs, "cpu")
    for k in (0, 9):
        with pytest.raises(ValueError, match="k must be in 1..8"):
            DeviceFidelity(enc[:50], meta, vocabs, "cpu", k=k)
    with pytest.raises(ValueError, match="needs at least 6"):
        DeviceFidelity(enc[:5], meta, vocabs, "cpu", k=5)             # M = k
    DeviceFidelity(enc[:6], meta, vocabs, "cpu", k=5)                 # M = k + 1
    ev = DeviceFidelity(enc[:50], meta, vocabs, "cpu", max_rows=10)
    ok = torch.from_numpy(enc[:10] + 0.0)
    with pytest.raises(ValueError, match="expected a float64"):
        ev.score(ok.float())
    with pytest.raises(ValueError, match="buffers hold 1..10"):
        ev.score(torch.cat([ok, ok]))


@pytest.mark.parametrize("n", [1, 5, 6])
def test_few_generated_rows(n):
    """n <= k generated rows have no k-th neighbour: ff = +inf, every real row lies in every generated ball"""
    df, meta, vocabs, enc, kinds = _small()
    ev = DeviceFidelity(enc[:60], meta, vocabs, "cpu", k=5, max_rows=8)
    s = ev.score(torch.from_numpy(enc[700:700 + n] + 0.0))
    want = fc.expected(enc[:60], enc[700:700 + n], kinds, 5)
    fc.assert_scores_equal(s.floats(), want, f"{n} rows")
    fc.assert_rows_equal(s, want)
    if n <= 5:
        assert np.isinf(want["ff"]).all() and bool(torch.isinf(ev.ff[:n]).all())
        assert s.floats()["recall"] == 1.0 and bool(s.real_rows()[1].all())
    else:
        assert np.isfinite(want["ff"]).all()


def test_loaded_generator_write_csv_all_and_sample_cli(tmp_path, capsys):
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

    def fresh():        # (the torch backend draws from torch's global generator)
        torch.manual_seed(11)
        return load_generator(path, torch.device("cpu"), backend="torch", seed=0)

    want = DeviceFidelity(real, meta, vocabs, "cpu", k=3, max_rows=150).score(fresh().device_table(150)).floats()
    gen = fresh()
    got = gen.fidelity(real, n=150, k=3)
    assert got == want and tuple(got) == KEYS
    kept = gen._evaluators["fidelity"][2]
    gen.fidelity(real, n=150, k=3)
    assert gen._evaluators["fidelity"][2] is kept                  # kept per table, n and k
    gen.fidelity(real, n=150, k=4)
    assert gen._evaluators["fidelity"][2] is not kept and gen._evaluators["fidelity"][2].k == 4
    # write_csv_all: the 4-tuple it was without fidelity_real, a fifth element with it
    four = fresh().write_csv_all(out, 150, privacy_real=real)
    assert len(four) == 4 and four[0] is None and four[1] is not None
    five = fresh().write_csv_all(out, 150, privacy_real=real, fidelity_real=real, fidelity_k=3)
    assert len(five) == 5 and five[:4] == four and five[4] == want
    assert len(pd.read_csv(out)) == 150
    # the CLI: one JSON line after all other output, the eight keys and k
    torch.manual_seed(11)
    dtds.sample.main(["-model", path, "-n", "150", "-backend", "torch", "-seed", "0", "-out", out, "-fidelity_against",
                      real_csv, "-fidelity_k", "3"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-2].startswith("150 rows -> ")
    line = json.loads(lines[-1])
    assert tuple(line) == KEYS + ("k",) and line == dict(want, k=3)
    torch.manual_seed(11)
    dtds.sample.main(["-model", path, "-n", "150", "-backend", "torch", "-seed", "0", "-out", out, "-fidelity_against",
                      real_csv, "-fidelity_k", "3", "-privacy_against", real_csv])
    lines = capsys.readouterr().out.strip().splitlines()
    assert json.loads(lines[-1]) == dict(want, k=3) and json.loads(lines[-2]) == four[1]
    assert lines[-3].startswith("150 rows -> ")
    # with -where (and the default k): the scored rows are the conditional request's
    dtds.sample.main(["-model", path, "-n", "60", "-backend", "torch", "-out", out, "-fidelity_against", real_csv,
                      "-privacy_against", real_csv, "-where", "protocol_type=udp"])
    lines = capsys.readouterr().out.strip().splitlines()
    line = json.loads(lines[-1])
    assert tuple(line) == KEYS + ("k",) and line["k"] == 5 and 0.0 <= line["precision"] <= 1.0
    base = DeviceFidelity(real, meta, vocabs, "cpu", k=5, max_rows=1).scores[4:].tolist()
    assert [line[key] for key in KEYS[4:]] == base
    assert tuple(json.loads(lines[-2])) == pc.KEYS and (pd.read_csv(out)["protocol_type"] == "udp").all()
    # with the privacy guard: the guarded rows are the ones scored, and the line is still the last
    dtds.sample.main(["-model", path, "-n", "60", "-backend", "torch", "-out", out, "-fidelity_against", real_csv,
                      "-min_dcr", "0", "-guard_against", real_csv])
    lines = capsys.readouterr().out.strip().splitlines()
    assert "guard min_dcr 0.0" in lines[-2] and tuple(json.loads(lines[-1])) == KEYS + ("k",)
    with pytest.raises(SystemExit):
        dtds.sample.main(["-model", path, "-fidelity_k", "3"])
    with pytest.raises(SystemExit):
        dtds.sample.main(["-model", path, "-fidelity_against", real_csv, "-fidelity_k", "9"])
