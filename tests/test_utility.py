"""The on-device utility evaluator (eval/utility_device.py) on the torch ops (ops/ref.py), on the CPU: against the
plain-numpy brute force of utility_cases.py, its semantics on tables small enough to work out by hand, its optimum
against sklearn's, and the front ends.  Bounds: utility_cases (derived there, W after several steps measured there)."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

import utility_cases as uc
from fed_tgan_amd.eval import DeviceUtility, UtilityScores
from fed_tgan_amd.ops.ref import TorchOps

CONT, CAT, TARGET = uc.CONT, uc.CAT, uc.TARGET
REF = TorchOps()


# ----------------------------------------------------------------------------- 1. against the brute force
@pytest.mark.parametrize("name", list(uc.CASES))
def test_matches_brute_force(name):
    ev, fake, got, want = uc.check_case(REF, "cpu", name)
    s = ev.score(torch.from_numpy(fake))
    assert isinstance(s, UtilityScores) and tuple(s.floats()) == uc.KEYS
    assert s.confusion().dtype == torch.int32 and s.weights().shape == (ev.D, ev.K)


def test_summation_order_spread_is_what_the_bound_was_measured_from():
    """W_TOL = 16 x the largest difference between two summation orders of the reference; two of the cases are
    measured again here so the constant cannot drift from the tables"""
    for name in ("cont33", "absent"):
        train, test, fake, kinds, cards = uc.build_case(name)
        a = uc.expected(train, test, fake, kinds, 20, (5, 20), cards)
        b = uc.expected(train, test, fake, kinds, 20, (5, 20), cards, chunk=uc.CHUNK)
        d = max(float(np.abs(a[s]["W_at"][k] - b[s]["W_at"][k]).max()) for s in ("real", "fake") for k in (5, 20))
        print(f"{name}: whole table against row groups: {d:.3e} (W_SPREAD {uc.W_SPREAD:.3e})")
        assert 0.0 < d <= uc.W_SPREAD


# ----------------------------------------------------------------------------- 2. semantics
def _tiny(train, test, fake, kinds, iters=20, **kw):
    ev = uc.coded_evaluator(np.array(train, dtype=np.float64), np.array(test, dtype=np.float64), kinds, iters=iters,
                            max_rows=len(fake), **kw)
    return ev, ev.score(torch.tensor(fake, dtype=torch.float64))


def test_absent_class_is_never_predicted():
    kinds = [CONT, TARGET]
    real = [[-2.0, 0], [0.0, 1], [2.0, 2], [-2.1, 0], [0.1, 1], [2.1, 2]]
    fake = [[-2.0, 0], [2.0, 2], [-1.9, 0], [1.9, 2]]             # class 1 is missing
    ev, s = _tiny(real, real, fake, kinds)
    conf, W = s.confusion().numpy(), s.weights().numpy()
    assert conf[:, 1].sum() == 0 and conf.sum() == 6 and (W[:, 1] == 0.0).all()
    assert conf[0, 0] == 2 and conf[2, 2] == 2 and conf[1].sum() == 2
    assert ev.conf_real.numpy().trace() == 6


def test_target_overflow_rows_have_weight_zero():
    kinds = [CONT, TARGET]
    real = [[-1.0, 0], [1.0, 1], [-1.2, 0], [1.2, 1]]
    base = [[-1.0, 0], [1.0, 1], [-1.1, 0], [1.1, 1]]
    junk = [[5.0, -1], [-5.0, float("nan")], [9.0, 2], [-9.0, 7.5]]
    ev, a = _tiny(real, real, base, kinds)
    ev2 = uc.coded_evaluator(np.array(real), np.array(real), kinds, iters=20, max_rows=8)
    b = ev2.score(torch.tensor(base + junk, dtype=torch.float64))
    assert ev2.train.s[4:8].tolist() == [0.0] * 4 and ev2.train.y[4:8].tolist() == [2] * 4
    assert ev2.train.info[:3].tolist() == [4.0, 2.0, 4.0] and ev2.train.s[:4].tolist() == [1.0] * 4
    assert torch.equal(a.weights(), b.weights()) and torch.equal(a.buf, b.buf)
    # a test row whose target is no code is skipped
    ev3 = uc.coded_evaluator(np.array(real), np.array(real + [[0.0, 1]]), kinds, iters=5, max_rows=4)
    ev3.test.y[4] = 2
    ev3.score(torch.tensor(base, dtype=torch.float64))
    assert int(ev3.conf.sum()) == 4


def test_overflow_category_is_a_feature_of_its_own():
    kinds = [CAT, TARGET]
    real = [[0, 0], [1, 1], [0, 0], [1, 1]]
    # in the generated table the value 7 (no code of the two categories) goes with class 1, the code 1 with class 0
    fake = [[0, 0], [7, 1], [0, 0], [-3, 1], [float("nan"), 1], [1, 0]]
    ev, s = _tiny(real, real, fake, kinds)
    W = s.weights().numpy()
    assert ev.D == 4 and ev.card_list == [2] and ev.train.cat_t[0, :6].tolist() == [0, 2, 0, 2, 2, 1]
    assert W[2, 1] > W[2, 0] and W[0, 0] > W[0, 1] and W[1, 0] > W[1, 1]
    assert s.confusion().numpy().tolist() == [[2, 0], [2, 0]]         # real code 1 now reads as class 0


def test_constant_continuous_column():
    kinds = [CONT, CONT, TARGET]
    real = [[3.0, -1.0, 0], [3.0, 1.0, 1], [3.0, -1.5, 0], [3.0, 1.5, 1]]
    ev, s = _tiny(real, real, real, kinds)
    assert ev.sd.tolist()[0] == 1.0 and ev.mean.tolist()[0] == 3.0
    assert (ev.train.cont[:4, 0] == 0.0).all() and (s.weights()[0] == 0.0).all()
    f = s.floats()
    assert np.isfinite(list(f.values())).all() and f["acc_fake"] == 1.0 and f["f1_gap"] == 0.0


def test_one_row_training_table():
    kinds = [CONT, CAT, TARGET]
    real = [[0.0, 0, 0], [1.0, 1, 1], [0.2, 0, 0], [0.9, 1, 1]]
    ev, s = _tiny(real, real, [[0.5, 1, 1]], kinds)
    f = s.floats()
    assert ev.train.info[:3].tolist() == [1.0, 1.0, 1.0] and np.isfinite(list(f.values())).all()
    assert s.confusion().numpy().tolist() == [[0, 2], [0, 2]] and f["acc_fake"] == 0.5
    assert (s.weights() == 0.0).all() and f["loss_fake"] == 0.0 and f["grad_fake"] == 0.0
    # and no valid row at all: nothing is present, class 0 is predicted
    s = ev.score(torch.tensor([[0.5, 1, -1]], dtype=torch.float64))
    assert s.confusion().numpy().tolist() == [[2, 0], [2, 0]] and bool(torch.isfinite(s.buf).all())


def test_single_class():
    kinds = [CONT, TARGET]
    real = [[0.0, 0], [1.0, 0], [2.0, 0]]
    ev, s = _tiny(real, real, real, kinds)
    f = s.floats()
    assert ev.K == 1 and (s.weights() == 0.0).all() and s.confusion().numpy().tolist() == [[3]]
    assert f["f1_fake"] == 1.0 and f["acc_fake"] == 1.0 and f["loss_fake"] == 0.0 and f["f1_gap"] == 0.0


def test_no_continuous_and_no_categorical_features():
    g = np.random.default_rng(0)
    y = g.integers(0, 2, 60)
    cats = np.stack([np.where(g.random(60) < 0.8, y, 1 - y), g.integers(0, 3, 60), y], axis=1).astype(np.float64)
    ev, s = _tiny(cats, cats, cats, [CAT, CAT, TARGET])
    assert ev.n_cont == 0 and ev.D == 3 + 4 + 1 and s.floats()["acc_fake"] >= 0.7
    conts = np.stack([y + 0.3 * g.normal(size=60), g.normal(size=60), y], axis=1)
    ev, s = _tiny(conts, conts, conts, [CONT, CONT, TARGET])
    assert ev.n_cat == 0 and ev.D == 3 and s.floats()["acc_fake"] >= 0.9 and s.floats()["f1_gap"] == 0.0


def test_ties_go_to_the_lowest_class():
    kinds = [CONT, TARGET]
    real = [[-1.0, 0], [1.0, 1], [-1.0, 2], [1.0, 1]]
    # iters = 0: W = 0, every logit ties, class 0 wins; with class 0 absent from the generated table, class 1 does
    ev, s = _tiny(real, real, real, kinds, iters=0)
    assert s.confusion().numpy().tolist() == [[1, 0, 0], [2, 0, 0], [1, 0, 0]]
    s = ev.score(torch.tensor([[0.0, 1], [0.0, 2]], dtype=torch.float64))
    assert s.confusion().numpy().tolist() == [[0, 1, 0], [0, 2, 0], [0, 1, 0]]


def test_refusals_name_the_columns():
    _, df, _, meta, vocabs, _, _, _ = uc.small_table()
    a, b = df.iloc[:80], df.iloc[80:120]
    cont_name = next(c["column_name"] for c in meta["columns"] if c["type"] != "categorical")
    with pytest.raises(ValueError, match=f"target '{cont_name}'.*regression"):
        DeviceUtility(a, b, meta, vocabs, "cpu", target=cont_name)
    with pytest.raises(ValueError, match="date columns"):
        DeviceUtility(a, b, dict(meta, date_info={"when": "%Y"}), vocabs, "cpu")
    bad = a.copy()
    bad[cont_name] = bad[cont_name].astype(np.float64)
    bad.loc[bad.index[3], cont_name] = float("inf")
    with pytest.raises(ValueError, match=cont_name):
        DeviceUtility(bad, b, meta, vocabs, "cpu")
    kinds = [CAT, CONT, CAT, TARGET]
    real = np.zeros((10, 4))
    real[0, 0], real[0, 2] = 599.0, 699.0
    with pytest.raises(ValueError, match=r"UTIL_MAX_FEATURES = 1024.*'c2' \(700\).*'c0' \(600\)"):
        uc.coded_evaluator(real, real, kinds)
    real = np.zeros((10, 4))
    real[0, 3], real[0, 0] = float(REF.UTIL_MAX_CLASSES), 4.0
    with pytest.raises(ValueError, match=r"65 classes of the target 'c3'.*UTIL_MAX_CLASSES = 64.*'c0' \(5\)"):
        uc.coded_evaluator(real, real, kinds)
    ev = uc.coded_evaluator(np.zeros((4, 4)), np.zeros((4, 4)), kinds, iters=1, max_rows=5)
    with pytest.raises(ValueError, match="expected a float64"):
        ev.score(torch.zeros(3, 4))
    with pytest.raises(ValueError, match=r"hold 1\.\.5"):
        ev.score(torch.zeros(6, 4, dtype=torch.float64))


# ----------------------------------------------------------------------------- 3. the optimum is sklearn's
def test_optimum_is_sklearns():
    """share of test rows left out as sklearn's own near-ties (top-two probability gap <= 1e-6): 0 of 200 with this
    seed"""
    from sklearn.linear_model import LogisticRegression
    kinds = [CONT, CONT, CAT, CONT, CAT, CONT, TARGET]
    cards, K = [3, 4], 3
    train = uc.random_table(600, kinds, 21, cards, K, sep=0.8)
    test = uc.random_table(200, kinds, 22, cards, K, sep=0.8)
    ev = uc.coded_evaluator(train, test, kinds, iters=1000, max_rows=600)
    s = ev.score(torch.from_numpy(train))
    f = s.floats()
    print(f)
    assert f["grad_fake"] < 1e-8
    fc, K_, mean, sd = uc.setup(train, test, kinds)
    F, y = uc.features(train, kinds, fc, K_, mean, sd)
    Ft, yt = uc.features(test, kinds, fc, K_, mean, sd)
    # sklearn adds an unpenalised intercept of its own; the constant column of F is then penalised to 0 and the
    # optimum's logits are the contract's, whose intercept row is unpenalised
    lr = LogisticRegression(C=1.0, class_weight="balanced", tol=1e-10, max_iter=10000)
    lr.fit(F, y)
    prob = np.sort(lr.predict_proba(Ft), axis=1)
    sure = prob[:, -1] - prob[:, -2] > 1e-6
    left_out = 1.0 - sure.mean()
    print(f"left out: {left_out:.4f}")
    assert left_out <= 0.02
    pred, _ = uc.predict(Ft, s.weights().numpy(), np.ones(K, dtype=bool))
    assert np.array_equal(pred[sure], lr.predict(Ft)[sure])
    assert np.array_equal(s.confusion().numpy(), uc.confusion(yt, pred, K))


# ----------------------------------------------------------------------------- 4. front ends
def test_copy_of_the_training_rows_has_no_gap():
    _, df, _, meta, vocabs, enc, _, _ = uc.small_table()
    from fed_tgan_amd.eval.privacy import code_real_table
    train, test = df.iloc[:500], df.iloc[500:700]
    ev = DeviceUtility(train, test, meta, vocabs, "cpu", iters=15, max_rows=600)
    f = ev.score(torch.from_numpy(code_real_table(train, meta, vocabs))).floats()
    assert f["f1_gap"] == 0.0 and f["acc_gap"] == 0.0 and f["f1_fake"] == f["f1_real"] > 0.5
    assert ev.target == meta["target"] and ev.K == len(vocabs[[c["column_name"] for c in meta["columns"]
                                                                 if c["type"] == "categorical"].index(ev.target)])


def test_loaded_generator_and_sample_cli(tmp_path, capsys):
    import dtds.sample
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.generator_io import export_generator, load_generator
    from fed_tgan_amd.models.samplers import CondTables
    _, df, _, meta, vocabs, _, tr, X = uc.small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), "cpu", backend="torch", seed=5)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    path, real_csv, out = str(tmp_path / "g.pt"), str(tmp_path / "real.csv"), str(tmp_path / "s.csv")
    test_csv = str(tmp_path / "test.csv")
    export_generator(path, eng, tr, CondTables.from_encoded(X, tr.layout), meta, vocabs, "Intrusion")
    df.iloc[:400].to_csv(real_csv, index=False)
    df.iloc[400:500].to_csv(test_csv, index=False)
    real, test = pd.read_csv(real_csv), pd.read_csv(test_csv)
    gen = load_generator(path, torch.device("cpu"), backend="torch", seed=0)
    # the default hold-out: rows with index % 5 == 4
    held = np.arange(len(real)) % 5 == 4
    torch.manual_seed(11)
    want = DeviceUtility(real[~held], real[held], meta, vocabs, "cpu", iters=10, max_rows=150).score(
        gen.device_table(150)).floats()
    torch.manual_seed(11)
    got = load_generator(path, torch.device("cpu"), backend="torch", seed=0).utility(real, n=150, iters=10)
    assert got == want and tuple(got) == uc.KEYS and 0.0 < want["f1_real"] <= 1.0
    # with a test table
    torch.manual_seed(11)
    want_t = DeviceUtility(real, test, meta, vocabs, "cpu", iters=10, max_rows=150).score(
        gen.device_table(150)).floats()
    torch.manual_seed(11)
    assert load_generator(path, torch.device("cpu"), backend="torch", seed=0).utility(real, test, n=150,
                                                                                       iters=10) == want_t
    # all four evaluators on one table
    torch.manual_seed(11)
    res = load_generator(path, torch.device("cpu"), backend="torch", seed=0).write_csv_all(
        out, 150, score_real=real, privacy_real=real, corr_real=real, utility_real=real, utility_iters=10)
    assert len(res) == 4 and res[3] == want and len(res[0]) == 2 and "dcr_p5" in res[1] and "corr_diff" in res[2]
    # the command line: the utility line comes after all other output
    torch.manual_seed(11)
    dtds.sample.main(["-model", path, "-n", "150", "-backend", "torch", "-seed", "0", "-out", out, "-utility_against",
                      real_csv, "-utility_iters", "10", "-corr_against", real_csv, "-privacy_against", real_csv,
                      "-score_against", real_csv])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-5].startswith("150 rows -> ") and lines[-4].startswith("Avg_JSD ")
    assert "dcr_p5" in json.loads(lines[-3]) and "corr_diff" in json.loads(lines[-2])
    assert json.loads(lines[-1]) == want and len(pd.read_csv(out)) == 150
    torch.manual_seed(11)
    dtds.sample.main(["-model", path, "-n", "150", "-backend", "torch", "-seed", "0", "-out", out, "-utility_against",
                      real_csv, "-utility_test", test_csv, "-utility_iters", "10"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-2].startswith("150 rows -> ") and json.loads(lines[-1]) == want_t
    # with -where: the fitted rows are the conditional request's
    dtds.sample.main(["-model", path, "-n", "60", "-backend", "torch", "-out", out, "-utility_against", real_csv,
                      "-utility_iters", "10", "-where", "protocol_type=udp"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert tuple(line) == uc.KEYS and line["f1_real"] == want["f1_real"]
    # without the flag nothing new is printed, and write_csv_evaluated keeps its two-tuple
    dtds.sample.main(["-model", path, "-n", "20", "-backend", "torch", "-out", out])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("20 rows -> ")
    assert len(gen.write_csv_evaluated(out, 30, privacy_real=real)) == 2
