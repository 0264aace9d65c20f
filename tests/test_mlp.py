"""The MLP-utility evaluator (fed_tgan_amd/eval/mlp_device.py) through the reference ops on the CPU: every case of
mlp_cases.py against the plain-numpy brute force, op by op and end to end (bounds: mlp_cases), the refusals, the
determinism of the initial weights and the front ends.  tests/test_hip_mlp.py runs the same cases through the HIP
kernels."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

import mlp_cases as mc
import utility_cases as uc
from fed_tgan_amd.eval import DeviceMLP, MLPScores
from fed_tgan_amd.eval.forest_device import KEYS as TREE_KEYS
from fed_tgan_amd.eval.mlp_device import KEYS
from fed_tgan_amd.eval.utility_device import KEYS as LR_KEYS
from fed_tgan_amd.ops.ref import TorchOps
from utility_cases import CAT, CONT, TARGET

REF = TorchOps()


# ----------------------------------------------------------------------------- 1. the cases
@pytest.mark.parametrize("name", list(mc.CASES))
def test_matches_brute_force(name):
    ev, fake, got, want = mc.check_case(REF, "cpu", name)
    s = ev.score(torch.from_numpy(fake))
    assert isinstance(s, MLPScores) and tuple(s.floats()) == KEYS == mc.KEYS
    W1, W2 = s.weights()
    assert W1.shape == (ev.D, ev.hidden) and W2.shape == (ev.hidden + 1, ev.K)


def test_cases_are_the_shapes_they_claim():
    c = mc.CASES
    assert [c[f"rows{n}"]["n"] for n in (1, 63, 64, 65, 131)] == [1, 63, 64, 65, 131] and c["rows65"]["batch"] == 64
    assert mc.batch_rows(131, 64, 0).tolist() == list(range(0, 131, 3)) and len(mc.batch_rows(131, 64, 2)) == 43
    assert (c["batch512"]["n"], c["batch512"]["batch"]) == (700, 512) and c["batch1"]["batch"] == 1
    want = mc.case_expected("wide")[5]
    assert want["fake"]["F"].shape == (50, REF.UTIL_MAX_FEATURES - 1) and c["wide"]["H"] == REF.MLP_MAX_HIDDEN
    assert max(v["K"] for v in c.values()) == REF.UTIL_MAX_CLASSES
    f = mc.case_expected("novalid")[5]["fake"]
    assert (f["y"][mc.batch_rows(131, 64, 1)] == 3).all() and (f["y"][mc.batch_rows(131, 64, 0)] < 3).all()
    f = mc.case_expected("absent")[5]["fake"]
    assert not f["present"].all() and (f["y"] == 4).any()


def test_summation_order_spread_is_what_the_bound_was_measured_from():
    """THETA_TOL = 16 x the largest difference between two summation orders of the reference; the two cases whose
    batches hold several row blocks are measured again here so the constant cannot drift from the tables"""
    tops = {}
    for name in ("batch512", "wide512"):
        train, test, fake, kinds, cardinalities, whole = mc.case_expected(name)
        c = mc.CASES[name]
        blocked = mc.expected(train, test, fake, kinds, c["H"], c["batch"], 20, (5, 20), cardinalities, block=mc.BLOCK)
        tops[name] = max(float(np.abs(whole[s]["theta_at"][k] - blocked[s]["theta_at"][k]).max())
                         for s in ("real", "fake") for k in (5, 20))
        print(f"spread of {name}: {tops[name]:.3e}")
    assert 0.0 < tops["batch512"] <= tops["wide512"] <= mc.THETA_SPREAD <= 2 * tops["wide512"]
    assert mc.THETA_TOL == 16 * mc.THETA_SPREAD


# ----------------------------------------------------------------------------- 2. properties
def _tiny(real, test, fake, kinds, **kw):
    ev = mc.coded_evaluator(np.asarray(real, dtype=np.float64), np.asarray(test, dtype=np.float64), kinds,
                            max_rows=len(fake), **kw)
    return ev, ev.score(torch.tensor(fake, dtype=torch.float64))


def test_zero_steps_scores_theta0():
    train, test, fake, kinds, cardinalities, _ = mc.case_expected("rows131")
    ev = mc.coded_evaluator(train, test, kinds, hidden=17, batch=64, steps=0, max_rows=len(fake),
                            cardinalities=cardinalities)
    s = ev.score(torch.from_numpy(fake))
    W1, W2 = s.weights()
    assert torch.equal(torch.cat([W1.reshape(-1), W2.reshape(-1)]), ev.theta0)
    want = mc.expected(train, test, fake, kinds, 17, 64, 0, (), cardinalities)
    assert np.array_equal(ev.theta0.numpy(), want["fake"]["theta0"])
    assert np.array_equal(s.confusion().numpy(), want["fake"]["conf"])
    f = s.floats()
    assert abs(f["mlp_loss_fake"] - want["fake"]["loss"]) <= 2 * mc.gamma(131 + 17 + 3) * want["fake"]["loss"]
    assert f["mlp_f1_fake"] == f["mlp_f1_real"] and f["mlp_f1_gap"] == 0.0


def test_same_seed_same_bits_other_seed_differs():
    train, test, fake, kinds, cardinalities, _ = mc.case_expected("rows131")
    kw = dict(hidden=17, batch=64, steps=5, max_rows=len(fake), cardinalities=cardinalities)
    a = mc.coded_evaluator(train, test, kinds, seed=3, **kw)
    b = mc.coded_evaluator(train, test, kinds, seed=3, **kw)
    c = mc.coded_evaluator(train, test, kinds, seed=4, **kw)
    assert torch.equal(a.theta0, b.theta0) and not torch.equal(a.theta0, c.theta0)
    t = torch.from_numpy(fake)
    sa, sb, sc = a.score(t), b.score(t), c.score(t)
    assert torch.equal(sa.buf.view(torch.int64), sb.buf.view(torch.int64))
    assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(sa.weights(), sb.weights()))
    assert not torch.equal(sa.weights()[0], sc.weights()[0])
    assert torch.equal(a.score(t).buf.view(torch.int64), sa.buf.view(torch.int64))      # a second run


def test_glorot_bounds_and_draw_order():
    D, H, K = 15, 17, 3
    train, test, fake, kinds, cardinalities, _ = mc.case_expected("rows131")
    ev = mc.coded_evaluator(train, test, kinds, hidden=H, batch=64, steps=0, max_rows=5, cardinalities=cardinalities)
    th = ev.theta0.numpy()
    b1, b2 = np.sqrt(6.0 / (D - 1 + H)), np.sqrt(6.0 / (H + K))
    g = np.random.default_rng(0)
    first = g.uniform(-b1, b1, (D - 1, H))
    assert ev.D == D and np.array_equal(th[:(D - 1) * H], first.reshape(-1))
    assert np.abs(th[:D * H]).max() <= b1 < np.abs(th[D * H:]).max() <= b2


def test_absent_class_is_never_predicted():
    kinds = [CONT, TARGET]
    real = [[-2.0, 0], [0.0, 1], [2.0, 2], [-2.1, 0], [0.1, 1], [2.1, 2]]
    fake = [[-2.0, 0], [2.0, 2], [-1.9, 0], [1.9, 2]]             # class 1 is missing
    ev, s = _tiny(real, real, fake, kinds, hidden=8, steps=50, batch=4)
    conf = s.confusion().numpy()
    assert conf[:, 1].sum() == 0 and conf.sum() == 6


def test_no_valid_row_at_all_is_weight_decay_alone():
    """a generated table without one valid target: m = 1, the gradient is alpha theta on the weights and 0 on the
    biases, class 0 is predicted"""
    kinds = [CONT, TARGET]
    real = [[-1.0, 0], [1.0, 1], [-1.2, 0], [1.2, 1]]
    fake = [[0.5, -1.0], [0.2, float("nan")], [0.1, 7.0]]
    ev, s = _tiny(real, real, fake, kinds, hidden=4, steps=1, batch=2)
    W1, W2 = s.weights()
    D, H, K = ev.D, 4, ev.K
    t0 = ev.theta0
    assert torch.equal(W1[D - 1], t0[:D * H].view(D, H)[D - 1]) and torch.equal(W2[H], t0[D * H:].view(H + 1, K)[H])
    assert not torch.equal(W1[0], t0[:H])
    assert s.confusion().numpy()[:, 1:].sum() == 0


def test_refusals_name_the_limits():
    _, df, _, meta, vocabs, _, _, _ = uc.small_table()
    a, b = df.iloc[:80], df.iloc[80:120]
    cont_name = next(c["column_name"] for c in meta["columns"] if c["type"] != "categorical")
    with pytest.raises(ValueError, match=f"target '{cont_name}'.*regression"):
        DeviceMLP(a, b, meta, vocabs, "cpu", target=cont_name)
    with pytest.raises(ValueError, match="DeviceMLP: the table has date columns"):
        DeviceMLP(a, b, dict(meta, date_info={"when": "%Y"}), vocabs, "cpu")
    bad = a.copy()
    bad[cont_name] = bad[cont_name].astype(np.float64)
    bad.loc[bad.index[3], cont_name] = float("inf")
    with pytest.raises(ValueError, match=f"the real column '{cont_name}' holds a value that is not a finite number"):
        DeviceMLP(bad, b, meta, vocabs, "cpu")
    coded = np.zeros((6, 2))
    coded[2, 0] = float("nan")
    with pytest.raises(ValueError, match="DeviceMLP: the real column 'c0' holds a value that is not a finite number"):
        mc.coded_evaluator(coded, np.zeros((3, 2)), [CONT, TARGET])
    with pytest.raises(ValueError, match=r"hidden 129 is outside 1 \.\. MLP_MAX_HIDDEN = 128"):
        DeviceMLP(a, b, meta, vocabs, "cpu", hidden=129)
    with pytest.raises(ValueError, match=r"hidden 0 is outside"):
        DeviceMLP(a, b, meta, vocabs, "cpu", hidden=0)
    with pytest.raises(ValueError, match=r"batch 1025 is outside 1 \.\. MLP_MAX_BATCH = 1024"):
        DeviceMLP(a, b, meta, vocabs, "cpu", batch=1025)
    with pytest.raises(ValueError, match=r"steps 10001 is outside 0 \.\. MLP_MAX_STEPS = 10000"):
        DeviceMLP(a, b, meta, vocabs, "cpu", steps=10001)
    kinds = [CAT, CONT, CAT, TARGET]
    real = np.zeros((10, 4))
    real[0, 0], real[0, 2] = 599.0, 699.0
    with pytest.raises(ValueError, match=r"DeviceMLP: .*UTIL_MAX_FEATURES = 1024.*'c2' \(700\).*'c0' \(600\)"):
        mc.coded_evaluator(real, real, kinds)
    real = np.zeros((10, 4))
    real[0, 3], real[0, 0] = float(REF.UTIL_MAX_CLASSES), 4.0
    with pytest.raises(ValueError, match=r"65 classes of the target 'c3'.*UTIL_MAX_CLASSES = 64.*'c0' \(5\)"):
        mc.coded_evaluator(real, real, kinds)
    ev = mc.coded_evaluator(np.zeros((4, 4)), np.zeros((4, 4)), kinds, steps=1, max_rows=5)
    with pytest.raises(ValueError, match="expected a float64"):
        ev.score(torch.zeros(3, 4))
    with pytest.raises(ValueError, match=r"hold 1\.\.5"):
        ev.score(torch.zeros(6, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="MLP_MAX_BATCH"):
        REF.mlp_step(ev.train, 5, 3, 2, ev.theta, ev.m, ev.v, ev.h, ev.dz, ev.dh, ev.cnt, ev.hidden, 0.0, 1e-3)


def test_limits_are_the_contracts():
    assert (REF.MLP_MAX_HIDDEN, REF.MLP_MAX_BATCH, REF.MLP_MAX_STEPS, REF.MLP_ROWS) == (128, 1024, 10000, mc.BLOCK)


# ----------------------------------------------------------------------------- 3. sanity and the front ends
def test_defaults_learn_the_small_table():
    _, df, _, meta, vocabs, _, _, _ = uc.small_table()
    from fed_tgan_amd.eval.privacy import code_real_table
    train, test = df.iloc[:500], df.iloc[500:700]
    ev = DeviceMLP(train, test, meta, vocabs, "cpu", max_rows=500)
    assert (ev.hidden, ev.steps, ev.batch, ev.lr, ev.alpha, ev.seed) == (100, 1000, 512, 1e-3, 1e-4, 0)
    f = ev.score(torch.from_numpy(code_real_table(train, meta, vocabs))).floats()
    print(f)
    assert f["mlp_f1_real"] > 0.5
    assert f["mlp_f1_gap"] == 0.0 and f["mlp_acc_gap"] == 0.0          # the same rows, the same bits


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
    kw = dict(hidden=9, steps=6, batch=50)

    def fresh():
        torch.manual_seed(11)
        return load_generator(path, torch.device("cpu"), backend="torch", seed=0)

    gen = fresh()
    held = np.arange(len(real)) % 5 == 4                          # the default hold-out: rows with index % 5 == 4
    want = DeviceMLP(real[~held], real[held], meta, vocabs, "cpu", max_rows=150, **kw).score(
        gen.device_table(150)).floats()
    got = fresh().mlp_utility(real, n=150, **kw)
    assert got == want and tuple(got) == KEYS and 0.0 <= want["mlp_f1_real"] <= 1.0
    gen = fresh()
    want_t = DeviceMLP(real, test, meta, vocabs, "cpu", max_rows=150, seed=2, **kw).score(
        gen.device_table(150)).floats()
    g2 = fresh()
    assert g2.mlp_utility(real, test, n=150, seed=2, **kw) == want_t != want
    assert g2._mlp_evaluator(real, test, 150, 9, 6, 50, 2) is g2._mlp_evaluator(real, test, 150, 9, 6, 50, 2)    # cached
    assert g2._mlp_evaluator(real, test, 150, 9, 6, 50, 2) is not g2._mlp_evaluator(real, test, 150, 9, 7, 50, 2)
    # write_csv_all: the default is today's dict, the models add their keys to it in the order lr, dt / rf, mlp
    ukw = dict(utility_hidden=9, utility_steps=6, utility_batch=50)
    res = fresh().write_csv_all(out, 150, utility_real=real, utility_iters=10)
    assert len(res) == 4 and tuple(res[3]) == LR_KEYS
    same = fresh().write_csv_all(out, 150, utility_real=real, utility_iters=10, **ukw)
    assert same[3] == res[3]
    every = fresh().write_csv_all(out, 150, utility_real=real, utility_iters=10, utility_trees=3, utility_depth=5,
                                  utility_models=("mlp", "rf", "lr", "dt"), **ukw)[3]
    assert tuple(every) == LR_KEYS + TREE_KEYS + KEYS and {k: every[k] for k in LR_KEYS} == res[3]
    assert {k: every[k] for k in KEYS} == want
    only = fresh().write_csv_all(out, 150, utility_real=real, utility_models=("mlp",), **ukw)[3]
    assert only == want and tuple(only) == KEYS
    with pytest.raises(ValueError, match="'mlp'.*svm"):
        fresh().write_csv_all(out, 20, utility_real=real, utility_models=("svm",))
    # the command line
    base = ["-model", path, "-n", "150", "-backend", "torch", "-seed", "0", "-out", out]
    mlp_args = ["-utility_hidden", "9", "-utility_steps", "6", "-utility_batch", "50"]
    torch.manual_seed(11)
    dtds.sample.main(base + ["-utility_against", real_csv, "-utility_iters", "10", "-utility_models", "lr,mlp"]
                     + mlp_args)
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-2].startswith("150 rows -> ") and len(pd.read_csv(out)) == 150
    assert json.loads(lines[-1]) == dict(res[3], **want) and tuple(json.loads(lines[-1])) == LR_KEYS + KEYS
    torch.manual_seed(11)
    dtds.sample.main(base + ["-utility_against", real_csv, "-utility_iters", "10"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res[3]
    with pytest.raises(SystemExit):
        dtds.sample.main(base + ["-utility_against", real_csv, "-utility_models", "svm"])
    with pytest.raises(SystemExit):
        dtds.sample.main(base + ["-utility_models", "mlp"])
    for flag in ("-utility_hidden", "-utility_steps", "-utility_batch"):
        with pytest.raises(SystemExit):
            dtds.sample.main(base + [flag, "7"])
    capsys.readouterr()
