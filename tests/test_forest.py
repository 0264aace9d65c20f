"""The tree-utility evaluator (fed_tgan_amd/eval/forest_device.py) through the reference ops on the CPU: every case of
forest_cases.py against the brute force (equalities), the properties the cases were built for, the criterion against
sklearn's, the refusals and the front ends.  tests/test_hip_forest.py runs the same cases through the HIP kernels."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

import forest_cases as fc
from fed_tgan_amd.eval import DeviceForest
from fed_tgan_amd.eval.forest_device import KEYS
from fed_tgan_amd.eval.utility_device import KEYS as LR_KEYS
from fed_tgan_amd.ops.ref import TorchOps
from utility_cases import CAT, CONT, TARGET

REF = TorchOps()


# ----------------------------------------------------------------------------- 1. Philox, restated twice
def test_philox_known_answer_and_torch_restatement():
    assert fc.philox_word(0, 0, 0, 0, 0) == 0x6627E8D5          # Random123's known answer for a zero counter and key
    seed = (0xDEADBEEF << 32) | 0x12345678
    lo = torch.arange(50, dtype=torch.int64)
    got = REF.tree_word(seed, fc.STREAM_FEAT, 77, 3, lo).tolist()
    assert got == [fc.philox_word(seed, fc.STREAM_FEAT, 77, 3, j) for j in range(50)]
    assert (REF.TREE_STREAM_DRAW, REF.TREE_STREAM_FEAT) == (fc.STREAM_DRAW, fc.STREAM_FEAT)


# ----------------------------------------------------------------------------- 2. the cases
@pytest.mark.parametrize("name", fc.CASES)
def test_cases_match_brute_force(name):
    fc.check_case(REF, "cpu", name)


def _tree(name, model="dt", t=0, side="fake"):
    return fc.expected_case(name)[1][side][model]["trees"][t]


def test_cases_show_what_they_were_built_for():
    """the brute force's own results (the ops equal them, test above)"""
    assert len(_tree("one_class")["heap"]) == 1 and len(_tree("no_valid")["heap"]) == 1
    assert _tree("no_valid")["counts"].sum() == 0
    c, want = fc.expected_case("no_valid")
    assert (want["fake"]["dt"]["conf"][:, 1:] == 0).all()            # an empty tree predicts class 0
    c, want = fc.expected_case("absent")
    for m in ("dt", "rf"):                                           # an absent class is never predicted
        assert (want["fake"][m]["conf"][:, [0, 2, 4]] == 0).all() and want["fake"][m]["conf"].sum() > 0
    assert want["fake"]["counts"][0] == want["fake"]["counts"][2] == 0
    c, want = fc.expected_case("constant")
    j = [k for k in c["kinds"] if k != TARGET].index(CONT)
    assert want["nbins"][j] == 1 and all(j not in tr["feature"].tolist() for tr in want["fake"]["rf"]["trees"])
    assert 2 in fc.expected_case("two_bins")[1]["nbins"]
    assert 256 in fc.expected_case("cont256")[1]["nbins"] and 256 in fc.expected_case("cat255")[1]["nbins"]
    c, want = fc.expected_case("cont400")
    assert max(len(np.unique(np.concatenate([c["train"], c["test"]])[:, j])) for j, k in enumerate(c["kinds"])
               if k == CONT) > 256 and max(want["nbins"]) == 256
    assert len(_tree("depth0")["heap"]) == 1 and len(_tree("depth1")["heap"]) == 3
    # the chain: end splits, so the depth limit is reached with impure leaves, and a deep enough tree fits its rows
    short, full = _tree("chain_short"), _tree("chain_full")
    assert short["heap"].max() >= 2 ** 3 and any((row > 0).sum() > 1 for row, f in zip(short["counts"], short["feature"])
                                                 if f < 0)
    want = fc.expected_case("chain_full")[1]
    assert want["fake"]["dt"]["scores"] == (1.0, 1.0) and all((row > 0).sum() == 1 for row, f in
                                                               zip(full["counts"], full["feature"]) if f < 0)
    c, _ = fc.expected_case("chain_full")
    assert c["p"]["max_depth"] >= np.log2(len(c["fake"]))
    # ties
    c, _ = fc.expected_case("twins")
    a, b = [f for f, k in enumerate(k for k in c["kinds"] if k != TARGET) if k == CONT]
    assert b not in _tree("twins")["feature"].tolist() and a in _tree("twins")["feature"].tolist()
    assert _tree("symmetric")["feature"][0] == 0 and _tree("symmetric")["bin"][0] == 0
    want = fc.expected_case("equal_masses")[1]
    assert (want["fake"]["dt"]["conf"][:, 1] == 0).all() and want["fake"]["dt"]["conf"].sum() == 8
    want = fc.expected_case("soft_tie")[1]
    assert (want["fake"]["rf"]["conf"][:, 1] == 0).all() and want["fake"]["rf"]["conf"].sum() == 2
    # min_leaf: every leaf holds at least three rows
    for tr in [_tree("min_leaf3")] + fc.expected_case("min_leaf3")[1]["fake"]["rf"]["trees"]:
        assert tr["counts"].sum(axis=1).min() >= 3 and (tr["feature"] >= 0).any()
    # XOR: no split improves the score, yet the tree splits and fits
    x = _tree("xor")
    assert len(x["heap"]) == 7 and fc.expected_case("xor")[1]["fake"]["dt"]["scores"] == (1.0, 1.0)
    w = fc.expected_case("xor")[1]["fake"]["w"]
    root = fc.side_term(x["counts"][0], w)
    assert fc.side_term(x["counts"][1], w) + fc.side_term(x["counts"][2], w) == root


def test_one_tree_without_bootstrap_is_the_decision_tree():
    c, want = fc.expected_case("rows257")
    ev = fc.case_evaluator(c, "cpu", REF)
    n = len(c["fake"])
    from fed_tgan_amd.eval.forest_device import TreeModel, TreeTable
    tab = TreeTable(n, ev.card, ev.edges, ev.eoff, ev.nbins, ev.max_bins, ev.K, "cpu")
    REF.tree_pack(torch.from_numpy(c["fake"]), ev.kind, ev.slot, tab)
    model = TreeModel(1, n, ev.K, ev.max_depth, "cpu")
    REF.tree_bootstrap(model.mult, n, False, ev.seed)
    REF.tree_grow(tab, n, model, ev.max_depth, ev.min_leaf, ev.F, ev.seed + 99)     # (no key is drawn: any seed)
    arrays = {k: getattr(model, k).numpy() for k in ("feature", "bin", "left", "heap", "counts")}
    fc.assert_trees(arrays, want["fake"]["dt"]["trees"], "forest of one")
    for T in (3, 5):
        model = TreeModel(T, n, ev.K, ev.max_depth, "cpu")
        REF.tree_bootstrap(model.mult, n, True, 7)
        assert model.mult.sum(dim=1).tolist() == [n] * T and not torch.equal(model.mult[0], model.mult[1])


# ----------------------------------------------------------------------------- 3. refusals
def test_refusals_name_their_columns_and_numbers():
    _, df, _, meta, vocabs, enc, _, _ = fc.small_table()
    a, b = df.iloc[:300], df.iloc[300:400]
    with pytest.raises(ValueError, match="date columns"):
        DeviceForest(a, b, dict(meta, date_info={"d": "%Y"}), vocabs, "cpu")
    cont_name = next(c["column_name"] for c in meta["columns"] if c["type"] != "categorical")
    with pytest.raises(ValueError, match=f"{cont_name!r} is not a categorical column"):
        DeviceForest(a, b, meta, vocabs, "cpu", target=cont_name)
    kinds = [CAT, CONT, CAT, TARGET]
    real = np.zeros((10, 4))
    real[0, 0], real[0, 2] = 299.0, 279.0
    with pytest.raises(ValueError, match=r"301 bins.*TREE_MAX_BINS = 256.*'c0' \(300\).*'c2' \(280\)"):
        fc.coded_evaluator(real, real, kinds)
    real = np.zeros((10, 4))
    real[0, 3], real[0, 0] = float(REF.TREE_MAX_CLASSES), 4.0
    with pytest.raises(ValueError, match=r"65 classes of the target 'c3'.*TREE_MAX_CLASSES = 64.*'c0' \(5\)"):
        fc.coded_evaluator(real, real, kinds)
    real = np.zeros((10, 4))
    with pytest.raises(ValueError, match=r"40000 rows, 100 trees of up to 79999 nodes \(max_depth 20\).*"
                                         r"more than max_scratch_bytes = 268435456"):
        fc.coded_evaluator(real, real, kinds, max_depth=20)
    with pytest.raises(ValueError, match=r"TREE_MAX_DEPTH = 20"):
        fc.coded_evaluator(real, real, kinds, max_depth=21)
    bad = real.copy()
    bad[3, 1] = float("inf")
    with pytest.raises(ValueError, match="'c1' holds a value that is not a finite number"):
        fc.coded_evaluator(bad, real, kinds)
    ev = fc.coded_evaluator(real, real, kinds, trees=2, max_depth=2, max_rows=5)
    with pytest.raises(ValueError, match="expected a float64"):
        ev.score(torch.zeros(3, 4))
    with pytest.raises(ValueError, match=r"hold 1\.\.5"):
        ev.score(torch.zeros(6, 4, dtype=torch.float64))


# ----------------------------------------------------------------------------- 4. against sklearn
def _gini_mass(m):
    return float(m.sum() * (1.0 - ((m / m.sum()) ** 2).sum()))


def test_root_split_is_sklearns_optimum():
    """losslessly binned features, max_depth 1: the root split maximises the same criterion, so its weighted impurity
    decrease is that of sklearn's stump (which may choose another split of equal decrease)"""
    from sklearn.tree import DecisionTreeClassifier
    kinds = [CONT, CAT, CONT, CAT, CONT, TARGET]
    cards, K = [3, 6], 4
    for seed in (31, 32, 33):
        table = np.round(fc.random_table(400, kinds, seed, cards, K, sep=0.7), 1)      # < 256 distinct values a column
        ev = fc.coded_evaluator(table, table, kinds, max_depth=1, max_rows=400, models=("dt",))
        for f, k in enumerate(kinds[:5]):             # lossless: a bin per distinct value
            assert k == CAT or ev.nbins_list[f] == len(np.unique(table[:, f])) <= 256
        s = ev.score(torch.from_numpy(table))
        tr = s.tree("dt", 0)
        w = ev.train.cw.numpy()
        M = tr["counts"].numpy()[:3] * w[None, :]
        ours = (_gini_mass(M[0]) - _gini_mass(M[1]) - _gini_mass(M[2])) / M[0].sum()
        sk = DecisionTreeClassifier(class_weight="balanced", max_depth=1, random_state=0).fit(table[:, :5], table[:, 5])
        t = sk.tree_
        wn, imp = t.weighted_n_node_samples, t.impurity
        theirs = (wn[0] * imp[0] - wn[1] * imp[1] - wn[2] * imp[2]) / wn[0]
        print(seed, ours, theirs, int(tr["feature"][0]), int(t.feature[0]))
        assert int(tr["feature"][0]) >= 0 and abs(ours - theirs) <= 1e-9 * abs(theirs)


def test_held_out_accuracy_is_within_sklearns_own_spread():
    """data.demo.small_table, train 500 / test 200, depth 12 (the default, at which most leaves are pure: in a
    shallow tree a leaf holds several whole classes, whose balanced masses tie exactly, and the accuracy says which
    class a tie goes to, not what the tree learnt).  Measured: ours 0.975, sklearn's ten 0.94 .. 0.96."""
    from sklearn.tree import DecisionTreeClassifier
    from fed_tgan_amd.eval.privacy import code_real_table
    _, df, _, meta, vocabs, enc, _, _ = fc.small_table()
    train, test = df.iloc[:500], df.iloc[500:700]
    ctr, cte = code_real_table(train, meta, vocabs), code_real_table(test, meta, vocabs)
    names = [c["column_name"] for c in meta["columns"]]
    tcol = names.index(meta["target"])
    feat = [j for j in range(len(names)) if j != tcol]
    ev = DeviceForest(train, test, meta, vocabs, "cpu", max_depth=12, max_rows=500, models=("dt",))
    ours = ev.score(torch.from_numpy(ctr)).floats()["dt_acc_real"]
    accs = []
    for rs in range(10):
        sk = DecisionTreeClassifier(class_weight="balanced", max_depth=12, random_state=rs).fit(ctr[:, feat], ctr[:, tcol])
        accs.append(float((sk.predict(cte[:, feat]) == cte[:, tcol]).mean()))
    print("ours", ours, "sklearn", accs)
    lo, hi = min(accs), max(accs)
    assert lo - (hi - lo) <= ours <= hi + (hi - lo)


def test_copy_of_the_training_rows_has_no_gap():
    from fed_tgan_amd.eval.privacy import code_real_table
    _, df, _, meta, vocabs, enc, _, _ = fc.small_table()
    train, test = df.iloc[:500], df.iloc[500:700]
    ev = DeviceForest(train, test, meta, vocabs, "cpu", trees=3, max_depth=8, max_rows=600)
    f = ev.score(torch.from_numpy(code_real_table(train, meta, vocabs))).floats()
    assert tuple(f) == KEYS
    for m in ("dt", "rf"):
        assert f[f"{m}_f1_gap"] == 0.0 and f[f"{m}_acc_gap"] == 0.0 and f[f"{m}_f1_fake"] == f[f"{m}_f1_real"] > 0.5
    assert ev.target == meta["target"]


# ----------------------------------------------------------------------------- 5. front ends
def test_loaded_generator_and_sample_cli(tmp_path, capsys):
    import dtds.sample
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.generator_io import export_generator, load_generator
    from fed_tgan_amd.models.samplers import CondTables
    _, df, _, meta, vocabs, _, tr, X = fc.small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), "cpu", backend="torch", seed=5)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    path, real_csv, out = str(tmp_path / "g.pt"), str(tmp_path / "real.csv"), str(tmp_path / "s.csv")
    test_csv = str(tmp_path / "test.csv")
    export_generator(path, eng, tr, CondTables.from_encoded(X, tr.layout), meta, vocabs, "Intrusion")
    df.iloc[:400].to_csv(real_csv, index=False)
    df.iloc[400:500].to_csv(test_csv, index=False)
    real, test = pd.read_csv(real_csv), pd.read_csv(test_csv)
    gen = load_generator(path, torch.device("cpu"), backend="torch", seed=0)
    kw = dict(trees=3, max_depth=5)
    held = np.arange(len(real)) % 5 == 4                          # the default hold-out: rows with index % 5 == 4
    torch.manual_seed(11)
    want = DeviceForest(real[~held], real[held], meta, vocabs, "cpu", max_rows=150, **kw).score(
        gen.device_table(150)).floats()
    torch.manual_seed(11)
    got = load_generator(path, torch.device("cpu"), backend="torch", seed=0).tree_utility(real, n=150, **kw)
    assert got == want and tuple(got) == KEYS and 0.0 < want["rf_f1_real"] <= 1.0
    torch.manual_seed(11)
    want_t = DeviceForest(real, test, meta, vocabs, "cpu", max_rows=150, **kw).score(gen.device_table(150)).floats()
    torch.manual_seed(11)
    g2 = load_generator(path, torch.device("cpu"), backend="torch", seed=0)
    assert g2.tree_utility(real, test, n=150, **kw) == want_t
    assert g2._forest_evaluator(real, test, 150, 3, 5) is g2._forest_evaluator(real, test, 150, 3, 5)     # cached
    # write_csv_all: the default is today's dict, the tree models add their keys to it
    torch.manual_seed(11)
    res = load_generator(path, torch.device("cpu"), backend="torch", seed=0).write_csv_all(
        out, 150, utility_real=real, utility_iters=10)
    assert len(res) == 4 and tuple(res[3]) == LR_KEYS
    torch.manual_seed(11)
    both = load_generator(path, torch.device("cpu"), backend="torch", seed=0).write_csv_all(
        out, 150, utility_real=real, utility_iters=10, utility_models=("lr", "dt", "rf"), utility_trees=3,
        utility_depth=5)[3]
    assert tuple(both) == LR_KEYS + KEYS and {k: both[k] for k in LR_KEYS} == res[3]
    assert {k: both[k] for k in KEYS} == want
    torch.manual_seed(11)
    only = load_generator(path, torch.device("cpu"), backend="torch", seed=0).write_csv_all(
        out, 150, utility_real=real, utility_models=("rf",), utility_trees=3, utility_depth=5)[3]
    assert tuple(only) == KEYS[6:] and only == {k: want[k] for k in KEYS[6:]}
    # the command line
    torch.manual_seed(11)
    dtds.sample.main(["-model", path, "-n", "150", "-backend", "torch", "-seed", "0", "-out", out, "-utility_against",
                      real_csv, "-utility_iters", "10", "-utility_models", "lr,dt,rf", "-utility_trees", "3",
                      "-utility_depth", "5"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-2].startswith("150 rows -> ") and json.loads(lines[-1]) == both and len(pd.read_csv(out)) == 150
    torch.manual_seed(11)
    dtds.sample.main(["-model", path, "-n", "150", "-backend", "torch", "-seed", "0", "-out", out, "-utility_against",
                      real_csv, "-utility_iters", "10"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res[3]
    with pytest.raises(SystemExit):
        dtds.sample.main(["-model", path, "-n", "20", "-backend", "torch", "-out", out, "-utility_models", "dt"])
    with pytest.raises(SystemExit):
        dtds.sample.main(["-model", path, "-n", "20", "-backend", "torch", "-out", out, "-utility_against", real_csv,
                          "-utility_models", "svm"])
    capsys.readouterr()
