"""The shared evaluator base (eval/base.py) and LoadedGenerator's one evaluator cache, on the CPU."""
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch

from fed_tgan_amd.data.vocab import CategoryVocab
from fed_tgan_amd.eval.base import category_counts, coded_table, column_slots
from fed_tgan_amd.eval.correlation import DeviceCorrelation
from fed_tgan_amd.eval.device import DeviceSimilarity
from fed_tgan_amd.eval.forest_device import DeviceForest
from fed_tgan_amd.eval.privacy import DevicePrivacy
from fed_tgan_amd.eval.utility_device import DeviceUtility
from fed_tgan_amd.models.generator_io import LoadedGenerator
from fed_tgan_amd.ops.ref import TorchOps

ROWS, MAX_ROWS = 40, 12
META = {"columns": [{"column_name": "x", "type": "continuous"}, {"column_name": "a", "type": "categorical"},
                    {"column_name": "y", "type": "continuous"}, {"column_name": "t", "type": "categorical"}],
        "non_negative_cols": [], "target": "t", "problem_type": "Classification"}
VOCABS = [CategoryVocab(["p", "q", "r"], "a"), CategoryVocab(["no", "yes"], "t")]


def real_frame() -> pd.DataFrame:
    rng = np.random.default_rng(3)
    return pd.DataFrame({"x": rng.normal(size=ROWS), "a": rng.choice(["p", "q", "r"], ROWS), "y": rng.normal(size=ROWS),
                         "t": np.where(np.arange(ROWS) % 3 == 0, "yes", "no")})


def coded() -> np.ndarray:
    rng = np.random.default_rng(4)
    return np.stack([rng.normal(size=ROWS), rng.integers(0, 3, ROWS), rng.normal(size=ROWS), np.arange(ROWS) % 2],
                    axis=1).astype(np.float64)


def evaluators():
    """the five evaluators over the same small real table, each with buffers for MAX_ROWS rows"""
    c, kw = coded(), dict(max_rows=MAX_ROWS)
    return [DeviceSimilarity(real_frame(), META, VOCABS, "cpu", **kw), DevicePrivacy(c, META, VOCABS, "cpu", **kw),
            DeviceCorrelation(c, META, VOCABS, "cpu", **kw), DeviceUtility(c, c[:10], META, VOCABS, "cpu", iters=2, **kw),
            DeviceForest(c, c[:10], META, VOCABS, "cpu", trees=2, max_depth=2, **kw)]


# ----------------------------------------------------------------------------- the helpers
def test_category_counts():
    table = np.array([[0.5, 1.0, 0.0], [1.5, 0.0, 6.0]])
    cat_cols = [1, 2]
    vocabs = [CategoryVocab(list("abcd"), "u"), CategoryVocab(list("ab"), "v")]
    assert category_counts(table, cat_cols, vocabs, None, "X") == [4, 7]         # the vocabulary / the codes decide
    assert category_counts(table, cat_cols, [], None, "X") == [2, 7]             # coded arrays come without vocabularies
    assert category_counts(table, cat_cols, vocabs, [9, 3], "X") == [9, 7]       # an override only raises a count
    with pytest.raises(ValueError, match=r"^X: cardinalities needs one entry per categorical column \(2\)$"):
        category_counts(table, cat_cols, vocabs, [9], "X")


def test_column_slots():
    assert column_slots([0, 1, 1, 0, 2]) == ([0, 0, 1, 1, 0], {0: 2, 1: 2, 2: 1})
    assert column_slots([0, 1, 1, 0, 2], {1: 0}) == ([0, 1, 2, 3, 0], {0: 4, 2: 1})


def test_coded_table_messages_name_the_caller():
    c = coded()
    assert coded_table(c, META, VOCABS, "DeviceX") is not None
    with pytest.raises(ValueError, match=r"^DeviceX: expected a coded \[m, 4\] real test table, got \(40, 3\)$"):
        coded_table(c[:, :3], META, VOCABS, "DeviceX", "real test")
    with pytest.raises(ValueError, match=r"^DeviceY: the real table is empty$"):
        coded_table(c[:0], META, VOCABS, "DeviceY")
    bad = c.copy()
    bad[3, 1] = -1.0
    with pytest.raises(ValueError, match=r"^DeviceY: the real column 'a' holds a value that is not a category code$"):
        coded_table(bad, META, VOCABS, "DeviceY")
    assert coded_table(bad, META, VOCABS, "DevicePrivacy", finite="array") is not None   # privacy: continuous only
    bad[5, 2] = np.inf
    with pytest.raises(ValueError, match=r"^DevicePrivacy: the real column 'y' holds a value that is not a finite"):
        coded_table(bad, META, VOCABS, "DevicePrivacy", finite="array")
    frame = real_frame()
    got = coded_table(frame, META, VOCABS, "DeviceX", lost_rows=True)
    assert got.shape == (ROWS, 4) and got.dtype == np.float64
    with pytest.raises(ValueError, match=r"^DevicePrivacy: the real table lacks columns \['y'\]$"):
        coded_table(frame.drop(columns="y"), META, VOCABS, "DeviceX")              # code_real_table's own message


# ----------------------------------------------------------------------------- score(), written once
def test_every_evaluator_refuses_a_wrong_table():
    evs = evaluators()
    assert [type(e).__name__ for e in evs] == ["DeviceSimilarity", "DevicePrivacy", "DeviceCorrelation",
                                               "DeviceUtility", "DeviceForest"]
    good = torch.from_numpy(coded()[:MAX_ROWS])
    for ev in evs:
        who = type(ev).__name__
        with pytest.raises(ValueError) as e:
            ev.score(good.float())
        assert str(e.value) == "score: expected a float64 [n, 4] table, got (12, 4) torch.float32", who
        with pytest.raises(ValueError) as e:
            ev.score(good[:, :3])
        assert str(e.value) == "score: expected a float64 [n, 4] table, got (12, 3) torch.float64", who
        with pytest.raises(ValueError) as e:
            ev.score(torch.from_numpy(coded()[:MAX_ROWS + 1]))
        assert str(e.value) == "score: 13 rows; this evaluator's buffers hold 1..12", who
        assert ev.score(good).buf.dtype == torch.float64 and not ev.graph and ev._staged is None


def test_score_ends_with_the_ops_check():
    class Checked(TorchOps):
        calls = 0

        def check(self):
            self.calls += 1

    c, ops = coded(), Checked()
    for ev in (DevicePrivacy(c, META, VOCABS, "cpu", ops=ops, max_rows=MAX_ROWS),
               DeviceUtility(c, c[:10], META, VOCABS, "cpu", ops=ops, iters=1, max_rows=MAX_ROWS)):
        before = ops.calls
        ev.score(torch.from_numpy(c[:5]))
        assert ops.calls == before + 1


# ----------------------------------------------------------------------------- LoadedGenerator's cache
def test_loaded_generator_keeps_one_evaluator_per_kind(tmp_path):
    engine = SimpleNamespace(device=torch.device("cpu"), ops=TorchOps())
    gen = LoadedGenerator("g", engine, None, META, VOCABS)
    frame, c = real_frame(), coded()
    held = c[:10]                    # (kept: an array is recognised by its id)
    path = str(tmp_path / "real.csv")
    frame.to_csv(path, index=False)
    getters = [(gen._evaluator, (path,)), (gen._evaluator, (frame,)), (gen._privacy_evaluator, (c,)),
               (gen._correlation_evaluator, (c,)), (gen._utility_evaluator, (frame, None)),
               (gen._forest_evaluator, (c, held))]
    for get, tables in getters:
        kw = dict(trees=2, max_depth=2) if get == gen._forest_evaluator else {}
        kw = dict(iters=2) if get == gen._utility_evaluator else kw
        ev = get(*tables, 8, **kw)
        assert get(*tables, 8, **kw) is ev and ev.max_rows == 8                   # a repeat call: the same object
        other = get(*tables, 9, **kw)
        assert other is not ev and other.max_rows == 9                            # new parameters: a new one
        assert get(*tables, 9, **kw) is other
    assert sorted(gen._evaluators) == ["correlation", "forest", "privacy", "similarity", "utility"]
    ev = gen._utility_evaluator(frame, None, 9, iters=2)                          # the default hold-out, written once
    assert (ev.n_train, ev.n_test) == (ROWS - ROWS // 5, ROWS // 5) and ev.iters == 2
    assert gen._utility_evaluator(frame, None, 9, iters=3).iters == 3
    assert gen._forest_evaluator(c, held, 9, 2, 2) is gen._forest_evaluator(c, held, 9, trees=2, max_depth=2)
