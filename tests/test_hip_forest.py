"""The tree-utility evaluator's HIP kernels (csrc/kernels/forest.hip) against the reference ops (ops/ref.py) on the
same device and against the plain-numpy brute force of forest_cases.py, op by op and end to end.  Every comparison is
an equality (forest_cases has the one bound, on the scores); repeated runs and hipGraph replays are compared bit for
bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import forest_cases as fc
from fed_tgan_amd.eval import DeviceForest
from fed_tgan_amd.ops.ref import TorchOps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = TorchOps()


@pytest.fixture(scope="module")
def hip():
    from fed_tgan_amd.ops import native
    from fed_tgan_amd.ops.hip import HipOps
    L = native.require()
    ops = HipOps(DEV, seed=1234)
    limits = (int(L.tree_max_bins()), int(L.tree_max_classes()), int(L.tree_max_depth()), int(L.tree_max_features()))
    for o in (ops, REF):
        assert (o.TREE_MAX_BINS, o.TREE_MAX_CLASSES, o.TREE_MAX_DEPTH, o.TREE_MAX_FEATURES) == limits
    assert fc.MAX_BINS == limits[0]
    return ops


# ----------------------------------------------------------------------------- HIP ops against the torch ops
@pytest.mark.parametrize("name", fc.CASES)
def test_cases_match_reference_ops_and_brute_force(hip, name):
    fc.check_case(hip, DEV, name, oracle_ops=REF)


# ----------------------------------------------------------------------------- determinism
def _table(n, seed):
    kinds = fc.make_kinds(6, 4, seed=0)
    cards = [2 + (5 * s) % 9 for s in range(4)]
    return kinds, cards, fc.random_table(n, kinds, seed, cards, 5)


def test_runs_and_graph_replay_are_bit_identical(hip):
    kinds, cards, real = _table(400, 1)
    _, _, test = _table(150, 2)
    n = 577
    tables = [torch.from_numpy(_table(n, 10 + i)[2]).to(DEV) for i in range(2)]
    small = torch.from_numpy(_table(70, 20)[2]).to(DEV)
    kw = dict(trees=4, max_depth=6, seed=3, max_rows=n)
    eager = fc.coded_evaluator(real, test, kinds, DEV, hip, **kw)
    graph = fc.coded_evaluator(real, test, kinds, DEV, hip, graph=True, **kw)
    fresh = fc.coded_evaluator(real, test, kinds, DEV, hip, **kw)

    def snap(s):
        out = [s.buf.view(torch.int64).clone()]
        for m in ("dt", "rf"):
            out.append(s.confusion(m).clone())
            for t in range(1 if m == "dt" else 4):
                out.extend(v.clone() for v in s.tree(m, t).values())
        return out

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    first = [snap(eager.score(t)) for t in tables]
    assert not same(first[0], first[1])
    for t, want in zip(tables, first):
        assert same(snap(eager.score(t)), want)                      # a second run
        for _ in range(3):
            assert same(snap(graph.score(t)), want)                  # capture, then two replays
    # a smaller table through the same evaluator leaves no trace of the larger one before it
    want = snap(fresh.score(small))
    assert same(snap(eager.score(small)), want) and same(snap(graph.score(small)), want)
    assert same(snap(eager.score(tables[0])), first[0])
    f = fresh.score(small).floats()
    assert all(np.isfinite(v) for v in f.values()) and f["dt_f1_real"] > 0.4 and f["rf_f1_real"] > 0.4


# ----------------------------------------------------------------------------- end to end
def test_generated_table_end_to_end(hip):
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.samplers import CondTables
    _, df, _, meta, vocabs, enc, tr, X = fc.small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), DEV, backend="hip", seed=3)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    train, test = df.iloc[:500], df.iloc[500:700]
    n = 1000
    vals = eng.generate_decoded(n)
    kw = dict(trees=5, max_depth=12, max_rows=n)
    s = DeviceForest(train, test, meta, vocabs, DEV, ops=eng.ops, **kw).score(vals)
    ref = DeviceForest(train, test, meta, vocabs, "cpu", ops=REF, **kw).score(vals.cpu())
    assert s.buf.cpu().numpy().tobytes() == ref.buf.numpy().tobytes()
    for m, T in (("dt", 1), ("rf", 5)):
        assert torch.equal(s.confusion(m).cpu(), ref.confusion(m))
        for t in range(T):
            for k, v in s.tree(m, t).items():
                assert torch.equal(v.cpu(), ref.tree(m, t)[k]), (m, t, k)
    f = s.floats()
    print(f)
    assert f["dt_f1_real"] > 0.5 and f["rf_f1_real"] > 0.5 and 0.0 <= f["rf_f1_fake"] <= 1.0


# ----------------------------------------------------------------------------- the checked build
CHECKED_SCRIPT = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {tests!r}]
from fed_tgan_amd.ops import native
from fed_tgan_amd.ops.hip import HipOps
from fed_tgan_amd.ops.ref import TorchOps
import forest_cases as fc
L = native.require()
assert native.CHECKED and L.is_checked(), "checked library not loaded"
dev = torch.device("cuda:0")
fc.check_case(HipOps(dev), dev, fc.SMALLEST, oracle_ops=TorchOps())
native.check()
print("CLEAN")
"""


def test_checked_build_runs_the_smallest_case_clean():
    env = dict(os.environ, FEDTGAN_CHECKED="1")
    script = CHECKED_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert r.returncode == 0 and "CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
