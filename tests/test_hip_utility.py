"""The utility evaluator's HIP kernels (csrc/kernels/utility.hip) against the reference ops (ops/ref.py) on the same
device and against the plain-numpy brute force of utility_cases.py, op by op and end to end.  Bounds: utility_cases
(derived there, W after several steps measured there); repeated runs and hipGraph replays are compared bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import utility_cases as uc
from fed_tgan_amd.eval import DeviceUtility
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
    limits = (int(L.util_max_features()), int(L.util_max_classes()), int(L.util_chunk()))
    assert (ops.UTIL_MAX_FEATURES, ops.UTIL_MAX_CLASSES, ops.UTIL_CHUNK) == limits
    assert (REF.UTIL_MAX_FEATURES, REF.UTIL_MAX_CLASSES, REF.UTIL_CHUNK) == limits and uc.CHUNK == limits[2]
    C = ops.UTIL_CHUNK
    assert [ops.util_groups(n, 100) for n in (1, C, C + 1, 2 * C + 1)] == [1, 1, 2, 3]
    assert uc.CASES["wide"][1] + sum(k + 1 for k in uc.CASES["wide"][2]) + 1 == ops.UTIL_MAX_FEATURES - 1
    assert max(c[3] for c in uc.CASES.values()) == ops.UTIL_MAX_CLASSES
    return ops


# ----------------------------------------------------------------------------- 5. HIP ops against the torch ops
@pytest.mark.parametrize("name", list(uc.CASES))
def test_cases_match_reference_ops_and_brute_force(hip, name):
    uc.check_case(hip, DEV, name, oracle_ops=REF)


def test_row_groups_of_several_chunks(hip):
    """the partials' budget caps the row groups: at D near the limit the Gram matrix's groups hold several chunks"""
    name = "wide"
    train, test, _, kinds, cardinalities = uc.build_case(name)
    n = 9 * hip.UTIL_CHUNK + 5
    D = hip.UTIL_MAX_FEATURES - 1
    assert hip.util_groups(n, D * D) < hip.util_groups(n, D * 3) == 10
    fake = uc.random_table(n, kinds, 7, uc.CASES[name][2], 3)
    ev = uc.coded_evaluator(train, test, kinds, DEV, hip, iters=1, max_rows=n, cardinalities=cardinalities)
    got, ref = uc.run_ops(hip, ev, fake, (1,)), uc.run_ops(REF, ev, fake, (1,))
    cards, K, mean, sd = uc.setup(train, test, kinds, cardinalities)
    F, y = uc.features(fake, kinds, cards, K, mean, sd)
    b = uc.assert_fit(got, uc.fit(F, y, K, 1, (1,)), "several chunks", (1,))
    uc.worst(got["M"], ref["M"], 2 * b["M"] + 1e-300, "several chunks M vs oracle")


# ----------------------------------------------------------------------------- 6. determinism
def _intrusion_like(n, seed):
    kinds = uc.make_kinds(22, 8, seed=0)
    cards = [2 + (5 * s) % 9 for s in range(8)]
    return kinds, cards, uc.random_table(n, kinds, seed, cards, 5)


def test_runs_and_graph_replay_are_bit_identical(hip):
    kinds, cards, real = _intrusion_like(700, 1)
    _, _, test = _intrusion_like(200, 2)
    n = 2 * hip.UTIL_CHUNK + 77
    tables = [torch.from_numpy(_intrusion_like(n, 10 + i)[2]).to(DEV) for i in range(2)]
    small = torch.from_numpy(_intrusion_like(70, 20)[2]).to(DEV)
    eager = uc.coded_evaluator(real, test, kinds, DEV, hip, iters=12, max_rows=n)
    graph = uc.coded_evaluator(real, test, kinds, DEV, hip, iters=12, max_rows=n, graph=True)
    fresh = uc.coded_evaluator(real, test, kinds, DEV, hip, iters=12, max_rows=n)

    def same(a, b):
        return (torch.equal(a.buf.view(torch.int64), b.buf.view(torch.int64)) and
                torch.equal(a.weights().view(torch.int64), b.weights().view(torch.int64)) and
                torch.equal(a.confusion(), b.confusion()))

    first = [eager.score(t) for t in tables]
    assert not same(first[0], first[1])
    for t, want in zip(tables, first):
        assert same(eager.score(t), want)                      # a second run
        for _ in range(2):
            assert same(graph.score(t), want)                  # capture, then replay
    # a smaller table through the same evaluator leaves no trace of the larger one before it
    want = fresh.score(small)
    assert same(eager.score(small), want) and same(graph.score(small), want)
    assert same(eager.score(tables[0]), first[0])
    f = want.floats()
    assert all(np.isfinite(v) for v in f.values()) and f["f1_real"] > 0.5


# ----------------------------------------------------------------------------- end to end
def test_generated_table_end_to_end(hip):
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.samplers import CondTables
    _, df, _, meta, vocabs, enc, tr, X = uc.small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), DEV, backend="hip", seed=3)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    train, test = df.iloc[:500], df.iloc[500:700]
    n = 1000
    vals = eng.generate_decoded(n)
    s = DeviceUtility(train, test, meta, vocabs, DEV, ops=eng.ops, iters=20, max_rows=n).score(vals)
    ref = DeviceUtility(train, test, meta, vocabs, "cpu", ops=REF, iters=20, max_rows=n).score(vals.cpu())
    uc.worst(s.weights().cpu().numpy(), ref.weights().numpy(), 2 * uc.W_TOL, "generated W")
    f, r = s.floats(), ref.floats()
    print(f, r)
    assert f["f1_real"] > 0.5 and 0.0 <= f["f1_fake"] <= 1.0 and np.isfinite(f["grad_fake"])
    assert abs(f["loss_fake"] - r["loss_fake"]) <= 1e-9 * max(1.0, abs(r["loss_fake"]))


# ----------------------------------------------------------------------------- 7. the checked build
CHECKED_SCRIPT = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {tests!r}]
from fed_tgan_amd.ops import native
from fed_tgan_amd.ops.hip import HipOps
from fed_tgan_amd.ops.ref import TorchOps
import utility_cases as uc
L = native.require()
assert native.CHECKED and L.is_checked(), "checked library not loaded"
dev = torch.device("cuda:0")
uc.check_case(HipOps(dev), dev, "rows1", oracle_ops=TorchOps())
native.check()
print("CLEAN")
"""


def test_checked_build_runs_the_smallest_case_clean():
    env = dict(os.environ, FEDTGAN_CHECKED="1")
    script = CHECKED_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert r.returncode == 0 and "CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
