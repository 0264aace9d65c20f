"""The MLP-utility evaluator's HIP kernels (csrc/kernels/mlp.hip) against the reference ops (ops/ref.py) on the same
device and against the plain-numpy brute force of mlp_cases.py, op by op and end to end.  Bounds: mlp_cases (derived
there, theta after several steps measured there), taken twice; repeated runs and hipGraph replays are compared bit for
bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mlp_cases as mc
from fed_tgan_amd.eval import DeviceMLP
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
    limits = (int(L.mlp_max_hidden()), int(L.mlp_max_batch()), int(L.mlp_max_steps()), int(L.mlp_rows()))
    assert (ops.MLP_MAX_HIDDEN, ops.MLP_MAX_BATCH, ops.MLP_MAX_STEPS, ops.MLP_ROWS) == limits
    assert (REF.MLP_MAX_HIDDEN, REF.MLP_MAX_BATCH, REF.MLP_MAX_STEPS, REF.MLP_ROWS) == limits
    assert limits == (128, 1024, 10000, mc.BLOCK)
    return ops


# ----------------------------------------------------------------------------- HIP ops against the torch ops
@pytest.mark.parametrize("name", list(mc.CASES))
def test_cases_match_reference_ops_and_brute_force(hip, name):
    mc.check_case(hip, DEV, name, oracle_ops=REF, factor=2.0)


def test_native_refusals(hip):
    train, test, fake, kinds, cardinalities, _ = mc.case_expected("rows65")
    ev = mc.coded_evaluator(train, test, kinds, DEV, hip, hidden=17, batch=64, steps=0, max_rows=65,
                            cardinalities=cardinalities)
    args = (ev.theta, ev.m, ev.v, ev.h, ev.dz, ev.dh, ev.cnt, 17, 0.0, 1e-3)
    with pytest.raises(RuntimeError, match="0 <= b < nb <= n"):
        hip.mlp_step(ev.train, 65, 2, 2, *args)
    with pytest.raises(RuntimeError, match="scratch"):
        hip.mlp_step(ev.train, 65, 0, 1, *args)                       # 65 rows in a batch; the scratch holds 64
    with pytest.raises(RuntimeError, match="MLP_MAX_HIDDEN"):
        hip.mlp_loss(ev.train, 65, ev.theta, 129, 0.0, ev.loss)
    with pytest.raises(RuntimeError, match="loss needs 3"):
        hip.mlp_loss(ev.train, 65, ev.theta, 17, 0.0, ev.loss[:2])


# ----------------------------------------------------------------------------- determinism
def test_runs_and_graph_replay_are_bit_identical(hip):
    kinds, cards, real = mc.intrusion_like(700, 1)
    test = mc.intrusion_like(200, 2)[2]
    n = 333
    tables = [torch.from_numpy(mc.intrusion_like(n, 10 + i)[2]).to(DEV) for i in range(2)]
    small = torch.from_numpy(mc.intrusion_like(70, 20)[2]).to(DEV)
    eager = mc.coded_evaluator(real, test, kinds, DEV, hip, steps=12, max_rows=n)
    graph = mc.coded_evaluator(real, test, kinds, DEV, hip, steps=12, max_rows=n, graph=True)
    fresh = mc.coded_evaluator(real, test, kinds, DEV, hip, steps=12, max_rows=n)

    def same(a, b):
        return (torch.equal(a.buf.view(torch.int64), b.buf.view(torch.int64)) and
                all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a.weights(), b.weights()))
                and torch.equal(a.confusion(), b.confusion()))

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
    assert all(np.isfinite(v) for v in f.values()) and 0.0 <= f["mlp_f1_real"] <= 1.0


# ----------------------------------------------------------------------------- end to end
def test_generated_table_end_to_end(hip):
    train, test, meta, vocabs, eng, vals = mc.generated_tables(DEV, "hip", 1000)
    s = DeviceMLP(train, test, meta, vocabs, DEV, ops=eng.ops, steps=20, max_rows=1000).score(vals)
    ref_ev = DeviceMLP(train, test, meta, vocabs, "cpu", ops=REF, steps=20, max_rows=1000)
    ref = ref_ev.score(vals.cpu())
    got = torch.cat([w.reshape(-1) for w in s.weights()]).cpu().numpy()
    want = torch.cat([w.reshape(-1) for w in ref.weights()]).numpy()
    mc.worst(got, want, 2 * mc.THETA_TOL, "generated theta")
    f, r = s.floats(), ref.floats()
    print(f, r)
    # the derived bound of the loss, from the brute force's gradient of the objective over the whole table at the
    # reference's theta: the two thetas differ by 2 THETA_TOL at most, and each side rounds its own sums
    from fed_tgan_amd.eval.privacy import code_real_table
    from utility_cases import CAT, CONT, TARGET, features, setup
    kinds = [TARGET if c["column_name"] == meta["target"] else CAT if c["type"] == "categorical" else CONT
             for c in meta["columns"]]
    cards, K, mean, sd = setup(code_real_table(train, meta, vocabs), code_real_table(test, meta, vocabs), kinds,
                               [len(v) for v in vocabs])
    F, y = features(vals.cpu().numpy(), kinds, cards, K, mean, sd)
    D, H = F.shape[1], 100
    assert (D, K) == (ref_ev.D, ref_ev.K)
    present = np.bincount(y, minlength=K + 1)[:K] > 0
    g1, g2, loss, _ = mc.objective(F, y, present, want[:D * H].reshape(D, H), want[D * H:].reshape(H + 1, K), mc.ALPHA)
    tol = float(np.abs(mc.flat(g1, g2)).sum()) * 2 * mc.THETA_TOL + 4 * mc.gamma(1000 + H + K) * loss
    print(f"loss {f['mlp_loss_fake']!r} against {r['mlp_loss_fake']!r} (brute force {loss!r}), bound {tol:.3e}")
    assert abs(f["mlp_loss_fake"] - r["mlp_loss_fake"]) <= tol
    assert 0.0 <= f["mlp_f1_fake"] <= 1.0 and 0.0 <= f["mlp_f1_real"] <= 1.0


# ----------------------------------------------------------------------------- the checked build
CHECKED_SCRIPT = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {tests!r}]
from fed_tgan_amd.ops import native
from fed_tgan_amd.ops.hip import HipOps
from fed_tgan_amd.ops.ref import TorchOps
import mlp_cases as mc
L = native.require()
assert native.CHECKED and L.is_checked(), "checked library not loaded"
dev = torch.device("cuda:0")
mc.check_case(HipOps(dev), dev, "rows1", oracle_ops=TorchOps(), factor=2.0)
native.check()
print("CLEAN")
"""


def test_checked_build_runs_the_smallest_case_clean():
    env = dict(os.environ, FEDTGAN_CHECKED="1")
    script = CHECKED_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert r.returncode == 0 and "CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
