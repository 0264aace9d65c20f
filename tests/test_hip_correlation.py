"""The correlation evaluator's HIP kernels (csrc/kernels/correlation.hip) against the plain-numpy brute force of
correlation_cases.py and against the reference ops (ops/ref.py).  Bounds: correlation_cases.TOL (derived there);
repeated runs and hipGraph replays are compared bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import correlation_cases as cc
from fed_tgan_amd.eval import DeviceCorrelation
from fed_tgan_amd.ops.ref import TorchOps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = TorchOps()
CONT, CAT = cc.CONT, cc.CAT


@pytest.fixture(scope="module")
def hip():
    from fed_tgan_amd.ops import native
    from fed_tgan_amd.ops.hip import HipOps
    L = native.require()
    ops = HipOps(DEV, seed=1234)
    assert (ops.CORR_CHUNK, ops.CORR_LDS_BINS) == (int(L.corr_chunk()), int(L.corr_lds_bins()))
    assert (REF.CORR_CHUNK, REF.CORR_LDS_BINS) == (ops.CORR_CHUNK, ops.CORR_LDS_BINS)
    K = ops.CORR_CHUNK
    assert [ops.corr_groups(n, 10, 3) for n in (1, K, K + 1, 2 * K + 1)] == [1, 1, 2, 3]
    assert 2 * 4 * ops.CORR_LDS_BINS <= 160 * 1024      # two workgroups' tables in a CU's LDS
    return ops


def _against_reference(hip, ev, table, what):
    """the HIP matrix against the reference ops run on the same device"""
    A, G, counts = cc.run_matrix(hip, ev, table)
    Ar, Gr, cr = cc.run_matrix(REF, ev, table)
    assert np.array_equal(counts, cr), what                   # integers
    cc.assert_matrix(A, Ar, what + " vs reference ops")
    return A, G, counts


@pytest.mark.parametrize("layout", list(cc.LAYOUTS))
def test_layouts_match_brute_force(hip, layout):
    for n in (1, 63, 64, 65, 2 * hip.CORR_CHUNK + 1):
        ev, fake = cc.check_layout(hip, DEV, layout, n, seed=n)
        _against_reference(hip, ev, fake, f"{layout} n={n}")


@pytest.mark.parametrize("n_cont", [1, 16, 17, 32, 33])
def test_tile_edges(hip, n_cont):
    """continuous columns around the 16-wide MFMA tile and the 32-wide tile of a wave; categories of 1, 2 and 70
    values, so one-hot rows start inside a tile, fill less than one and span several"""
    cards = [1, 2, 70]
    kinds = [CONT] * n_cont + [CAT] * 3
    real = cc.random_table(700, kinds, 1, cards)
    fake = cc.random_table(333, kinds, 2, cards)
    want = cc.expected(real, fake, kinds, cardinalities=cards)
    ev = cc.coded_evaluator(real, kinds, DEV, hip, max_rows=333, cardinalities=cards)
    A, _, _ = _against_reference(hip, ev, fake, f"edges n_cont={n_cont}")
    cc.assert_matrix(A, want["A_fake"], f"edges n_cont={n_cont}")
    cc.assert_scores(ev.score(torch.from_numpy(fake).to(DEV)).floats(), want, len(kinds), f"edges n_cont={n_cont}")


def test_capped_row_groups_sum_several_chunks_each(hip):
    """the partials' budget caps the row groups (a 512-column table at 40,000 rows: 6 groups of 7 chunks); here the
    budget is shrunk to two groups' worth, so 6 and 4 chunks fold into 2 groups of 3 and of 2 chunks"""
    kinds = cc.layout_kinds(5, 4)
    chunk = hip.CORR_CHUNK
    n = 5 * chunk + 1
    real = cc.random_table(700, kinds, 1)
    fake = cc.random_table(n, kinds, 2)
    W, nc = cc.coded_evaluator(real, kinds, DEV, hip, max_rows=1).W, 5
    assert hip.corr_groups(n, W, nc) == 6
    prev = torch.ops.fedtgan.set_tuning("corr_part_target", 2 * W * nc + 1)
    try:
        assert [hip.corr_groups(m, W, nc) for m in (n, 3 * chunk + 1, 2 * chunk, chunk)] == [2, 2, 2, 1]
        assert hip.corr_part(n, W, nc) == max(2 * W * nc, 6 * nc)
        ev = cc.coded_evaluator(real, kinds, DEV, hip, max_rows=n)         # its scratch is sized under the budget
        assert ev.part.numel() == hip.corr_part(n, W, nc)
        for m in (n, 3 * chunk + 1):
            want = cc.expected(real, fake[:m], kinds)
            A, _, _ = _against_reference(hip, ev, fake[:m], f"capped groups n={m}")
            cc.assert_matrix(A, want["A_fake"], f"capped groups n={m}")
            cc.assert_scores(ev.score(torch.from_numpy(fake[:m].copy()).to(DEV)).floats(), want, len(kinds),
                             f"capped groups n={m}")
    finally:
        torch.ops.fedtgan.set_tuning("corr_part_target", prev)
    assert hip.corr_groups(n, W, nc) == 6


def test_large_pair_counts_in_global_memory(hip):
    K = 181
    while (K + 1) * (K + 1) <= hip.CORR_LDS_BINS:       # (a larger constant: a cardinality past it)
        K += 50
    g = np.random.default_rng(4)
    kinds = [CAT, CAT, CONT, CAT]

    def table(n):
        a = g.integers(0, K, n)
        b = (a + g.integers(0, 3, n)) % K
        return np.stack([a, b, a * 0.1 + g.normal(size=n), g.integers(0, 3, n)], axis=1).astype(np.float64)

    real, fake = table(3000), table(3000)
    fake[::11, 0] = -3.0                                  # the overflow bin of a large table
    cards = [K, K, 3]
    ev = cc.coded_evaluator(real, kinds, DEV, hip, max_rows=3000, cardinalities=cards)
    assert ev.global_pairs == [(0, 1)] and (K + 1) ** 2 > hip.CORR_LDS_BINS >= ev.lds_bins == (K + 1) * 4
    want = cc.expected(real, fake, kinds, cardinalities=cards)
    A, _, counts = _against_reference(hip, ev, fake, "large pair")
    cc.assert_matrix(A, want["A_fake"], "large pair")
    assert int(counts[:K + 1].sum()) == 3000 and int(counts[K]) == len(fake[::11])
    cc.assert_scores(ev.score(torch.from_numpy(fake).to(DEV)).floats(), want, len(kinds), "large pair")


def test_two_runs_are_bit_identical(hip):
    n_cont, n_cat = cc.LAYOUTS["intrusion"]
    kinds = cc.layout_kinds(n_cont, n_cat)
    real = cc.random_table(500, kinds, 1)
    fake = cc.random_table(2 * hip.CORR_CHUNK + 77, kinds, 2)
    ev = cc.coded_evaluator(real, kinds, DEV, hip, max_rows=len(fake))
    a = cc.run_matrix(hip, ev, fake)        # (guard tails checked inside)
    b = cc.run_matrix(hip, ev, fake)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    s1, s2 = ev.score(torch.from_numpy(fake).to(DEV)), ev.score(torch.from_numpy(fake).to(DEV))
    assert torch.equal(s1.buf.view(torch.int64), s2.buf.view(torch.int64)) and torch.equal(s1.matrix(), s2.matrix())


def test_graph_replay_is_bit_identical(hip):
    from fed_tgan_amd.eval.device import MAX_GRAPHS
    kinds = cc.layout_kinds(5, 4)
    real = cc.random_table(900, kinds, 1)
    n = hip.CORR_CHUNK + 5
    eager = cc.coded_evaluator(real, kinds, DEV, hip, max_rows=n)
    graph = cc.coded_evaluator(real, kinds, DEV, hip, max_rows=n, graph=True)
    tables = [torch.from_numpy(cc.random_table(n, kinds, 10 + i)).to(DEV) for i in range(MAX_GRAPHS + 2)]
    for i, t in enumerate(tables):      # the last two go through the staging buffer and share its graph
        want = eager.score(t)
        for _ in range(2):
            got = graph.score(t)
            assert torch.equal(want.buf.view(torch.int64), got.buf.view(torch.int64)), i
            assert torch.equal(want.matrix(), got.matrix()), i
    assert len(graph._graphs) == MAX_GRAPHS + 1 and graph._staged is not None
    assert float(eager.score(tables[0]).buf[0]) != float(eager.score(tables[-1]).buf[0])


# ----------------------------------------------------------------------------- end to end
def test_generated_table_end_to_end(hip):
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.samplers import CondTables
    _, df, _, meta, vocabs, enc, tr, X = cc.small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), DEV, backend="hip", seed=3)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    real = df.iloc[:500]
    n = 2000
    vals = eng.generate_decoded(n)
    assert vals.is_cuda and vals.dtype == torch.float64 and vals.shape == (n, len(meta["columns"]))
    s = DeviceCorrelation(real, meta, vocabs, DEV, ops=eng.ops, max_rows=n).score(vals)
    ref = DeviceCorrelation(real, meta, vocabs, "cpu", ops=REF, max_rows=n).score(vals.cpu())
    cc.assert_matrix(s.matrix().cpu().numpy(), ref.matrix().numpy(), "generated")
    C = len(meta["columns"])
    f = s.floats()
    cc.assert_scores(f, ref.floats(), C, "generated")
    assert f["corr_diff"] > 0.0 and f["corr_diff_rr"] > 0.0
    p = s.pairs(7)
    names = [c["column_name"] for c in meta["columns"]]
    assert len(p) == 7 and set(p["column_i"]) <= set(names) and set(p["column_j"]) <= set(names)
    assert (p["column_i"] != p["column_j"]).all() and p["abs_diff"][0] == f["corr_max_abs"]


CHECKED_SCRIPT = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {tests!r}]
from fed_tgan_amd.ops import native
from fed_tgan_amd.ops.hip import HipOps
from fed_tgan_amd.ops.ref import TorchOps
from fed_tgan_amd.eval import DeviceCorrelation
import correlation_cases as cc
L = native.require()
assert native.CHECKED and L.is_checked(), "checked library not loaded"
dev = torch.device("cuda:0")
_, df, _, meta, vocabs, enc, _, _ = cc.small_table()
t = torch.from_numpy(np.ascontiguousarray(np.asarray(enc)[100:300], dtype=np.float64))
f = DeviceCorrelation(df.iloc[:300], meta, vocabs, dev, ops=HipOps(dev), max_rows=200).score(t.to(dev)).floats()
native.check()
want = DeviceCorrelation(df.iloc[:300], meta, vocabs, "cpu", ops=TorchOps(), max_rows=200).score(t).floats()
cc.assert_scores(f, want, len(meta["columns"]), "checked")
print("CLEAN", f)
"""


def test_checked_build_scores_a_clean_table():
    env = dict(os.environ, FEDTGAN_CHECKED="1")
    script = CHECKED_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert r.returncode == 0 and "CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
