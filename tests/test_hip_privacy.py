"""The privacy evaluator's HIP kernels (csrc/kernels/privacy.hip) against the reference ops (ops/ref.py) and, end to
end, against the plain-numpy brute force of privacy_cases.py.  Bounds: privacy_cases.TOL (derived there); the integer
cases and repeated runs are compared bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import privacy_cases as pc
from fed_tgan_amd.eval import DevicePrivacy
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
    assert (ops.NN_QUERY_TILE, ops.NN_REF_TILE, ops.NN_CHUNK_ROWS) == (int(L.nn_query_tile()), int(L.nn_ref_tile()),
                                                                       int(L.nn_chunk_rows()))
    K = ops.NN_CHUNK_ROWS
    assert [ops.nn_chunks(n) for n in (1, K - 1, K, K + 1, 2 * K + 7)] == [1, 1, 1, 2, 3]
    return ops


def _shapes(hip):
    """every query-side size with two reference-side sizes and every reference-side size with two query-side
    sizes, around the query tile, the LDS tile and the chunk"""
    tq, tr, k = hip.NN_QUERY_TILE, hip.NN_REF_TILE, hip.NN_CHUNK_ROWS
    nqs = [1, 2, tq - 1, tq, tq + 1, 3 * tq + 5]
    nrs = [1, 2, 3, tr - 1, tr + 1, k - 1, k, k + 1, 2 * k + 7]
    pairs = [(nq, nr) for nq in nqs for nr in (tr + 1, k + 1)] + [(nq, nr) for nr in nrs for nq in (2, tq + 1)]
    return sorted(set(pairs)), [1, 2, tr + 1, tq + 1, k + 1, 2 * k + 7]


def _both(hip, q_cont, q_cat, r_cont, r_cat, same, what):
    """HIP against TorchOps on the same device tensors' values, and the returned i1 through the oracle"""
    w1, w2, _ = pc.run_top2(REF, DEV, q_cont, q_cat, r_cont, r_cat, same)
    d1, d2, i1 = pc.run_top2(hip, DEV, q_cont, q_cat, r_cont, r_cat, same)
    pc.assert_top2(d1, d2, i1, w1, w2, q_cont, q_cat, r_cont, r_cat, same, what)
    return d1, d2, i1


@pytest.mark.parametrize("layout", ["cont", "cat", "small", "intrusion"])
def test_top2_matches_reference(hip, layout):
    n_cont, n_cat = pc.LAYOUTS[layout]
    pairs, selfs = _shapes(hip)
    for nq, nr in pairs:
        t = pc.random_packed(nq, nr, n_cont, n_cat, seed=nq * 7 + nr)
        _, _, i1 = _both(hip, *t, False, f"{layout} {nq}x{nr}")
        if n_cont == 0:       # integer distances: the lowest index of a tie, exactly
            assert np.array_equal(i1, pc.top2(*t)[2]), (layout, nq, nr)
    for n in selfs:           # a table against itself, self excluded
        t = pc.random_packed(n, n, n_cont, n_cat, seed=n, same=True)
        _both(hip, *t, True, f"{layout} self {n}")


@pytest.mark.parametrize("same", [False, True])
def test_top2_wide_rows_take_the_column_blocked_path(hip, same):
    n_cont, n_cat = pc.LAYOUTS["wide"]
    tq, k = hip.NN_QUERY_TILE, hip.NN_CHUNK_ROWS
    for nq, nr in ((tq + 1, k + 1), (2, 3)):
        if same:
            nq = nr
        t = pc.random_packed(nq, nr, n_cont, n_cat, seed=nq + nr, same=same)
        _both(hip, *t, same, f"wide {nq}x{nr} same={same}")


def test_exact_integer_cases_bit_for_bit(hip):
    """the CPU file's cases; the equal candidates sit in different chunks, and in different LDS tiles of one chunk"""
    tr, k = hip.NN_REF_TILE, hip.NN_CHUNK_ROWS
    pc.check_exact_cases(hip, DEV, k + 40, [(5, k + 3), (tr + 1, 5 * tr + 2), (k - 1, k)])
    pc.check_exact_cases(hip, DEV, 40, [(3, 30), (5, 6)])
    pc.check_single_reference_row(hip, DEV)


def test_two_runs_are_bit_identical(hip):
    q_cont, q_cat, r_cont, r_cat = pc.random_packed(600, 2 * hip.NN_CHUNK_ROWS + 7, 22, 20, seed=3)
    a = pc.run_top2(hip, DEV, q_cont, q_cat, r_cont, r_cat, False)      # (guard tails checked inside)
    b = pc.run_top2(hip, DEV, q_cont, q_cat, r_cont, r_cat, False)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("rows", [1, 257, 1500])
def test_pack_matches_reference(hip, rows):
    g = torch.Generator().manual_seed(rows)
    kinds = [pc.CONT, pc.CAT, pc.CONT, pc.CAT, pc.CONT, pc.CAT, pc.CONT]
    slots = [0, 0, 1, 1, 2, 2, 3]
    vals = torch.randn(rows, len(kinds), generator=g, dtype=torch.float64) * 100.0
    for c, k in enumerate(kinds):
        if k == pc.CAT:
            vals[:, c] = torch.randint(0, 3000, (rows,), generator=g).double()
    vals[0, 1] = 2.0 ** 31 - 2.0                      # the largest code
    vals[rows - 1, 3] = 70000.0                       # a real category past a vocabulary
    lo = torch.randn(4, generator=g, dtype=torch.float64) * 10.0
    scale = 1.0 / (torch.rand(4, generator=g, dtype=torch.float64) * 50.0 + 0.01)

    def run(ops, dev):
        cont = torch.full((rows + 2, 4), -5.0, dtype=torch.float64, device=dev)
        cat = torch.full((rows + 2, 3), -5, dtype=torch.int32, device=dev)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)      # noqa: E731
        ops.nn_pack(vals.to(dev), i32(kinds), i32(slots), lo.to(dev), scale.to(dev), cont, cat)
        return cont.cpu(), cat.cpu()

    hc, hk = run(hip, DEV)
    rc, rk = run(REF, "cpu")
    assert torch.equal(hc.view(torch.int64), rc.view(torch.int64))      # one subtraction, one product: bit-equal
    assert torch.equal(hk, rk)
    assert int(hk[0, 0]) == 2 ** 31 - 2 and int(hk[rows - 1, 1]) == 70000
    assert bool((hc[rows:] == -5.0).all()) and bool((hk[rows:] == -5).all())


@pytest.mark.parametrize("n", [1, 2, 20, 21, 2049])     # 0.05 (n - 1): 0, fractional, fractional, 1, past a sort tile
def test_percentiles_match_numpy(hip, n):
    g = np.random.default_rng(n)
    d2 = g.random(n) * 4.0
    d1 = d2 * g.random(n)
    d1[::5] = 0.0
    d2[::10] = 0.0
    if n > 2:
        d2[1] = np.inf
    dcr, nndr, want = pc.table_scores(d1, d2)
    pad = 3
    keys = torch.full((2, n + pad), -9.0, dtype=torch.float64, device=DEV)
    out = torch.full((6,), -9.0, dtype=torch.float64, device=DEV)
    part = torch.zeros(hip.nn_stats_part(n), dtype=torch.float64, device=DEV)
    hip.nn_stats(torch.from_numpy(d1).to(DEV), torch.from_numpy(d2).to(DEV), n, keys, torch.empty_like(keys), part, out)
    got = out.cpu().tolist()
    assert got[4:] == [-9.0, -9.0] and bool((keys[:, n:] == -9.0).all())
    assert np.abs(keys[0, :n].cpu().numpy() - np.sort(dcr)).max() <= pc.TOL
    assert np.abs(keys[1, :n].cpu().numpy() - np.sort(nndr)).max() <= pc.TOL
    print(n, got[:4], want)
    assert np.abs(np.asarray(got[:4]) - np.asarray(want)).max() <= pc.TOL
    assert got[3] == want[3]                                                   # a count over n
    ref_out = torch.zeros(6, dtype=torch.float64)
    REF.nn_stats(torch.from_numpy(d1), torch.from_numpy(d2), n, torch.zeros(2, n, dtype=torch.float64), None, None,
                 ref_out)
    assert np.abs(np.asarray(got[:4]) - ref_out[:4].numpy()).max() <= pc.TOL


# ----------------------------------------------------------------------------- end to end
def test_generated_table_end_to_end(hip, tmp_path):
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.generator_io import export_generator, load_generator
    from fed_tgan_amd.models.samplers import CondTables
    _, df, _, meta, vocabs, enc, tr, X = pc.small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), DEV, backend="hip", seed=3)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    real = df.iloc[:500]
    n = 700
    vals = eng.generate_decoded(n)
    assert vals.is_cuda and vals.dtype == torch.float64 and vals.shape == (n, len(meta["columns"]))
    eager = DevicePrivacy(real, meta, vocabs, DEV, ops=eng.ops, max_rows=n)
    graph = DevicePrivacy(real, meta, vocabs, DEV, ops=eng.ops, max_rows=n, graph=True)
    se = eager.score(vals)
    se2 = eager.score(vals)
    sg1 = graph.score(vals)
    sg2 = graph.score(vals)
    assert len(graph._graphs) == 1
    for other in (se2, sg1, sg2):      # a second run, a hipGraph replay and a second replay: bit-identical
        assert torch.equal(se.buf.view(torch.int64), other.buf.view(torch.int64))
        for x, y in zip(se.rows(), other.rows()):
            assert torch.equal(x, y)
    kinds = [pc.CAT if c["type"] == "categorical" else pc.CONT for c in meta["columns"]]
    coded = np.ascontiguousarray(np.asarray(enc)[:500], dtype=np.float64)
    want = pc.expected(coded, vals.cpu().numpy(), kinds)
    pc.assert_scores(se.floats(), want, "generated")
    dcr, nndr, i1 = (t.cpu().numpy() for t in se.rows())
    assert np.abs(dcr - want["dcr"]).max() <= pc.TOL and np.abs(nndr - want["nndr"]).max() <= pc.TOL
    assert i1.dtype == np.int32 and (i1 >= 0).all() and (i1 < 500).all()
    # the reference ops on the same device agree too (the -backend torch path)
    st = DevicePrivacy(real, meta, vocabs, DEV, ops=REF, max_rows=n).score(vals)
    pc.assert_scores(st.floats(), want, "reference ops")
    # LoadedGenerator.privacy: the same numbers as scoring its device_table by hand
    path = str(tmp_path / "g.pt")
    export_generator(path, eng, tr, CondTables.from_encoded(X, tr.layout), meta, vocabs, "Intrusion")
    by_hand = eager.score(load_generator(path, DEV, backend="hip", seed=9).device_table(n)).floats()
    assert load_generator(path, DEV, backend="hip", seed=9).privacy(real, n=n) == by_hand


CHECKED_SCRIPT = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {tests!r}]
from fed_tgan_amd.ops import native
from fed_tgan_amd.ops.hip import HipOps
from fed_tgan_amd.eval import DevicePrivacy
import privacy_cases as pc
L = native.require()
assert native.CHECKED and L.is_checked(), "checked library not loaded"
dev = torch.device("cuda:0")
_, df, _, meta, vocabs, enc, _, _ = pc.small_table()
ev = DevicePrivacy(df.iloc[:300], meta, vocabs, dev, ops=HipOps(dev), max_rows=200)
t = torch.from_numpy(np.ascontiguousarray(np.asarray(enc)[100:300], dtype=np.float64)).to(dev)
f = ev.score(t).floats()
native.check()
assert f["copies"] == 1.0 and f["dcr_min"] == 0.0, f
print("CLEAN", f)
"""


def test_checked_build_scores_a_clean_table():
    env = dict(os.environ, FEDTGAN_CHECKED="1")
    script = CHECKED_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert r.returncode == 0 and "CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
