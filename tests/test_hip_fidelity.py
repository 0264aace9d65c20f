"""The fidelity evaluator's HIP kernels (csrc/kernels/fidelity.hip) against the plain-numpy brute force of
fidelity_cases.py and the reference ops (ops/ref.py).  Lattice tables, on which every term and sum is exact with or
without a fused multiply-add, are compared bit for bit; random continuous ones within privacy_cases.TOL (derived
there), the counts by a sandwich of the brute force's counts at radii (1 -+ TOL) times the oracle's."""
import numpy as np
import pytest
import torch

import fidelity_cases as fc
import privacy_cases as pc
from fed_tgan_amd.ops.ref import TorchOps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REF = TorchOps()
KS = (1, 5, 8)


@pytest.fixture(scope="module")
def hip():
    from fed_tgan_amd.ops import native
    from fed_tgan_amd.ops.hip import HipOps
    L = native.require()
    ops = HipOps(DEV, seed=1234)
    assert (ops.NN_QUERY_TILE, ops.NN_REF_TILE, ops.NN_CHUNK_ROWS) == (int(L.nn_query_tile()), int(L.nn_ref_tile()),
                                                                       int(L.nn_chunk_rows()))
    assert ops.FID_MAX_K == int(L.fid_max_k()) == REF.FID_MAX_K
    K = ops.NN_CHUNK_ROWS
    assert [ops.nn_topk_scratch(10, n, 5) for n in (1, K, K + 1, 2 * K + 7)] == [50, 50, 100, 150]
    assert [ops.nn_ball_scratch(10, n) for n in (1, K, K + 1, 2 * K + 7)] == [15, 15, 30, 45]
    return ops


def _shapes(hip, k):
    """every query-side size with two reference-side sizes and every reference-side size with two query-side sizes,
    around the query tile, the LDS tile and the chunk; and the sizes of the self passes, where the excluded index
    falls in every chunk position"""
    tq, tr, K = hip.NN_QUERY_TILE, hip.NN_REF_TILE, hip.NN_CHUNK_ROWS
    nqs = [1, 2, tq - 1, tq + 1, 3 * tq + 5]
    nrs = [k + 1, tr - 1, tr + 1, K - 1, K, K + 1, 2 * K + 7]
    pairs = [(nq, nr) for nq in nqs for nr in (tr + 1, K + 1)] + [(nq, nr) for nr in nrs for nq in (2, tq + 1)]
    return sorted(set(pairs)), [k + 1, tr + 1, tq + 1, K + 1, 2 * K + 7]


# ----------------------------------------------------------------------------- 1. lattice cases, bit for bit
@pytest.mark.parametrize("layout", ["cont", "cat", "small", "intrusion"])
def test_lattice_cases_bit_for_bit(hip, layout):
    """radii, counts and minima equal the brute force exactly: ties, copies and boundary hits included (the guard
    tails of every output and of the scratch are checked inside run_topk / run_ball / run_reduce)"""
    n_cont, n_cat = pc.LAYOUTS[layout]
    pairs = {}                  # a shape is computed once and serves every k that has it
    selfs = {}
    for k in KS:
        p, s = _shapes(hip, k)
        for shape in p:
            pairs.setdefault(shape, []).append(k)
        for n in s:
            selfs.setdefault(n, []).append(k)
    for (nq, nr), ks in sorted(pairs.items()):
        t = fc.lattice_packed(nq, nr, n_cont, n_cat, seed=nq * 7 + nr)
        fc.check_exact(hip, DEV, *t, ks, False, f"{layout} {nq}x{nr}", dist=fc.lattice_dist2)
    for n, ks in sorted(selfs.items()):
        t = fc.lattice_packed(n, n, n_cont, n_cat, seed=n, same=True)
        fc.check_exact(hip, DEV, *t, ks, True, f"{layout} self {n}", dist=fc.lattice_dist2)


def test_wide_rows_take_the_column_blocked_path(hip):
    n_cont, n_cat = pc.LAYOUTS["wide"]
    tq, K = hip.NN_QUERY_TILE, hip.NN_CHUNK_ROWS
    # (tq + 1, K + 1) at every k; (k + 2, k + 3) and a table of k + 3 rows against itself at k = 5
    for nq, nr, ks, same in ((tq + 1, K + 1, KS, False), (7, 8, (5,), False), (8, 8, (5,), True)):
        t = fc.lattice_packed(nq, nr, n_cont, n_cat, seed=nq + nr, same=same)
        fc.check_exact(hip, DEV, *t, ks, same, f"wide {nq}x{nr} same={same}", dist=fc.lattice_dist2)


# ----------------------------------------------------------------------------- 2. random continuous cases
@pytest.mark.parametrize("nq,nr,n_cont,n_cat,seed", [(600, 4103, 22, 20, 3), (257, 2049, 5, 4, 1), (300, 500, 1, 0, 2),
                                                     (513, 2055, 0, 1, 4)])
def test_random_continuous_cases(hip, nq, nr, n_cont, n_cat, seed):
    """Radii within TOL of the oracle's; the HIP count at the oracle's radii between the brute force's counts at radii
    (1 - TOL) and (1 + TOL) times them, per row, and dmin within TOL.  The sandwich has to be tight (lower == upper)
    on 99 % of the rows at least, so the test cannot pass vacuously."""
    k = 5
    q_cont, q_cat, r_cont, r_cat = fc.continuous_packed(nq, nr, n_cont, n_cat, seed)
    rel = lambda got, want: np.abs(got - want) / np.maximum(1.0, want)      # noqa: E731
    # the oracle's radii of the reference table (the reference ops, on this device) and of the queries
    for cont, cat, what in ((r_cont, r_cat, "rr"), (q_cont, q_cat, "ff")):
        want = fc.run_topk(REF, DEV, cont, cat, cont, cat, k, True)
        got = fc.run_topk(hip, DEV, cont, cat, cont, cat, k, True)
        assert np.isfinite(want).all() and np.isfinite(got).all()
        err = rel(got, want)
        print(f"{what} max rel err {err.max():.3e}")
        assert (err <= pc.TOL).all(), (what, float(err.max()))
        if what == "rr":
            rad = want
    d = pc.dist2(q_cont, q_cat, r_cont, r_cat)
    lower, _ = fc.ball(d, rad * (1.0 - pc.TOL))
    upper, want_min = fc.ball(d, rad * (1.0 + pc.TOL))
    cnt, dmin = fc.run_ball(hip, DEV, q_cont, q_cat, r_cont, r_cat, rad)
    loose = int((lower != upper).sum())
    print(f"{nq}x{nr}: sandwich loose on {loose} of {nq} rows; dmin max rel err {rel(dmin, want_min).max():.3e}")
    assert loose <= nq // 100
    assert ((lower <= cnt) & (cnt <= upper)).all(), np.nonzero((cnt < lower) | (cnt > upper))[0][:8]
    assert (rel(dmin, want_min) <= pc.TOL).all()
    # two runs are bit-identical
    again = fc.run_ball(hip, DEV, q_cont, q_cat, r_cont, r_cat, rad)
    assert again[0].tobytes() == cnt.tobytes() and again[1].tobytes() == dmin.tobytes()


# ----------------------------------------------------------------------------- 3. the copy identity
@pytest.mark.parametrize("k", KS)
def test_copy_identity(hip, k):
    """A row-permuted copy of a random continuous real table: every generated row lies exactly on the boundary of
    the balls of the k real rows whose k-th neighbour is its original, and at the centre of its own, whichever launch
    computed the distance and whichever the radius.  On the CPU with numpy: 1.0, 1.0, (k + 1) / k, 1.0."""
    m = hip.NN_CHUNK_ROWS + 40
    g = np.random.default_rng(17)
    real = np.concatenate([g.random((m, 6)), g.integers(0, 4, (m, 3)).astype(np.float64)], axis=1)
    kinds = [pc.CONT] * 6 + [pc.CAT] * 3
    fake = torch.from_numpy(real[g.permutation(m)]).to(DEV)
    f = fc.coded_evaluator(real, kinds, DEV, hip, k=k, max_rows=m).score(fake).floats()
    print(k, f)
    assert f["precision"] == 1.0 and f["recall"] == 1.0 and f["coverage"] == 1.0
    assert f["density"] == (k + 1) / k


# ----------------------------------------------------------------------------- 4. end to end
def test_evaluator_matches_reference_ops_end_to_end(hip):
    m, n = hip.NN_CHUNK_ROWS + 40, 3 * hip.NN_QUERY_TILE + 5
    real, fake, kinds = fc.lattice_table(m, n, seed=5)
    vals = torch.from_numpy(fake).to(DEV)
    eager = fc.coded_evaluator(real, kinds, DEV, hip, k=5, max_rows=n + 3)
    graph = fc.coded_evaluator(real, kinds, DEV, hip, k=5, max_rows=n + 3, graph=True)
    ref = fc.coded_evaluator(real, kinds, DEV, REF, k=5, max_rows=n + 3)
    se, se2, sg1, sg2, sr = eager.score(vals), eager.score(vals), graph.score(vals), graph.score(vals), ref.score(vals)
    assert len(graph._graphs) == 1
    want = fc.expected(real, fake, kinds, 5)
    fc.assert_scores_equal(se.floats(), want, "lattice table")
    fc.assert_scores_equal(sr.floats(), want, "lattice table, reference ops")
    fc.assert_rows_equal(se, want)
    for other in (se2, sg1, sg2, sr):      # a second run, a hipGraph replay and a second replay, the reference ops
        assert torch.equal(se.buf.view(torch.int64), other.buf.view(torch.int64))
        for x, y in zip(se.rows() + se.real_rows(), other.rows() + other.real_rows()):
            assert x.dtype == y.dtype and torch.equal(x, y)
    assert torch.equal(eager.rr, ref.rr) and np.array_equal(eager.rr.cpu().numpy(), want["rr"])
    assert np.array_equal(eager.ff[:n].cpu().numpy(), want["ff"])
