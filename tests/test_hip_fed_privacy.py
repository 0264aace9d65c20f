"""Federated privacy audit and guard on the HIP backend: the two shard-merge kernels against their torch twins on every
output, the sharded evaluator and guard against the pooled ones bit for bit (eager and replayed as a hipGraph), and the
two-client in-process federation."""
import numpy as np
import pytest
import torch

import fed_privacy_cases as fc
from fed_tgan_amd.ops.ref import TorchOps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REF = TorchOps()


@pytest.fixture(scope="module")
def hip():
    from fed_tgan_amd.ops import native
    from fed_tgan_amd.ops.hip import HipOps
    native.require()
    return HipOps(DEV, seed=1234)


# ----------------------------------------------------------------------------- kernels vs twins
@pytest.mark.parametrize("k", fc.SHARD_COUNTS)
def test_merge_kernels_equal_their_twins(hip, k):
    assert (hip.NN_REF_TILE, hip.NN_CHUNK_ROWS, hip.NN_MAX_SHARDS) == (REF.NN_REF_TILE, REF.NN_CHUNK_ROWS,
                                                                       REF.NN_MAX_SHARDS)
    for n in fc.QUERY_COUNTS:
        parts, near, offsets = fc.merge_inputs(k, n, hip)
        got = fc.run_merge(hip, DEV, parts, near, offsets)
        want = fc.run_merge(REF, "cpu", parts, near, offsets)
        for g, w, name in zip(got, want, ("d1", "d2", "i1", "owner", "by_client", "near", "near_owner")):
            assert g.dtype == w.dtype and torch.equal(g, w), (k, n, name)


def test_merge_kernels_at_the_shard_limit_and_on_searched_partials(hip):
    """64 shards (the limit; 65 is refused), and the partials of real searches: HIP's own nn_top2 / nn_within answers
    of the planted case folded by the kernel and by the twin"""
    k, n = hip.NN_MAX_SHARDS, 257
    g = np.random.default_rng(5)
    parts = torch.from_numpy(np.sort(g.integers(0, 3, (k, n, 2)).astype(np.float64) * 0.5, axis=2))
    parts = torch.cat([parts, torch.from_numpy(g.integers(0, 9, (k, n, 1)).astype(np.float64))], dim=2).contiguous()
    near = torch.from_numpy(np.where(g.random((k, n)) < 0.02, g.integers(0, 9, (k, n)), -1).astype(np.int32))
    offsets = torch.arange(k, dtype=torch.int64) * 9
    for a, b in zip(fc.run_merge(hip, DEV, parts, near, offsets), fc.run_merge(REF, "cpu", parts, near, offsets)):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match="64"):
        hip.nn_merge_shards(torch.zeros(65, 4, 3, dtype=torch.float64, device=DEV),
                            torch.zeros(65, dtype=torch.int64, device=DEV),
                            torch.zeros(4, dtype=torch.float64, device=DEV),
                            torch.zeros(4, dtype=torch.float64, device=DEV),
                            torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV),
                            torch.zeros(2, 65, dtype=torch.int64, device=DEV))
    (shards, q, _, _), sharded, _ = fc.evaluators(8, DEV, hip)
    v = torch.from_numpy(q.copy()).to(DEV)
    parts = torch.stack([s.search(v).clone() for s in sharded.shards]).cpu()
    t2 = torch.tensor([0.3], dtype=torch.float64, device=DEV)
    near = torch.stack([s.within(v, t2).clone() for s in sharded.shards]).cpu()
    assert int((near >= 0).sum()) > 0
    for a, b in zip(fc.run_merge(hip, DEV, parts, near, sharded.offsets.cpu()),
                    fc.run_merge(REF, "cpu", parts, near, sharded.offsets.cpu())):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- federated equals pooled
@pytest.mark.parametrize("k", fc.SHARD_COUNTS)
def test_federated_equals_pooled(hip, k):
    for n in fc.QUERY_COUNTS:
        fc.check_federated_equals_pooled(k, n, DEV, hip)


@pytest.mark.parametrize("k", (1, 3, 8))
def test_replayed_equals_eager(hip, k):
    for n in (65, 257):
        eager = fc.check_federated_equals_pooled(k, n, DEV, hip)
        for _ in range(2):          # the capture's own pass, then a replay of it
            replayed = fc.check_federated_equals_pooled(k, n, DEV, hip, graph=True)
            for a, b in zip((eager._d1, eager._d2, eager._i1, eager.owners(), eager.by_client()),
                            (replayed._d1, replayed._d2, replayed._i1, replayed.owners(), replayed.by_client())):
                assert torch.equal(a, b), (k, n)
            assert torch.equal(eager.buf[:4].view(torch.int64), replayed.buf[:4].view(torch.int64)), (k, n)


def test_clients_and_federator_halves(hip):
    fc.check_merge_partials(3, 65, DEV, hip)


# ----------------------------------------------------------------------------- the guard
@pytest.mark.parametrize("k", fc.SHARD_COUNTS)
def test_guard_near_equals_pooled(hip, k):
    fc.check_guard_near(k, DEV, hip)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_guarded_table_equals_pooled(use_graph):
    a, b, _ = fc.guarded_tables(DEV, "hip", use_graph)
    assert a.shape == b.shape and torch.equal(a, b)


# ----------------------------------------------------------------------------- the federation
def test_emulated_federation_audit_and_guard(tmp_path):
    from fed_tgan_amd.ops import native
    native.require()
    fc.check_emulated_federation(tmp_path, "hip", DEV, rows=1000, n_sample=600, batch=500)
