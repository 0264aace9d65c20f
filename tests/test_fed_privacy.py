"""Federated privacy audit and guard on the CPU (torch ops): the shard merges against a numpy statement of their
contract, the sharded evaluator and guard against the pooled ones bit for bit, and the federation: the in-process
emulation, real processes over gloo, the refused combinations and the feature switched off."""
import os
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import fed_privacy_cases as fc
from fed_tgan_amd.eval import DevicePrivacy
from fed_tgan_amd.eval.fed_privacy import ShardedPrivacy, ShardPrivacy, merge_partials, shard_offsets
from fed_tgan_amd.eval.privacy import combine_bounds, table_bounds
from fed_tgan_amd.ops.ref import TorchOps

REF = TorchOps()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the merges
@pytest.mark.parametrize("n", fc.QUERY_COUNTS)
@pytest.mark.parametrize("k", fc.SHARD_COUNTS)
def test_merges_match_their_definition(k, n):
    parts, near, offsets = fc.merge_inputs(k, n, REF)
    got = fc.run_merge(REF, "cpu", parts, near, offsets)
    want = fc.numpy_merge(parts.numpy(), near.numpy(), offsets.numpy())
    for g, w, name in zip(got, want, ("d1", "d2", "i1", "owner", "by_client", "near", "near_owner")):
        assert np.array_equal(g.numpy(), w), (k, n, name)
    assert got[2].dtype == torch.int32 and got[3].dtype == torch.int32 and got[4].dtype == torch.int64


def test_merge_edge_cases():
    inf = float("inf")
    # two one-row shards holding the same record: each contributes d2 = +inf, the union d1 = d2 = 0 (NNDR 1)
    parts = torch.tensor([[[0.0, inf, 0.0]], [[0.0, inf, 0.0]]], dtype=torch.float64)
    d1, d2, i1, owner, by, _, _ = fc.run_merge(REF, "cpu", parts, torch.full((2, 1), -1, dtype=torch.int32),
                                               torch.tensor([0, 1]))
    assert (d1.item(), d2.item(), i1.item(), owner.item()) == (0.0, 0.0, 0, 0) and by.tolist() == [[1, 0], [1, 1]]
    # one real row overall: d2 = +inf; the shard without a candidate contributes nothing
    parts = torch.tensor([[[inf, inf, -1.0]], [[2.0, inf, 0.0]]], dtype=torch.float64)
    d1, d2, i1, owner, by, near, nown = fc.run_merge(REF, "cpu", parts, torch.tensor([[-1], [0]], dtype=torch.int32),
                                                     torch.tensor([0, 5]))
    assert (d1.item(), d2.item(), i1.item(), owner.item()) == (2.0, inf, 5, 1) and by.tolist() == [[0, 1], [0, 0]]
    assert near.item() == 5 and nown.item() == 1
    with pytest.raises(ValueError, match="64"):
        REF.nn_merge_shards(torch.zeros(65, 1, 3, dtype=torch.float64), torch.zeros(65, dtype=torch.int64),
                            *(torch.zeros(1) for _ in range(5)))
    with pytest.raises(ValueError, match="64"):
        shard_offsets([1] * 65, "cpu")


# ----------------------------------------------------------------------------- federated equals pooled
@pytest.mark.parametrize("n", fc.QUERY_COUNTS)
@pytest.mark.parametrize("k", fc.SHARD_COUNTS)
def test_federated_equals_pooled(k, n):
    fc.check_federated_equals_pooled(k, n, "cpu", REF)


def test_one_shard_is_the_pooled_evaluator():
    (shards, q, _, _), sharded, pooled = fc.evaluators(1, "cpu", REF)
    v = torch.from_numpy(q.copy())
    got, want = sharded.score(v), pooled.score(v)
    assert torch.equal(got.buf[:4], want.buf[:4]) and torch.equal(got._i1, want._i1)
    assert bool((got.owners() == 0).all()) and got.by_client()[0].tolist() == [len(q)]
    for a, b in zip(got.rows(), want.rows()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("k", (2, 8))
def test_clients_and_federator_halves(k):
    fc.check_merge_partials(k, 65, "cpu", REF)


def test_bounds_and_refusals():
    shards, _, _, _ = fc.sharded_case(3, REF)
    lo, hi = combine_bounds([table_bounds(s, fc.META) for s in shards])
    pooled = np.concatenate(shards)[:, fc.CONT_COLS]
    assert np.array_equal(lo, pooled.min(axis=0)) and np.array_equal(hi, pooled.max(axis=0))
    own = DevicePrivacy(shards[0], fc.META, [], "cpu", ops=REF, max_rows=4, baseline=False)
    same = DevicePrivacy(shards[0], fc.META, [], "cpu", ops=REF, max_rows=4, baseline=False,
                         bounds=table_bounds(shards[0], fc.META))
    assert torch.equal(own.lo, same.lo) and torch.equal(own.scale, same.scale) and torch.equal(own.r_cont, same.r_cont)
    with pytest.raises(ValueError, match="bounds"):
        DevicePrivacy(shards[0], fc.META, [], "cpu", ops=REF, bounds=(lo[:2], hi[:2]))
    with pytest.raises(ValueError, match="bounds"):
        ShardPrivacy(shards[0], fc.META, [], "cpu", None, 4, ops=REF)
    with pytest.raises(ValueError, match="date"):
        ShardPrivacy(shards[0], dict(fc.META, date_info={"c0": "%Y"}), [], "cpu", (lo, hi), 4, ops=REF)
    bad = shards[1].copy()
    bad[0, fc.CONT_COLS[0]] = np.nan
    with pytest.raises(ValueError, match="finite"):
        ShardedPrivacy([shards[0], bad], fc.META, [], "cpu", ops=REF)
    with pytest.raises(ValueError, match="shards"):
        ShardedPrivacy([], fc.META, [], "cpu", ops=REF)
    sp = ShardPrivacy(shards[0], fc.META, [], "cpu", (lo, hi), 4, ops=REF)
    with pytest.raises(ValueError, match="rows"):
        sp.search(torch.zeros(5, len(fc.KINDS), dtype=torch.float64))
    with pytest.raises(ValueError, match="partials"):
        merge_partials(torch.zeros(2, 4, 2, dtype=torch.float64), torch.zeros(2, dtype=torch.int64), ops=REF)


# ----------------------------------------------------------------------------- the guard
@pytest.mark.parametrize("k", fc.SHARD_COUNTS)
def test_guard_near_equals_pooled(k):
    fc.check_guard_near(k, "cpu", REF)


def test_guarded_table_equals_pooled():
    """The radius is the median DCR of a first unguarded pass; the pooled guard alone has to reject 20-80 % of the
    generated rows (asserted in guarded_tables), then both guards deliver the same table."""
    a, b, _ = fc.guarded_tables(torch.device("cpu"), "torch", None)
    assert a.shape == b.shape and torch.equal(a, b)


# ----------------------------------------------------------------------------- the federation
def test_emulated_federation_audit_and_guard(tmp_path):
    fc.check_emulated_federation(tmp_path, "torch", torch.device("cpu"))


def test_features_off_issue_nothing(tmp_path):
    from fed_tgan_amd.fed.local import run_local_emulation
    rt = run_local_emulation(fc.fed_config(tmp_path, epochs=1), 2, backend="torch", device=torch.device("cpu"))
    assert rt._audit is None and rt.privacy_rows == []
    assert "t_audit" not in rt.timer.last() and "t_generate" in rt.timer.last()
    assert sorted(os.listdir(tmp_path / "Intrusion_result")) == ["Intrusion_synthesis_epoch_0.csv"]


def test_gloo_processes_write_the_files(tmp_path):
    """two co-located client processes over gloo: the audit's and the guard's files"""
    import subprocess
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, "-m", "dtds.distributed", "-world_size", "2", "-colocated", "-epochs", "2",
                        "-backend", "torch", "-synthetic_rows", "300", "-n_sample", "201", "-batch_size", "100",
                        "-out_dir", str(tmp_path), "-quiet", "-privacy_every", "1", "-min_dcr", "0", "-guard_rows",
                        "120"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    res = tmp_path / "Intrusion_result"
    online = pd.read_csv(res / "privacy_online.csv")
    assert online["Epoch_No."].tolist() == [0, 1] and np.isfinite(online["DCR_p5"]).all()
    assert all(sum(int(x) for x in s.split()) == 201 for s in online["Nearest_by_client"])
    assert pd.read_csv(res / "Intrusion_guarded.csv").shape == (120, 42)


def test_refused_combinations_name_the_flag(tmp_path):
    from fed_tgan_amd.cli import main
    from fed_tgan_amd.fed.audit import refuse_unsupported
    from fed_tgan_amd.fed.local import run_local_emulation

    class HierComm:
        pass
    with pytest.raises(ValueError, match="-mode mdgan"):
        refuse_unsupported(fc.fed_config(tmp_path, privacy_every=1, mode="mdgan"))
    with pytest.raises(ValueError, match="-batched_clients on"):
        refuse_unsupported(fc.fed_config(tmp_path, min_dcr=0.5, batched_clients="on"))
    with pytest.raises(ValueError, match="-world_size N -local_clients K"):
        refuse_unsupported(fc.fed_config(tmp_path, min_dcr=0.0), HierComm())
    with pytest.raises(ValueError, match="min_dcr"):
        refuse_unsupported(fc.fed_config(tmp_path, min_dcr=-1.0))
    refuse_unsupported(fc.fed_config(tmp_path, mode="mdgan", batched_clients="on"), HierComm())     # both off: nothing
    # at start-up: the runtime's constructor, before any data is read
    with pytest.raises(RuntimeError, match="-batched_clients on"):
        run_local_emulation(fc.fed_config(tmp_path, privacy_every=1, batched_clients="on"), 2, backend="torch",
                            device=torch.device("cpu"))
    for bad in (["-mode", "mdgan"], ["-batched_clients", "on", "-local_clients", "2"],
                ["-world_size", "2", "-local_clients", "2"]):
        with pytest.raises(SystemExit):
            main(["-privacy_every", "1", "-backend", "torch", "-out_dir", str(tmp_path)] + bad)
