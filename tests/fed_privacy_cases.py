"""Shared cases of the federated-privacy tests (test_fed_privacy.py on the CPU with the torch ops,
test_hip_fed_privacy.py on the GPU): small mixed tables (5 continuous + 4 categorical columns) cut into K shards whose
sizes sit on both sides of the kernels' reference tile and chunk and include a one-row shard, with rows planted where
a merge of per-shard answers can go wrong, and the checks both backends run: the sharded evaluator / guard against the
pooled one on the concatenated shards, bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch

import privacy_cases as pc
from fed_tgan_amd.eval import DevicePrivacy, PrivacyGuard
from fed_tgan_amd.eval.fed_privacy import (ShardedGuard, ShardedPrivacy, ShardPrivacy, merge_partials, shard_offsets)
from fed_tgan_amd.eval.privacy import combine_bounds, table_bounds

CONT, CAT = pc.CONT, pc.CAT
KINDS = (CONT, CAT, CONT, CONT, CAT, CONT, CAT, CONT, CAT)
CONT_COLS = [j for j, k in enumerate(KINDS) if k == CONT]
CAT_COLS = [j for j, k in enumerate(KINDS) if k == CAT]
META = {"columns": [{"column_name": f"c{j}", "type": "categorical" if k == CAT else "continuous"}
                    for j, k in enumerate(KINDS)], "non_negative_cols": []}
SHARD_COUNTS = (1, 2, 3, 8)
QUERY_COUNTS = (1, 63, 65, 257)
MAX_ROWS = max(QUERY_COUNTS)


def shard_sizes(k: int, ops) -> list:
    """Row counts of k shards from the kernels' own tile sizes: a one-row shard, shards one row short of / past the
    LDS reference tile, and shards one row short of / past one reference chunk (two partials per query)."""
    tile, chunk = int(ops.NN_REF_TILE), int(ops.NN_CHUNK_ROWS)
    return {1: [chunk + 1],
            2: [chunk + 1, tile + 1],
            3: [tile + 1, 1, chunk - 1],
            8: [tile - 1, 1, tile + 1, chunk + 1, tile, chunk - 1, 2 * tile + 1, 5]}[k]


def sharded_case(k: int, ops, seed: int = 0):
    """(shards: k coded float64 tables, queries [MAX_ROWS, 9], plants: {name: query row}).  The first query rows are
    the planted ones, in the order of ``plants``, so the first n rows of the queries hold as many as fit:

    both     a copy of a record that two shards hold (k >= 2; else twice in the one shard): d1 = d2 = 0
    tie      two shards hold different records at distance exactly 1 (one categorical mismatch each, equal continuous
             values); the one with the lower global index has the HIGHER local index (k >= 2)
    second   the nearest record is in one shard, the second nearest in another, everything else is farther (k >= 2)
    single   a copy of a record only one shard holds: d1 = 0 < d2
    """
    g = np.random.default_rng(100 + seed)
    sizes = shard_sizes(k, ops)
    shards = []
    for m in sizes:
        t = np.zeros((m, len(KINDS)))
        t[:, CONT_COLS] = g.random((m, len(CONT_COLS))) * g.uniform(0.5, 2.0) + g.uniform(-1.0, 1.0)
        t[:, CAT_COLS] = g.integers(0, 4, (m, len(CAT_COLS)))
        shards.append(t)
    q = np.zeros((MAX_ROWS, len(KINDS)))
    q[:, CONT_COLS] = g.random((MAX_ROWS, len(CONT_COLS))) * 2.5 - 1.0
    q[:, CAT_COLS] = g.integers(0, 5, (MAX_ROWS, len(CAT_COLS)))
    pooled = np.concatenate(shards)
    copy = g.random(MAX_ROWS) < 0.2
    q[copy] = pooled[g.integers(0, len(pooled), MAX_ROWS)[copy]]
    big = [s for s in range(k) if sizes[s] >= 5]            # shards with room for planted records
    lo_s, hi_s = big[0], big[-1]
    plants = {}
    c0, c1, c2 = CAT_COLS[0], CAT_COLS[1], CAT_COLS[2]
    # both: a record of its own code, twice
    rec = shards[lo_s][2].copy()
    rec[c0] = 50
    shards[lo_s][2] = rec
    if k >= 2:
        shards[hi_s][0] = rec
    else:
        shards[lo_s][4] = rec
    q[0] = rec
    plants["both"] = 0
    row = 1
    if k >= 2:
        # tie: the lower shard's record at local index 3, the higher shard's at local index 1
        base = shards[lo_s][3].copy()
        base[c0] = 51
        a, b = base.copy(), base.copy()
        a[c1] = 7
        b[c2] = 8
        shards[lo_s][3], shards[hi_s][1] = a, b
        q[row] = base
        plants["tie"] = row
        row += 1
        # second: nearest in the higher shard, second nearest in the lower one, both far closer than anything else
        base = shards[hi_s][2].copy()
        base[c0] = 52
        span = pooled[:, CONT_COLS[0]].max() - pooled[:, CONT_COLS[0]].min()
        a, b = base.copy(), base.copy()
        a[CONT_COLS[0]] += 1e-3 * span
        b[CONT_COLS[0]] += 2e-3 * span
        shards[hi_s][2], shards[lo_s][1] = a, b
        q[row] = base
        plants["second"] = row
        row += 1
    rec = shards[hi_s][3 if sizes[hi_s] > 3 else 0].copy()
    rec[c0] = 53
    shards[hi_s][3 if sizes[hi_s] > 3 else 0] = rec
    q[row] = rec
    plants["single"] = row
    return shards, q, plants, (lo_s, hi_s)


def offsets_of(shards) -> np.ndarray:
    return np.concatenate([[0], np.cumsum([len(s) for s in shards])[:-1]]).astype(np.int64)


_CACHE = {}


def evaluators(k: int, dev, ops, graph: bool = False):
    """(case, ShardedPrivacy, pooled DevicePrivacy) per (k, device, graph), built once"""
    key = (k, str(dev), type(ops).__name__, bool(graph))
    if key not in _CACHE:
        case = sharded_case(k, ops)
        sharded = ShardedPrivacy(case[0], META, [], dev, max_rows=MAX_ROWS, graph=graph, ops=ops)
        pooled = DevicePrivacy(np.concatenate(case[0]), META, [], dev, ops=ops, max_rows=MAX_ROWS, baseline=False)
        _CACHE[key] = (case, sharded, pooled)
    return _CACHE[key]


def check_federated_equals_pooled(k: int, n: int, dev, ops, graph: bool = False):
    """ShardedPrivacy(shards).score(v) against DevicePrivacy(concat(shards), baseline=False).score(v), bit for bit,
    and the planted rows; returns the sharded scores"""
    (shards, q, plants, (lo_s, hi_s)), sharded, pooled = evaluators(k, dev, ops, graph)
    v = torch.from_numpy(q[:n].copy()).to(dev)
    got, want = sharded.score(v), pooled.score(v)
    tag = (k, n, graph)
    assert torch.equal(sharded.shards[0].lo, pooled.lo) and torch.equal(sharded.shards[0].scale, pooled.scale), tag
    for a, b, name in zip((got._d1, got._d2, got._i1), (want._d1, want._d2, want._i1), ("d1", "d2", "i1")):
        assert a.dtype == b.dtype and torch.equal(a, b), (tag, name, torch.nonzero(a != b).view(-1)[:8].tolist())
    assert torch.equal(got.buf[:4].view(torch.int64), want.buf[:4].view(torch.int64)), (tag, got.buf, want.buf)
    assert bool(torch.isnan(got.buf[4:]).all()), tag
    # owner is consistent with the offsets: offsets[owner] <= i1 < offsets[owner] + rows[owner]
    off = torch.from_numpy(offsets_of(shards))
    rows = torch.tensor([len(s) for s in shards])
    own, i1 = got.owners().cpu().long(), got._i1.cpu().long()
    assert own.dtype == torch.int64 and got.owners().dtype == torch.int32
    assert bool(((own >= 0) & (own < k)).all()), tag
    assert bool(((i1 >= off[own]) & (i1 < off[own] + rows[own])).all()), tag
    bc = got.by_client().cpu()
    assert bc.dtype == torch.int64 and tuple(bc.shape) == (2, k)
    assert bc[0].tolist() == torch.bincount(own, minlength=k).tolist() and int(bc[0].sum()) == n, \
        (tag, bc.tolist(), torch.bincount(own, minlength=k).tolist())
    assert torch.equal(sharded.owners(), got.owners()) and torch.equal(sharded.by_client(), got.by_client())
    d1, d2 = got._d1.cpu(), got._d2.cpu()
    glob = lambda s, local: int(off[s]) + local         # noqa: E731
    assert d1[plants["both"]] == 0.0 and d2[plants["both"]] == 0.0 and i1[plants["both"]] == glob(lo_s, 2), tag
    copies = [int(((torch.from_numpy(s)[None, :, :] == v.cpu()[:, None, :]).all(dim=2)).any(dim=1).sum())
              for s in shards]
    assert bc[1].tolist() == copies, (tag, bc[1].tolist(), copies)
    if k >= 2 and n > plants["tie"]:
        r = plants["tie"]
        assert d1[r] == 1.0 and d2[r] == 1.0 and i1[r] == glob(lo_s, 3) and own[r] == lo_s, tag
    if k >= 2 and n > plants["second"]:
        r = plants["second"]
        assert 0.0 < d1[r] < d2[r] < 1.0 and i1[r] == glob(hi_s, 2) and own[r] == hi_s, tag
        alone = ShardPrivacy(shards[hi_s], META, [], dev, sharded.bounds, MAX_ROWS, ops=ops).search(v)
        assert float(alone[r, 0]) == float(d1[r]) and float(alone[r, 1]) >= 1.0, tag      # its own second is far
    if n > plants["single"]:
        r = plants["single"]
        assert d1[r] == 0.0 and d2[r] > 0.0 and own[r] == hi_s, tag
    return got


def check_merge_partials(k: int, n: int, dev, ops):
    """the clients' halves one by one (bounds exchanged, ShardPrivacy.search) and the federator's half alone equal
    the in-process evaluator"""
    (shards, q, _, _), sharded, _ = evaluators(k, dev, ops)
    bounds = combine_bounds([table_bounds(s, META) for s in shards])
    assert all(np.array_equal(a, b) for a, b in zip(bounds, sharded.bounds))
    v = torch.from_numpy(q[:n].copy()).to(dev)
    parts = torch.stack([ShardPrivacy(s, META, [], dev, bounds, n, ops=ops).search(v).clone() for s in shards])
    got = merge_partials(parts, shard_offsets([len(s) for s in shards], dev), ops=ops)
    want = sharded.score(v)
    for a, b in zip((got._d1, got._d2, got._i1, got.owners(), got.by_client()),
                    (want._d1, want._d2, want._i1, want.owners(), want.by_client())):
        assert torch.equal(a, b), (k, n)
    assert torch.equal(got.buf[:4].view(torch.int64), want.buf[:4].view(torch.int64))


# ----------------------------------------------------------------------------- merge ops, backend against backend
def merge_inputs(k: int, n: int, ops, seed: int = 0):
    """(parts float64 [k, n, 3], near int32 [k, n], offsets int64 [k]) on the CPU: random partials over few distinct
    distances (ties across shards everywhere), zeros, one-row shards (d2 = +inf) and shards without a candidate"""
    g = np.random.default_rng(7 * k + n + seed)
    sizes = shard_sizes(k, ops)
    parts = np.zeros((k, n, 3))
    near = np.zeros((k, n), dtype=np.int32)
    for s, m in enumerate(sizes):
        a, b = g.integers(0, 4, n) * 0.25, g.integers(0, 4, n) * 0.25
        parts[s, :, 0], parts[s, :, 1] = np.minimum(a, b), np.maximum(a, b)
        parts[s, :, 2] = g.integers(0, m, n)
        if m == 1:
            parts[s, :, 1] = np.inf
        none = g.random(n) < 0.15
        parts[s, none] = (np.inf, np.inf, -1.0)
        near[s] = np.where(g.random(n) < 0.3, g.integers(0, m, n), -1)
    if k >= 2:
        parts[:, n - 1] = (np.inf, np.inf, -1.0)        # a row no shard has a candidate for
        near[:, n - 1] = -1
    return torch.from_numpy(parts), torch.from_numpy(near), torch.from_numpy(offsets_of([np.zeros(m) for m in sizes]))


def run_merge(ops, dev, parts, near, offsets, guard: int = 3):
    """both merges of ops -> the outputs on the CPU; output tails carry a value that has to survive"""
    k, n = near.shape
    f = lambda v, dt: torch.full((n + guard,), v, dtype=dt, device=dev)        # noqa: E731
    d1, d2 = f(-7.0, torch.float64), f(-7.0, torch.float64)
    i1, owner, near_out, owner2 = (f(-7, torch.int32) for _ in range(4))
    by_client = torch.full((2, k), 99, dtype=torch.int64, device=dev)           # overwritten, not added to
    off = offsets.to(dev)
    ops.nn_merge_shards(parts.to(dev), off, d1, d2, i1, owner, by_client)
    ops.nn_within_merge_shards(near.to(dev), off, near_out, owner2)
    for t in (d1, d2, i1, owner, near_out, owner2):
        assert bool((t[n:] == -7).all())
    return [t[:n].cpu() for t in (d1, d2, i1, owner)] + [by_client.cpu()] + [t[:n].cpu() for t in (near_out, owner2)]


def numpy_merge(parts: np.ndarray, near: np.ndarray, offsets: np.ndarray):
    """the contract from the definitions: the two smallest of the multiset of every shard's (d1, d2), the lowest global
    index at the smallest, per-client counts; the first shard with a hit"""
    k, n, _ = parts.shape
    d = np.concatenate([parts[:, :, 0], parts[:, :, 1]], axis=0)
    two = np.sort(d, axis=0)[:2]
    glob = np.where(parts[:, :, 2] >= 0, offsets[:, None] + parts[:, :, 2], np.inf)
    at = np.where(parts[:, :, 0] == two[0][None, :], glob, np.inf)
    none = np.isinf(two[0])
    i1 = np.where(none, -1, np.where(np.isinf(at.min(axis=0)), -1, at.min(axis=0))).astype(np.int64)
    owner = np.where(none, -1, at.argmin(axis=0))
    by = np.stack([np.bincount(owner[owner >= 0], minlength=k), (parts[:, :, 0] == 0).sum(axis=1)])
    hit = near >= 0
    first = np.where(hit.any(axis=0), hit.argmax(axis=0), -1)
    cols = np.arange(n)
    near_out = np.where(first >= 0, offsets[first.clip(0)] + near[first.clip(0), cols], -1)
    return two[0], two[1], i1, owner, by, near_out, first


# ----------------------------------------------------------------------------- the guard
def split_rows(table: np.ndarray, k: int):
    """k shards of a table in row order: the first one row long, the rest even"""
    cuts = [0, 1] + [1 + (len(table) - 1) * i // (k - 1) for i in range(1, k)] if k > 1 else [0, len(table)]
    return [table[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def check_guard_near(k: int, dev, ops):
    """ShardedGuard.near(v) equals PrivacyGuard(concat).near(v) at T = 0 and at a radius that rejects"""
    (shards, q, _, _), sharded, pooled = evaluators(k, dev, ops)
    v = torch.from_numpy(q.copy()).to(dev)
    T = float(pooled.score(v).rows()[0].median())
    assert T > 0
    for t in (0.0, T):
        want_flag, want = pooled.guard(t).near(v)
        for guard in (sharded.guard(t), ShardedGuard(shards, META, [], dev, min_dcr=t, ops=ops)):
            flag, near = guard.near(v)
            assert near.dtype == torch.int32 and torch.equal(near, want) and torch.equal(flag, want_flag), (k, t)
        assert 0 < int(want_flag.sum()) < len(q), (k, t)


def guarded_tables(dev, backend: str, use_graph, k: int = 3, n: int = 300, chunk: int = 128):
    """generate_decoded_guarded(n, guard) with the pooled guard and with the sharded one, each on a fresh engine from
    one seed, at the median DCR of a first unguarded pass -> (pooled table, sharded table, pooled reject share)"""
    import guard_cases as gc
    _, _, _, meta, vocabs, enc, _, _ = pc.small_table()
    real = np.asarray(enc, dtype=np.float64)
    shards = split_rows(real, k)
    assert sum(len(s) for s in shards) == len(real) and len(shards[0]) == 1
    out = []
    T = None
    for sharded in (False, True):
        torch.manual_seed(23)
        eng, _ = gc.make_engine(dev, backend, seed=9)
        if T is None:
            ev = DevicePrivacy(real, meta, vocabs, dev, ops=eng.ops, max_rows=n, baseline=False)
            T = float(ev.score(eng.generate_decoded(n)).rows()[0].median())
            torch.manual_seed(23)
            eng2, _ = gc.make_engine(dev, backend, seed=9)
            if hasattr(eng, "release"):
                eng.release()
            eng = eng2
        guard = (ShardedGuard(shards, meta, vocabs, dev, min_dcr=T, ops=eng.ops) if sharded
                 else PrivacyGuard(real, meta, vocabs, dev, min_dcr=T, ops=eng.ops))
        tab = eng.generate_decoded_guarded(n, guard, chunk=chunk, use_graph=use_graph)
        out.append((tab.cpu(), dict(eng.last_guard)))
        if hasattr(eng, "release"):
            eng.release()
    (a, la), (b, lb) = out
    share = la["rejected"] / la["generated"]
    print(f"T = {T!r}: the pooled guard rejected {la['rejected']} of {la['generated']} ({100 * share:.1f} %)")
    assert 0.2 <= share <= 0.8, share
    assert la == lb, (la, lb)
    return a, b, share


# ----------------------------------------------------------------------------- the federation
def fed_config(out_dir, **kw):
    from fed_tgan_amd.data.schema import intrusion_spec
    from fed_tgan_amd.fed.runtime import FedConfig
    from fed_tgan_amd.models.engine import EngineConfig
    base = dict(spec=intrusion_spec(), epochs=2, synthetic_rows=300, n_sample=200, out_dir=str(out_dir),
                gmm_backend="torch", engine=EngineConfig(batch_size=100), verbose=False, phase_detail=True)
    base.update(kw)
    return FedConfig(**base)


def pooled_evaluator(rt, dev, max_rows):
    """DevicePrivacy on the pooled synthetic shards of the runtime's federation, coded as the clients code them"""
    import pandas as pd
    frame = pd.concat(rt._synthetic_shards(range(rt.comm.n_clients)))
    return DevicePrivacy(frame, rt.global_meta, rt.vocabs, dev, ops=rt.engine.ops, max_rows=max_rows, baseline=False)


def check_emulated_federation(tmp, backend: str, dev, rows: int = 300, n_sample: int = 200, batch: int = 100):
    """Two client threads, two epochs: an audit every round, then the same federation with the guard at the median DCR
    the audit found.  The kept scores equal the pooled evaluator's bit for bit, the files exist with the right row
    counts, every guarded row scores pooled d1 > t2."""
    import os
    import pandas as pd
    from fed_tgan_amd.fed.local import run_local_emulation
    from fed_tgan_amd.models.engine import EngineConfig
    size = dict(synthetic_rows=rows, n_sample=n_sample, engine=EngineConfig(batch_size=batch))
    rt = run_local_emulation(fed_config(os.path.join(str(tmp), "a"), privacy_every=1, keep_audit_table=True, **size),
                             2, backend=backend, device=dev)
    assert [r["epoch"] for r in rt.privacy_rows] == [0, 1]
    for r in rt.privacy_rows:
        assert set(r) == {"epoch", "dcr_p5", "nndr_p5", "dcr_min", "copies", "nearest_by_client", "copies_by_client"}
        assert sum(r["nearest_by_client"]) == n_sample and len(r["copies_by_client"]) == 2
    assert "t_audit" in rt.timer.last()
    epoch, table, scores = rt._audit.kept
    assert epoch == 1 and tuple(table.shape) == (n_sample, 42)
    pooled = pooled_evaluator(rt, dev, 1024)
    assert pooled.n_real == 2 * rows
    want = pooled.score(table)
    assert torch.equal(scores._d1, want._d1) and torch.equal(scores._d2, want._d2) and torch.equal(scores._i1, want._i1)
    assert torch.equal(scores.buf[:4].view(torch.int64), want.buf[:4].view(torch.int64))
    assert rt.privacy_rows[1]["dcr_p5"] == scores.floats()["dcr_p5"]
    online = pd.read_csv(os.path.join(str(tmp), "a", "Intrusion_result", "privacy_online.csv"))
    assert len(online) == 2 and online["Epoch_No."].tolist() == [0, 1]
    assert not os.path.exists(os.path.join(str(tmp), "a", "Intrusion_result", "Intrusion_guarded.csv"))
    T = float(scores.rows()[0].median())
    assert T > 0
    if hasattr(rt, "close"):
        rt.close()
    rt = run_local_emulation(fed_config(os.path.join(str(tmp), "b"), privacy_every=2, min_dcr=T, guard_rows=150,
                                        keep_audit_table=True, **size), 2, backend=backend, device=dev)
    assert [r["epoch"] for r in rt.privacy_rows] == [1]
    res = os.path.join(str(tmp), "b", "Intrusion_result")
    assert len(pd.read_csv(os.path.join(res, "privacy_online.csv"))) == 1
    guarded = pd.read_csv(os.path.join(res, "Intrusion_guarded.csv"))
    assert guarded.shape == (150, 42)
    lg = rt._audit.last_guard
    print(f"T = {T!r}: {lg}")
    assert lg["kept"] == 150 and lg["rejected"] > 0
    tab = rt._audit.kept_guarded
    pooled = pooled_evaluator(rt, dev, 1024)
    pooled.score(tab)
    assert bool((pooled.d1[:150] > T * T).all())
    flagged, _ = pooled.guard(T).near(tab)
    assert not bool(flagged.any())
    if hasattr(rt, "close"):
        rt.close()
