"""The similarity evaluator's HIP kernels (csrc/kernels/similarity.hip) against the reference ops (ops/ref.py) and,
end to end, against the CPU evaluator on the written CSV.  Tolerances as in test_similarity_device.py
(similarity_cases.py): W1 abs <= 1e-10; JSD abs <= 1e-9 where the reference is >= 1e-3, else both <= 1e-7."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import similarity_cases as sc
from fed_tgan_amd.eval.device import DeviceSimilarity
from fed_tgan_amd.eval.similarity import column_similarity, stat_sim
from fed_tgan_amd.ops.ref import TorchOps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = TorchOps()
INF = float("inf")


@pytest.fixture(scope="module")
def hip():
    from fed_tgan_amd.ops import native
    from fed_tgan_amd.ops.hip import HipOps
    native.require()
    return HipOps(DEV, seed=1234)


def _i32(v, device=DEV):
    return torch.tensor(list(v), dtype=torch.int32, device=device)


# ----------------------------------------------------------------------------- sort
def _sort_input(kind, cols, n, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        x = torch.randn(cols, n, generator=g, dtype=torch.float64)
    elif kind == "constant":
        x = torch.full((cols, n), 2.5, dtype=torch.float64)
    elif kind == "ascending":
        x = torch.arange(n, dtype=torch.float64).repeat(cols, 1) - 7.0
    elif kind == "descending":
        x = -torch.arange(n, dtype=torch.float64).repeat(cols, 1)
    elif kind == "ints":
        x = torch.randint(0, 8, (cols, n), generator=g).double()
    else:       # random with +inf sentinels (and both zeros)
        x = torch.randn(cols, n, generator=g, dtype=torch.float64)
        x[torch.rand(cols, n, generator=g) < 0.2] = INF
        x[torch.rand(cols, n, generator=g) < 0.05] = 0.0
        x[torch.rand(cols, n, generator=g) < 0.05] = -0.0
    return x


@pytest.mark.parametrize("kind", ["random", "constant", "ascending", "descending", "ints", "sentinels"])
def test_sort_matches_torch_sort(hip, kind):
    T = hip.SIM_SORT_TILE
    assert T == int(hip.L.sim_sort_tile())
    seed = 0
    for n in (1, 2, T - 1, T, T + 1, 3 * T + 5, 5 * T - 1, 8 * T):
        for cols in (1, 3):
            seed += 1
            x = _sort_input(kind, cols, n, seed)
            pad = 3                                        # the key rows are longer than n: the tail stays untouched
            keys = torch.full((cols, n + pad), -123.0, dtype=torch.float64)
            keys[:, :n] = x
            a, b = keys.to(DEV), keys.to(DEV)
            hip.sim_sort(a, n, torch.empty_like(a))
            hip.sim_sort(b, n, torch.zeros_like(b))
            want = torch.sort(x, dim=1).values
            assert bool((a[:, :n].cpu() == want).all()), (kind, n, cols)
            assert bool((a[:, n:] == -123.0).all()), (kind, n, cols)
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (kind, n, cols)      # two runs: bit-identical


# ----------------------------------------------------------------------------- prepare
def _ulp_diff(a, b):
    ia, ib = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return (ia - ib).abs()


@pytest.mark.parametrize("rows", [1, 257, 1500])      # 256-thread workgroups: 257 spills one row into a second one
@pytest.mark.parametrize("wide_vocab", [False, True])  # True: the count table exceeds the LDS histogram (global atomics)
def test_prepare_matches_reference(hip, rows, wide_vocab):
    g = torch.Generator().manual_seed(rows)
    kinds = [REF.SIM_PLAIN, REF.SIM_CAT, REF.SIM_NONNEG, REF.SIM_CAT, REF.SIM_PLAIN, REF.SIM_CAT, REF.SIM_NONNEG]
    slots = [0, 0, 1, 1, 2, 2, 3]
    vocab = [5, 40, 3000 if wide_vocab else 7]
    width = max(vocab) + 2                                 # (extra slots past the vocabularies stay zero)
    vals = torch.randn(rows, len(kinds), generator=g, dtype=torch.float64)
    for c, k in enumerate(kinds):
        if k == REF.SIM_CAT:
            vals[:, c] = torch.randint(0, vocab[slots[c]], (rows,), generator=g).double()
        elif k == REF.SIM_NONNEG:
            vals[:, c] = torch.rand(rows, generator=g, dtype=torch.float64) * 12.0 - 1.0
    # what the CSV carries no number for: NaN, +-inf, and a non-negative code whose exp underflows (-1 -> blank);
    # codes outside the vocabulary are ignored
    vals[0, 0] = float("nan")
    vals[rows // 2, 4] = -INF
    vals[rows - 1, 2] = -800.0
    vals[rows // 3, 6] = INF
    vals[rows - 1, 1] = 5.0
    vals[0, 3] = -1.0
    vals[rows // 2, 5] = float("nan")
    n_cont, n_cat = 4, 3

    def run(ops, dev):
        keys = torch.full((n_cont, rows + 2), -5.0, dtype=torch.float64, device=dev)
        valid = torch.full((n_cont,), 99, dtype=torch.int32, device=dev)
        counts = torch.full((n_cat, width), 99, dtype=torch.int32, device=dev)
        ops.sim_prepare(vals.to(dev), _i32(kinds, dev), _i32(slots, dev), _i32(vocab, dev), keys, valid, counts)
        return keys.cpu(), valid.cpu(), counts.cpu()

    hk, hv, hc = run(hip, DEV)
    rk, rv, rc = run(REF, "cpu")
    assert torch.equal(hc, rc)
    assert torch.equal(hv, rv)
    assert int(hc.sum()) == 3 * rows - 3                   # one ignored code in each categorical column
    for s in (0, 2):        # plain columns: bit-equal
        assert torch.equal(hk[s].view(torch.int64), rk[s].view(torch.int64))
    # exp-decoded columns: the sentinels in the same places; the device's exp and numpy's may differ in the last
    # place, so a key exp(x) - 1 >= 1 (a binade at most one below exp(x)'s: the subtraction is exact) is within
    # 2 ulp; below that the subtraction cancels leading bits and the same difference is worth more ulps of the
    # smaller key, so there the bound is 2 ulp of exp(x) < 2, i.e. 2 * 2^-52 absolute.  Measured on an MI355X over
    # 200,000 codes in (-1, 12): the two exps differ in the last place for 8 % of them; keys >= 1 differ by at most
    # 2 ulp, keys in (0, 1) by at most 2^-52 absolute (1 ulp of exp(x); up to 512 ulp of a key near zero), keys <= 0
    # (-0.0 after the ceil, or the sentinel) not at all
    for s in (1, 3):
        assert torch.equal(torch.isinf(hk[s]), torch.isinf(rk[s]))
        big = torch.isfinite(rk[s]) & (rk[s] >= 1.0)
        small = torch.isfinite(rk[s]) & (rk[s] < 1.0)
        assert int(big.sum()) + int(small.sum()) >= rows - 1
        if big.any():
            assert int(_ulp_diff(hk[s][big], rk[s][big]).max()) <= 2
        if small.any():
            assert float((hk[s][small] - rk[s][small]).abs().max()) <= 2.0 * 2.0 ** -52
    assert bool((hk[:, rows:] == -5.0).all())


# ----------------------------------------------------------------------------- W1 / JSD
def _w1_both(hip, real_rows, fake_rows):
    """rows of unsorted values (lists / tensors, possibly with +inf sentinels in fake) -> (hip, reference) W1"""
    nc = len(real_rows)
    ldr, ldf = max(len(r) for r in real_rows), max(len(f) for f in fake_rows)
    real = torch.full((nc, ldr), INF, dtype=torch.float64)
    fake = torch.full((nc, ldf), INF, dtype=torch.float64)
    for c in range(nc):
        real[c, :len(real_rows[c])] = torch.as_tensor(real_rows[c], dtype=torch.float64)
        fake[c, :len(fake_rows[c])] = torch.as_tensor(fake_rows[c], dtype=torch.float64)
    real, fake = torch.sort(real, dim=1).values, torch.sort(fake, dim=1).values
    n_real = _i32([len(r) for r in real_rows], "cpu")
    n_fake = torch.isfinite(fake).sum(1).to(torch.int32)
    want = torch.zeros(nc, dtype=torch.float64)
    REF.sim_w1(real, n_real, fake, n_fake, ldf, want)
    got = torch.full((nc,), -1.0, dtype=torch.float64, device=DEV)
    part = torch.zeros(hip.sim_w1_part(nc, ldr + ldf), dtype=torch.float64, device=DEV)
    hip.sim_w1(real.to(DEV), n_real.to(DEV), fake.to(DEV), n_fake.to(DEV), ldf, got, part)
    got2 = torch.full((nc,), -1.0, dtype=torch.float64, device=DEV)
    hip.sim_w1(real.to(DEV), n_real.to(DEV), fake.to(DEV), n_fake.to(DEV), ldf, got2, part)
    assert torch.equal(got.view(torch.int64), got2.view(torch.int64))
    return got.cpu(), want


def test_w1_sizes_and_ties(hip):
    T = hip.SIM_SORT_TILE
    g = torch.Generator().manual_seed(5)
    for n_r, m in ((1, 1), (1, T + 1), (T + 1, 1), (3 * T + 5, 2 * T - 1)):
        real = [torch.randn(n_r, generator=g, dtype=torch.float64) * 3.0,
                torch.randint(0, 8, (n_r,), generator=g).double(),            # heavy ties
                torch.full((n_r,), 4.0, dtype=torch.float64)]                 # constant real column: scale 1
        fake = [torch.randn(m, generator=g, dtype=torch.float64) * 5.0 + 1.0,    # values outside the real range
                torch.randint(-2, 11, (m,), generator=g).double(),
                torch.randn(m, generator=g, dtype=torch.float64) + 4.0]
        # every fake value ties a real value
        real.append(torch.randn(n_r, generator=g, dtype=torch.float64))
        fake.append(real[-1][torch.randint(0, n_r, (m,), generator=g)])
        got, want = _w1_both(hip, real, fake)
        assert bool(torch.isfinite(want).all())
        assert float((got - want).abs().max()) <= sc.W1_TOL, (n_r, m, got, want)
    # the fourth column against itself: exactly the same points on both sides
    got, want = _w1_both(hip, [real[3]], [real[3]])
    assert float(got[0]) == 0.0 and float(want[0]) == 0.0


def test_w1_without_valid_fake_values_is_nan(hip):
    got, want = _w1_both(hip, [[0.0, 1.0, 2.0], [0.0, 1.0, 2.0]], [[INF, INF, INF, INF], [0.5, INF, 1.5, INF]])
    assert np.isnan(float(got[0])) and np.isnan(float(want[0]))
    assert abs(float(got[1]) - float(want[1])) <= sc.W1_TOL and float(want[1]) > 0.0


def test_jsd_matches_reference(hip):
    g = torch.Generator().manual_seed(9)
    rows = []
    for width in (1, 3, 70, 300, 1000):         # 300 / 1000: more slots than the workgroup has threads
        r = torch.randint(0, 50, (width,), generator=g)
        f = torch.randint(0, 50, (width,), generator=g)
        r[torch.rand(width, generator=g) < 0.3] = 0      # vocabulary entries the real table lacks (fake-only categories)
        f[torch.rand(width, generator=g) < 0.3] = 0      # real categories the fake table misses (counted twice)
        r[0] = max(int(r[0]), 1)
        rows.append((r, f))
    rows.append((torch.tensor([3, 0, 9, 0]), torch.tensor([0, 7, 0, 2])))     # no real category in the fake column: 1
    rows.append((torch.tensor([3, 1, 9, 4]), torch.tensor([0, 0, 0, 0])))     # an empty fake column: 1
    rows.append((torch.tensor([3, 1, 9, 4]), torch.tensor([6, 2, 18, 8])))    # the same frequencies: ~0
    width = max(len(r) for r, _ in rows)
    rc = torch.zeros(len(rows), width, dtype=torch.int32)
    fc = torch.zeros(len(rows), width, dtype=torch.int32)
    for i, (r, f) in enumerate(rows):
        rc[i, :len(r)], fc[i, :len(f)] = r.int(), f.int()
    want = torch.zeros(len(rows), dtype=torch.float64)
    REF.sim_jsd(rc, fc, want)
    got = torch.full((len(rows),), -1.0, dtype=torch.float64, device=DEV)
    hip.sim_jsd(rc.to(DEV), fc.to(DEV), got)
    got2 = torch.full((len(rows),), -1.0, dtype=torch.float64, device=DEV)
    hip.sim_jsd(rc.to(DEV), fc.to(DEV), got2)
    assert torch.equal(got.view(torch.int64), got2.view(torch.int64))
    got = got.cpu()
    assert float(want[-3]) == 1.0 and float(want[-2]) == 1.0 and float(got[-3]) == 1.0 and float(got[-2]) == 1.0
    assert float(want[-1]) <= sc.JSD_ZERO_TOL and float(got[-1]) <= sc.JSD_ZERO_TOL
    big = want >= sc.JSD_FLOOR
    assert int(big.sum()) >= 6                  # (a one-slot column scores 0 or 1 by construction)
    assert float((got - want).abs()[big].max()) <= sc.JSD_TOL, (got, want)


def test_mean_of_columns(hip):
    s = torch.tensor([0.0, 0.0, 0.25, 0.5, 0.125, 1.0, 3.0], dtype=torch.float64, device=DEV)
    hip.sim_mean(s, 3, 2)
    assert s[:2].tolist() == [(0.25 + 0.5 + 0.125) / 3, 2.0]
    s = torch.tensor([0.0, 0.0, 0.25], dtype=torch.float64, device=DEV)
    hip.sim_mean(s, 1, 0)
    assert float(s[0]) == 0.25 and np.isnan(float(s[1]))


@pytest.mark.parametrize("name", sc.CASES)
def test_cases_match_cpu_evaluator(hip, name):
    """the CPU file's cases, moved to the device"""
    real, vals, meta, vocabs, cats = sc.case(name)
    sim = DeviceSimilarity(real, meta, vocabs, DEV, ops=hip, max_rows=len(vals))
    scores = sim.score(torch.from_numpy(vals.copy()).to(DEV))
    want_cols, want_avg = sc.expected(name)
    sc.assert_scores(scores.columns(), scores.floats(), want_cols, want_avg, name)
    ref = DeviceSimilarity(real, meta, vocabs, "cpu", max_rows=len(vals)).score(torch.from_numpy(vals.copy()))
    sc.assert_scores(scores.columns(), scores.floats(), ref.columns(), ref.floats(), name + " (reference ops)")


# ----------------------------------------------------------------------------- end to end
def test_generated_table_end_to_end(hip, tmp_path):
    from fed_tgan_amd.data.decode import csv_layout
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.samplers import CondTables
    from fed_tgan_amd.utils import csvio
    spec, df, _, meta, vocabs, _, tr, X = sc.small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), DEV, backend="hip", seed=3)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    real = sc.through_csv(df.iloc[:500])
    n = 700
    vals = eng.generate_decoded(n)
    assert vals.is_cuda and vals.dtype == torch.float64 and vals.shape == (n, len(meta["columns"]))
    eager = DeviceSimilarity(real, meta, vocabs, DEV, ops=eng.ops, max_rows=n)
    graph = DeviceSimilarity(real, meta, vocabs, DEV, ops=eng.ops, max_rows=n, graph=True)
    se = eager.score(vals)
    sg1 = graph.score(vals)
    sg2 = graph.score(vals)
    assert len(graph._graphs) == 1
    for other in (sg1, sg2):        # hipGraph replay vs eager launches, and two replays: bit-identical
        assert torch.equal(se.buf.view(torch.int64), other.buf.view(torch.int64))
    path = str(tmp_path / "fake.csv")
    csvio.write_layout(path, vals.cpu().numpy(), csv_layout(meta, vocabs))
    fake = pd.read_csv(path)
    sc.assert_scores(se.columns(), se.floats(), column_similarity(real, fake, spec.categorical_list),
                     stat_sim(real, fake, spec.categorical_list), "generated")
    # a table in another buffer goes through the same evaluator (a graph of its own)
    sg3 = graph.score(vals.clone())
    assert torch.equal(se.buf.view(torch.int64), sg3.buf.view(torch.int64))


CHECKED_SCRIPT = r"""
import sys, torch
sys.path[:0] = [{root!r}, {tests!r}]
from fed_tgan_amd.ops import native
from fed_tgan_amd.ops.hip import HipOps
from fed_tgan_amd.eval.device import DeviceSimilarity
import similarity_cases as sc
L = native.require()
assert native.CHECKED and L.is_checked(), "checked library not loaded"
dev = torch.device("cuda:0")
real, vals, meta, vocabs, cats = sc.case("plain")
sim = DeviceSimilarity(real, meta, vocabs, dev, ops=HipOps(dev), max_rows=len(vals))
t = torch.from_numpy(vals.copy()).to(dev)
clean = sim.score(t).floats()
print("CLEAN", clean)
j = [c["column_name"] for c in meta["columns"]].index(cats[0])
t[5, j] = 100000.0          # a code outside the vocabulary: flagged and ignored, never used as an index
try:
    sim.score(t)
except RuntimeError as e:
    print("CHECK:", e)
    sys.exit(0)
sys.exit(3)
"""


def test_checked_build_flags_a_code_outside_the_vocabulary():
    env = dict(os.environ, FEDTGAN_CHECKED="1")
    script = CHECKED_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert r.returncode == 0 and "CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "categorical code outside its vocabulary" in r.stdout, r.stdout[-2000:]


# ----------------------------------------------------------------------------- one-GPU federation
def _fed_cfg(out, **kw):
    from fed_tgan_amd.data.schema import intrusion_spec
    from fed_tgan_amd.fed.runtime import FedConfig
    from fed_tgan_amd.models.engine import EngineConfig
    base = dict(spec=intrusion_spec(), epochs=2, synthetic_rows=4000, n_sample=3000, out_dir=str(out), backend="hip",
                gmm_backend="torch", engine=EngineConfig(batch_size=500), verbose=False)
    base.update(kw)
    return FedConfig(**base)


def _one_client_run(out, **kw):
    from fed_tgan_amd.fed.runtime import FedRuntime
    from fed_tgan_amd.parallel.comm import Comm
    rt = FedRuntime(_fed_cfg(out, **kw), Comm(0, 1, [0], "gloo", device=DEV), DEV)
    rt.initialize()
    rt.fit()
    torch.cuda.synchronize()
    res = out / "Intrusion_result"
    return rt, res, [(res / f"Intrusion_synthesis_epoch_{e}.csv").read_bytes() for e in range(2)]


def _check_online(out, res):
    from fed_tgan_amd.data.schema import intrusion_spec
    from fed_tgan_amd.eval.similarity import similarity_table
    online = pd.read_csv(res / "similarity_online.csv", float_precision="round_trip")
    assert list(online.columns) == ["Epoch_No.", "Avg_JSD", "Avg_WD"] and online["Epoch_No."].tolist() == [0, 1]
    want = similarity_table(str(out / "data" / "raw" / "Intrusion_train.csv"),
                            [str(res / f"Intrusion_synthesis_epoch_{e}.csv") for e in range(2)],
                            intrusion_spec().categorical_list)
    for e in range(2):
        assert want["Avg_JSD"][e] >= sc.JSD_FLOOR
        assert abs(online["Avg_JSD"][e] - want["Avg_JSD"][e]) <= sc.JSD_TOL, (e, online, want)
        assert abs(online["Avg_WD"][e] - want["Avg_WD"][e]) <= sc.W1_TOL, (e, online, want)


@pytest.fixture(scope="module")
def unscored_run(tmp_path_factory):
    """the run every scored one is compared with: eval_every == 0 (one client: deterministic in the seed)"""
    out = tmp_path_factory.mktemp("fed_off")
    rt, res, csvs = _one_client_run(out)
    assert "similarity_online.csv" not in os.listdir(res)
    return csvs, rt.engine.flat.clone(), rt.engine.ops.ctr.clone()


# the three places a round's table first exists on the federator: sample_round unpipelined, sample_round with the
# generation on its side stream, and the hand-off deferred past the next round's training issue
@pytest.mark.parametrize("pipe,defer", [(False, False), (True, False), (True, True)],
                         ids=["unpipelined", "pipelined", "deferred"])
def test_gpu_federation_scores_every_round(tmp_path, unscored_run, pipe, defer):
    """every round scored on the device: the online table equals the CPU evaluator on the epoch CSVs, and those, the
    trained model and the Philox counter equal the run without scoring (it draws no random number and does not
    disturb generation)"""
    rt, res, csvs = _one_client_run(tmp_path, eval_every=1, dump_real=True, pipeline_sample=pipe, defer_handoff=defer,
                                    metrics_log=str(tmp_path / "m.jsonl"))
    assert rt.engine.ops.name == "hip" and rt._pipe == pipe
    c0, f0, k0 = unscored_run
    assert csvs == c0
    assert torch.equal(rt.engine.flat, f0) and torch.equal(rt.engine.ops.ctr, k0)
    _check_online(tmp_path, res)
    import json
    with open(tmp_path / "m.jsonl") as f:
        sims = [r for r in map(json.loads, f) if "avg_jsd" in r]
    assert [r["epoch"] for r in sims] == [0, 1]


def test_gpu_emulated_clients_gathered_table_is_scored(tmp_path):
    """two emulated clients on one GPU: each generates its share, the federator scores the gathered device table"""
    from fed_tgan_amd.fed.local import run_local_emulation
    rt = run_local_emulation(_fed_cfg(tmp_path, shard_mode="iid", eval_every=1, dump_real=True), 2, backend="hip",
                             device=DEV)
    assert rt.engine.ops.name == "hip"
    _check_online(tmp_path, tmp_path / "Intrusion_result")
