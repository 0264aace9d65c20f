"""eval/device.py DeviceSimilarity with the reference ops (ops/ref.py TorchOps) on the CPU, against the CPU evaluator
(eval/similarity.py stat_sim / column_similarity) on the CSVs of the same tables; then the public interface: the
served generator's -score_against and the federation's -eval_every.

Tolerances (similarity_cases.py): W1 abs <= 1e-10 (<= 1e5 fp64 terms of magnitude <= 1 sum to an error of ~1e-11);
JSD abs <= 1e-9 where the reference value is >= 1e-3; near zero the square root amplifies rounding, so there both
values only have to be <= 1e-7.
"""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

import similarity_cases as sc
from fed_tgan_amd.eval.device import DeviceSimilarity
from fed_tgan_amd.ops.ref import TorchOps


def _score(name, **kw):
    real, vals, meta, vocabs, cats = sc.case(name)
    sim = DeviceSimilarity(real, meta, vocabs, torch.device("cpu"), **kw)
    return sim, sim.score(torch.from_numpy(vals.copy()))


@pytest.mark.parametrize("name", sc.CASES)
def test_reference_ops_match_stat_sim(name):
    sim, scores = _score(name, max_rows=700)
    assert isinstance(sim.ops, TorchOps)
    want_cols, want_avg = sc.expected(name)
    assert scores.avg_jsd.dim() == 0 and scores.avg_wd.dim() == 0
    sc.assert_scores(scores.columns(), scores.floats(), want_cols, want_avg, name)


def test_mixed_case_holds_the_corner_cases():
    """the planted cases are what they claim to be, judged by the CPU evaluator alone"""
    real, vals, meta, vocabs, cats = sc.case("mixed")
    cols, _ = sc.expected("mixed")
    v = dict(zip(cols["column"], cols["value"]))
    assert v[cats[0]] == 1.0                                   # no real category in the fake column
    assert 0.0 < v[cats[1]] < 1.0 and 0.0 < v[cats[2]] < 1.0
    names = [c["column_name"] for c in meta["columns"]]
    plain = [n for n in names if n not in cats and n not in meta["non_negative_cols"]]
    assert real[plain[0]].nunique() == 1                       # constant real column
    j = names.index(plain[1])
    assert vals[:, j].min() < real[plain[1]].min()             # fake values outside the real range
    conts = [n for n in names if n not in cats]
    assert any(real[n].nunique() < 40 and (real[n] == real[n].round()).all() for n in conts)   # heavy integer ties


def test_identical_tables_score_zero():
    _, scores = _score("identical", max_rows=300)
    cols = scores.columns()
    assert (cols["value"][cols["metric"] == "JSD"] <= sc.JSD_ZERO_TOL).all()
    assert (cols["value"][cols["metric"] == "WD"].abs() <= sc.W1_TOL).all()


def test_underflowing_code_is_dropped():
    real, vals, meta, vocabs, cats = sc.case("mixed")
    sim = DeviceSimilarity(real, meta, vocabs, torch.device("cpu"), max_rows=len(vals))
    sim.score(torch.from_numpy(vals.copy()))
    names = [c["column_name"] for c in meta["columns"]]
    nonneg = [n for n in names if n not in cats and n in meta["non_negative_cols"]]
    slot = sim.col_of[nonneg[0]][1]
    assert int(sim.valid[slot]) == len(vals) - 1
    assert torch.isinf(sim.keys[slot, len(vals) - 1])          # the sentinel sorts last


def test_more_rows_than_the_buffers_hold_raises():
    real, vals, meta, vocabs, cats = sc.case("plain")
    sim = DeviceSimilarity(real, meta, vocabs, torch.device("cpu"), max_rows=len(vals) - 1)
    with pytest.raises(ValueError, match="rows"):
        sim.score(torch.from_numpy(vals.copy()))


def test_date_columns_raise():
    real, vals, meta, vocabs, cats = sc.case("plain")
    meta = copy.deepcopy(meta)
    meta["date_info"] = {"when": "YYYY-MM-DD"}
    with pytest.raises(ValueError, match="date"):
        DeviceSimilarity(real, meta, vocabs, torch.device("cpu"))


def test_no_valid_fake_value_scores_nan():
    ops = TorchOps()
    real = torch.tensor([[0.0, 1.0, 2.0]], dtype=torch.float64)
    fake = torch.full((1, 4), float("inf"), dtype=torch.float64)
    out = torch.zeros(1, dtype=torch.float64)
    ops.sim_w1(real, torch.tensor([3], dtype=torch.int32), fake, torch.tensor([0], dtype=torch.int32), 4, out)
    assert np.isnan(float(out[0]))


# ----------------------------------------------------------------------------- public interface
import json          # noqa: E402
import os            # noqa: E402
import re            # noqa: E402
import subprocess    # noqa: E402
import sys           # noqa: E402

import pandas as pd  # noqa: E402

from fed_tgan_amd.data.schema import intrusion_spec                          # noqa: E402
from fed_tgan_amd.eval.similarity import similarity_table, stat_sim         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
CATS = intrusion_spec().categorical_list


def _close(got, want, what):
    """the file's tolerances on a pair (avg_jsd, avg_wd); the runs' JSD averages are far above the 1e-3 floor"""
    assert want[0] >= sc.JSD_FLOOR, (what, want)
    assert abs(got[0] - want[0]) <= sc.JSD_TOL and abs(got[1] - want[1]) <= sc.W1_TOL, (what, got, want)


@pytest.fixture(scope="module")
def gloo_run(tmp_path_factory):
    """two co-located client ranks over gloo, CPU backend, two epochs, every round scored"""
    out = tmp_path_factory.mktemp("fed_eval")
    r = subprocess.run([sys.executable, "-m", "dtds.distributed", "-world_size", "2", "-colocated", "-epochs", "2",
                        "-backend", "torch", "-synthetic_rows", "1000", "-n_sample", "501", "-batch_size", "100",
                        "-out_dir", str(out), "-quiet", "-dump_real", "-eval_every", "1", "-metrics_log",
                        str(out / "metrics.jsonl")], cwd=ROOT, env=ENV, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_federation_scores_every_round(gloo_run):
    res = gloo_run / "Intrusion_result"
    online = pd.read_csv(res / "similarity_online.csv", float_precision="round_trip")
    assert list(online.columns) == ["Epoch_No.", "Avg_JSD", "Avg_WD"] and online["Epoch_No."].tolist() == [0, 1]
    want = similarity_table(str(gloo_run / "data" / "raw" / "Intrusion_train.csv"),
                            [str(res / f"Intrusion_synthesis_epoch_{e}.csv") for e in range(2)], CATS)
    for e in range(2):
        _close((online["Avg_JSD"][e], online["Avg_WD"][e]), (want["Avg_JSD"][e], want["Avg_WD"][e]), f"epoch {e}")
    with open(gloo_run / "metrics.jsonl") as f:
        recs = [json.loads(line) for line in f if line.strip()]
    sims = [r for r in recs if "avg_jsd" in r]
    assert [r["epoch"] for r in sims] == [0, 1] and all(set(r) == {"epoch", "avg_jsd", "avg_wd"} for r in sims)
    assert [r["avg_jsd"] for r in sims] == online["Avg_JSD"].tolist()
    assert [r["avg_wd"] for r in sims] == online["Avg_WD"].tolist()


def test_sample_score_against(gloo_run, tmp_path):
    model = gloo_run / "models" / "Intrusion_generator.pt"
    real = gloo_run / "data" / "raw" / "Intrusion_train.csv"
    out = tmp_path / "s.csv"
    r = subprocess.run([sys.executable, "-m", "dtds.sample", "-model", str(model), "-n", "700", "-out", str(out),
                        "-backend", "torch", "-score_against", str(real)], cwd=ROOT, env=ENV, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert re.fullmatch(r"700 rows -> .*s\.csv \(\d+\.\d{3} s, torch on cpu\)", lines[-2]), lines
    m = re.fullmatch(r"Avg_JSD (\S+) Avg_WD (\S+) \(against .*\)", lines[-1])
    assert m, lines
    want = stat_sim(pd.read_csv(real), pd.read_csv(out), CATS)
    _close((float(m.group(1)), float(m.group(2))), want, "dtds.sample")
    # the same through the Python interface: a frame or a path, fresh rows each call
    from fed_tgan_amd.models.generator_io import load_generator
    gen = load_generator(str(model), torch.device("cpu"), backend="torch")
    a = gen.score(pd.read_csv(real), n=300)
    assert len(a) == 2 and all(isinstance(x, float) for x in a) and 0.0 < a[0] < 1.0 and a[1] > 0.0


def test_off_by_default_changes_nothing(tmp_path):
    from fed_tgan_amd.fed.local import run_local_emulation
    from fed_tgan_amd.fed.runtime import FedConfig
    from fed_tgan_amd.models.engine import EngineConfig

    def run(sub, **kw):
        cfg = FedConfig(spec=intrusion_spec(), epochs=2, synthetic_rows=1000, n_sample=400, out_dir=str(tmp_path / sub),
                        backend="torch", gmm_backend="torch", engine=EngineConfig(batch_size=100), verbose=False,
                        seed=5, **kw)
        torch.manual_seed(123)
        run_local_emulation(cfg, 1, backend="torch", device=torch.device("cpu"))
        return tmp_path / sub / "Intrusion_result"

    assert FedConfig(spec=intrusion_spec()).eval_every == 0 and FedConfig(spec=intrusion_spec()).eval_real is None
    off, on = run("off"), run("on", eval_every=1)
    assert sorted(os.listdir(off)) == ["Intrusion_synthesis_epoch_0.csv", "Intrusion_synthesis_epoch_1.csv"]
    assert "similarity_online.csv" in os.listdir(on)
    for e in range(2):          # scoring draws no random number and touches no table
        name = f"Intrusion_synthesis_epoch_{e}.csv"
        assert (off / name).read_bytes() == (on / name).read_bytes()


def test_eval_every_with_client_csvs_needs_eval_real(tmp_path):
    df = sc.small_table()[1]
    path = tmp_path / "client.csv"
    df.iloc[:300].to_csv(path, index=False)
    r = subprocess.run([sys.executable, "-m", "dtds.distributed", "-world_size", "2", "-colocated", "-backend", "torch",
                        "-datapath", str(path), "-eval_every", "1", "-out_dir", str(tmp_path)], cwd=ROOT, env=ENV,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "-eval_real" in r.stderr, (r.returncode, r.stderr[-1500:])
    assert not (tmp_path / "Intrusion_result").exists()          # no rank started
