"""The privacy guard on the CPU: the reference ops of the radius test (ops/ref.py nn_within, guard_mark, the one-bin
partition) against the plain-numpy oracle, PrivacyGuard, CTGANEngine.generate_decoded_guarded on the torch backend,
and the front ends (LoadedGenerator, ``dtds.sample -min_dcr``)."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

import guard_cases as gc
import privacy_cases as pc
from fed_tgan_amd.eval import DevicePrivacy, PrivacyGuard
from fed_tgan_amd.ops.ref import TorchOps

REF = TorchOps()


# ----------------------------------------------------------------------------- the reference ops
@pytest.mark.parametrize("layout", list(gc.WITHIN_LAYOUTS))
def test_reference_within_matches_oracle(layout):
    for nq in gc.WITHIN_NQ:
        for nr in (1, 17, 2049):
            gc.check_within_case(REF, "cpu", layout, nq, nr)


def test_input_conditions_hold_for_every_kernel_case():
    """the seeds of the GPU test's cases, checked here: both input conditions hold, and only the one listed case has
    its threshold off the middle pair"""
    for layout in gc.WITHIN_LAYOUTS:
        for nq in gc.WITHIN_NQ:
            for nr in gc.WITHIN_NR:
                _, d, ts = gc.within_case(layout, nq, nr)
                for lo, hi, t2 in ts:
                    assert gc.conditions(d, lo, hi, t2) == (True, True), (layout, nq, nr)
                u = np.unique(d.min(axis=1))
                if len(u) >= 2 and (layout, nq, nr) not in gc.WITHIN_OFF_MIDDLE:
                    k = len(u) // 2
                    assert ts == [(float(u[k - 1]), float(u[k]), 0.5 * float(u[k - 1] + u[k]))]


def test_exact_cases():
    gc.check_exact_within(REF, "cpu")


def test_infinite_radius_and_huge_value():
    gc.check_infinite_radius_and_huge_value(REF, "cpu")


@pytest.mark.parametrize("with_request", [False, True], ids=["plain", "request"])
@pytest.mark.parametrize("mode", ["ample", "inside"])
def test_mark_and_partition(mode, with_request):
    for seed, m in enumerate(gc.MARK_ROWS):
        gc.check_mark_partition(REF, "cpu", m, mode, with_request, seed)


# ----------------------------------------------------------------------------- PrivacyGuard
def test_guard_object():
    _, df, _, meta, vocabs, enc, _, _ = pc.small_table()
    enc = np.ascontiguousarray(np.asarray(enc), dtype=np.float64)
    ev = DevicePrivacy(df.iloc[:300], meta, vocabs, "cpu", max_rows=50, baseline=False)
    g = PrivacyGuard(df.iloc[:300], meta, vocabs, "cpu", min_dcr=0.0)
    shared = ev.guard(0.0)
    assert shared.r_cont is ev.r_cont and shared.r_cat is ev.r_cat and shared.lo is ev.lo and shared.scale is ev.scale
    assert torch.equal(g.r_cont, ev.r_cont) and torch.equal(g.r_cat, ev.r_cat) and g.t2.tolist() == [0.0]
    assert ev.guard(0.5).t2.tolist() == [0.25] and g.t2.dtype == torch.float64
    # rows 290..309: the first ten are real records at their own index, the rest are not in the guarded table
    vals = torch.from_numpy(enc[290:310] + 0.0)
    flagged, near = g.near(vals)
    s = ev.score(vals)
    assert flagged.tolist() == (s.rows()[0] == 0).tolist() and flagged[:10].all()
    assert near[:10].tolist() == s.rows()[2][:10].tolist() and (near[~flagged] == -1).all()
    with pytest.raises(ValueError, match="expected a float64"):
        g.near(vals.float())
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_dcr"):
            PrivacyGuard(df.iloc[:50], meta, vocabs, "cpu", min_dcr=bad)
        with pytest.raises(ValueError, match="min_dcr"):
            ev.guard(bad)
    with pytest.raises(ValueError, match="date"):
        PrivacyGuard(df.iloc[:50], dict(meta, date_info={"when": "%Y"}), vocabs, "cpu")
    coded = enc[:50].copy()
    cont = next(j for j, c in enumerate(meta["columns"]) if c["type"] != "categorical")
    coded[3, cont] = np.nan
    with pytest.raises(ValueError, match=meta["columns"][cont]["column_name"]):
        PrivacyGuard(coded, meta, vocabs, "cpu")


# ----------------------------------------------------------------------------- engine (torch backend)
def test_engine_deterministic_rejection():
    gc.deterministic_rejection("cpu", "torch", use_graph=False)


def test_engine_deterministic_rejection_with_request():
    gc.deterministic_rejection("cpu", "torch", use_graph=False, where={"class": {"back.": 2, "satan.": 1}})


def test_engine_radius():
    gc.radius_scenario("cpu", "torch")


def test_engine_exhaustion():
    gc.exhaustion_scenario("cpu", "torch")


def test_engine_refuses_a_foreign_guard_and_serves_zero_rows():
    _, _, _, meta, vocabs, _, _, _ = pc.small_table()
    eng, _ = gc.make_engine("cpu", "torch")
    guard = PrivacyGuard(gc.unmatched_real_row(), meta, vocabs, "cpu")
    assert eng.generate_decoded_guarded(0, guard).shape == (0, len(meta["columns"]))
    assert eng.last_guard == {"passes": 0, "generated": 0, "rejected": 0, "kept": 0}
    other = pc.coded_evaluator(np.zeros((2, 3)), [pc.CONT, pc.CAT, pc.CONT], max_rows=1, baseline=False).guard(0.0)
    with pytest.raises(ValueError, match="3-column"):
        eng.generate_decoded_guarded(10, other)


# ----------------------------------------------------------------------------- front ends
def test_loaded_generator_and_sample_cli(tmp_path, capsys):
    import dtds.sample
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    from fed_tgan_amd.models.generator_io import export_generator, load_generator
    from fed_tgan_amd.models.samplers import CondTables
    _, df, _, meta, vocabs, _, tr, X = pc.small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), "cpu", backend="torch", seed=5)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    path, real_csv = str(tmp_path / "g.pt"), str(tmp_path / "real.csv")
    out, out2 = str(tmp_path / "s.csv"), str(tmp_path / "s2.csv")
    export_generator(path, eng, tr, CondTables.from_encoded(X, tr.layout), meta, vocabs, "Intrusion")
    df.iloc[:400].to_csv(real_csv, index=False)
    torch.manual_seed(11)
    dtds.sample.main(["-model", path, "-n", "150", "-backend", "torch", "-seed", "0", "-out", out, "-min_dcr", "0",
                      "-privacy_against", real_csv])
    lines = capsys.readouterr().out.strip().splitlines()
    assert '"copies": 0.0' in lines[-1] and json.loads(lines[-1])["copies"] == 0.0
    assert lines[-2].startswith("150 rows -> ") and "guard min_dcr 0.0: " in lines[-2]
    assert " generated rows rejected" in lines[-2] and " passes, 0 of " in lines[-2]
    assert len(pd.read_csv(out)) == 150
    # the library call gives the table the command line wrote
    gen = load_generator(path, torch.device("cpu"), backend="torch", seed=0)
    torch.manual_seed(11)
    vals = gen.sample(150, min_dcr=0.0, guard_real=pd.read_csv(real_csv))
    assert vals.shape == (150, len(meta["columns"])) and gen.engine.last_guard["kept"] == 150
    gen._write_values(out2, vals)
    assert open(out2).read() == open(out).read()
    # -guard_against names another table; -where combines
    dtds.sample.main(["-model", path, "-n", "60", "-backend", "torch", "-out", out, "-min_dcr", "0.05",
                      "-guard_against", real_csv, "-where", "protocol_type=udp"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith("60 rows -> ") and "generated rows accepted" in line and "guard min_dcr 0.05: " in line
    assert (pd.read_csv(out)["protocol_type"] == "udp").all()
    # a radius needs a table
    with pytest.raises(SystemExit) as e:
        dtds.sample.main(["-model", path, "-n", "10", "-backend", "torch", "-out", out, "-min_dcr", "0"])
    assert e.value.code == 2 and "-min_dcr needs a real table" in capsys.readouterr().err
    with pytest.raises(ValueError, match="guard_real"):
        gen.sample(10, min_dcr=0.0)
    with pytest.raises(ValueError, match="min_dcr"):
        gen.sample(10, min_dcr=-1.0, guard_real=real_csv)
