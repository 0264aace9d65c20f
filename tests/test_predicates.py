"""Range and set predicates of conditional generation on the CPU path (torch backend): the request language, the
reference ops on hand-made tables, the engine end to end with a generator wired on its mode indicators and with the
random-init one, and the public interfaces (CTGANSynthesizer, ``python -m dtds.sample``)."""
import math

import numpy as np
import pandas as pd
import pytest
import torch
from scipy.stats import norm

from fed_tgan_amd.models.conditional import (PRED_MAX, ConditionalSamplingError, build_request, mode_tables,
                                             parse_where, range_weights, request_from_codes)
from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
from fed_tgan_amd.models.samplers import CondTables
from fed_tgan_amd.ops.ref import TorchOps
from cond_helpers import code as _code, names as _names
from helpers import small_table
import pred_cases as pc

RANGE, SET = pc.RANGE, pc.SET


# ----------------------------------------------------------------------------- resolution
def test_range_drives_through_the_mode_span():
    _, _, _, meta, _, _, tr, _ = small_table()
    js = _names(meta).index("serror_rate")
    req = pc.request(pc.SERROR, 300)
    assert req["drv"].tolist() == [js, js] and req["quota"].tolist() == [300] and req["fixed_j"].numel() == 0
    assert req["pred_j"].tolist() == [js] and req["pred_kind"].tolist() == [RANGE]
    assert req["pred_lo"].tolist() == [0.9] and req["pred_hi"].tolist() == [1.0]      # not a non-negative column
    mu, sd = mode_tables(tr, js)
    reach = [k for k in range(len(mu)) if mu[k] - 4 * sd[k] <= 1.0 and mu[k] + 4 * sd[k] >= 0.9]
    assert req["drv_opt"].tolist() == reach
    narrow = int(np.argmin(np.abs(mu)))                        # the mode with mean 0 and sd 0.015 is absent
    assert abs(mu[narrow]) < 0.01 and sd[narrow] < 0.02 and narrow not in reach and len(reach) == len(mu) - 1
    cum = req["drv_cum"].tolist()
    assert all(a < b for a, b in zip(cum, cum[1:])) and cum[-1] == 1.0
    cnt = pc.counts()[js]
    # Phi(b) - Phi(a), from the survival function where both arguments are positive
    w = []
    for k in reach:
        a, b = (0.9 - mu[k]) / sd[k], (1.0 - mu[k]) / sd[k]
        w.append(cnt[k] * ((norm.sf(a) - norm.sf(b)) if a > 0 else (norm.cdf(b) - norm.cdf(a))))
    modes, got_w = range_weights(tr, js, 0.9, 1.0, cnt)
    assert modes == reach
    np.testing.assert_allclose(got_w, w, rtol=1e-12)
    assert 180 < w[0] < 200 and 0.1 < w[1] < 0.2                 # about 189 for mode 0 and 0.13 for mode 2
    want = np.cumsum(w) / np.sum(w)
    np.testing.assert_allclose(cum[:-1], want[:-1], rtol=1e-12)
    np.testing.assert_allclose(np.diff([0.0] + cum) * np.sum(w), w, rtol=1e-12)
    assert req["values"] == ["serror_rate in [0.9, 1.0]"]
    assert req["predicates"] == [("serror_rate", "range", (0.9, 1.0))]


def test_non_negative_bounds_are_converted_once():
    req = pc.request({"src_bytes": {"min": 100, "max": 1000}}, 10)
    assert req["pred_lo"].tolist() == [math.log1p(100)] and req["pred_hi"].tolist() == [math.log1p(1000)]
    assert req["predicates"] == [("src_bytes", "range", (100.0, 1000.0))]          # messages keep the printed bounds
    r0 = pc.request({"src_bytes": {"min": 0, "max": 5}}, 10)
    assert r0["pred_lo"].tolist() == [-math.inf] and r0["pred_hi"].tolist() == [math.log1p(5)]
    r1 = pc.request({"src_bytes": {"min": 3}}, 10)
    assert r1["pred_lo"].tolist() == [math.log1p(3)] and r1["pred_hi"].tolist() == [math.inf]
    with pytest.raises(ValueError, match="non-negative"):
        pc.request({"src_bytes": {"max": -1}}, 10)


def test_set_drives_with_the_span_counts():
    _, _, _, meta, vocabs, _, tr, _ = small_table()
    jp = _names(meta).index("protocol_type")
    req = pc.request({"protocol_type": ["tcp", "udp"]}, 50)
    codes = [_code(vocabs, "protocol_type", v) for v in ("tcp", "udp")]
    lut = req["pred_lut"].tolist()
    assert req["pred_kind"].tolist() == [SET] and req["pred_lut_off"].tolist() == [0]
    assert req["pred_lut_len"].tolist() == [len(lut)] == [3]
    assert [c for c, b in enumerate(lut) if b] == sorted(codes)
    i2s = list(tr.meta[jp]["i2s"])
    opts = sorted(i2s.index(c) for c in codes)
    assert req["drv"].tolist() == [jp, jp] and req["drv_opt"].tolist() == opts
    cnt = pc.counts()[jp]
    np.testing.assert_allclose(np.diff([0.0] + req["drv_cum"].tolist()), cnt[opts] / cnt[opts].sum(), rtol=1e-12)
    assert req["drv_cum"][-1].item() == 1.0


def test_weighted_driver_keeps_its_buffers_and_gains_a_predicate():
    _, _, _, meta, vocabs, _, tr, _ = small_table()
    both = pc.request({"class": {"back.": 2, "satan.": 1}, "serror_rate": {"max": 0.5}}, 300)
    plain = build_request(tr, meta, vocabs, {"class": {"back.": 2, "satan.": 1}}, 300, "cpu")
    for k in ("drive", "bin_opt", "bin_code", "quota", "filled", "seg_off", "fixed_j", "fixed_code", "stats"):
        assert torch.equal(both[k], plain[k]) and both[k].dtype == plain[k].dtype, k
    assert both["values"] == plain["values"] and both["quotas"] == plain["quotas"] and "drv" not in both
    assert both["pred_j"].tolist() == [_names(meta).index("serror_rate")] and both["pred_kind"].tolist() == [RANGE]
    assert both["pred_lo"].tolist() == [-math.inf] and both["pred_hi"].tolist() == [0.5]
    assert plain["pred_j"].numel() == 0 and plain["pred_stats"].tolist() == [0] * (2 + PRED_MAX)
    # a scalar that drives keeps its path too; the set behind it is a filter
    r = pc.request({"class": "smurf.", "protocol_type": ["icmp", "tcp"]}, 10)
    assert "drv" not in r and r["pred_kind"].tolist() == [SET] and r["fixed_j"].numel() == 0
    # behind a driving range a scalar becomes a one-value set
    r = pc.request({"serror_rate": {"min": 0.9}, "protocol_type": "tcp"}, 10)
    assert r["pred_kind"].tolist() == [RANGE, SET] and r["fixed_j"].numel() == 0 and r["quota"].tolist() == [10]
    assert sum(r["pred_lut"].tolist()) == 1


def _many_predicates(k):
    _, _, _, meta, _, _, tr, _ = small_table()
    cont = [c["column_name"] for j, c in enumerate(meta["columns"]) if tr.meta[j]["type"] == "continuous"]
    assert len(cont) >= k
    return {"class": "smurf.", **{c: {"min": -1e9} for c in cont[:k]}}


@pytest.mark.parametrize("where, match", [
    ({"duration": "1"}, "continuous"),
    ({"duration": 1.0}, r"continuous.*min"),
    ({"duration": {"low": 1}}, "continuous"),
    ({"duration": {"min": 0, "most": 2}}, "continuous"),
    ({"duration": {}}, "continuous"),
    ({"serror_rate": {"min": 0.8, "max": 0.2}}, "exceeds max"),
    ({"serror_rate": {"min": float("nan")}}, "finite"),
    ({"serror_rate": {"max": float("inf")}}, "finite"),
    ({"protocol_type": []}, "empty list"),
    ({"protocol_type": ["tcp", "tcp"]}, "listed twice"),
    ({"protocol_type": ["tcp", "ipx"]}, "not in the vocabulary"),
    ({"serror_rate": {"min": 2, "max": 3}}, r"serror_rate.*no mode.*\[2\.0, 3\.0\].*reach"),
])
def test_request_errors(where, match):
    with pytest.raises(ValueError, match=match):
        pc.request(where, 10)


def test_predicate_limit():
    assert pc.request(_many_predicates(PRED_MAX), 10)["pred_j"].numel() == PRED_MAX
    with pytest.raises(ValueError, match=f"limit is {PRED_MAX}"):
        pc.request(_many_predicates(PRED_MAX + 1), 10)


def test_set_value_outside_model_options():
    import copy
    _, _, _, meta, vocabs, _, tr, _ = small_table()
    tr2 = copy.copy(tr)
    tr2.meta = copy.deepcopy(tr.meta)
    tr2.meta[_names(meta).index("protocol_type")]["i2s"] = [1, 0]          # this model never saw udp (code 2)
    with pytest.raises(ValueError, match="not among the model's options"):
        build_request(tr2, meta, vocabs, {"protocol_type": ["tcp", "udp"]}, 10, "cpu", counts=pc.counts())


def test_driver_table_zero_weights():
    """A point range holds no mass of any Gaussian: the reachable modes are drawn uniformly."""
    _, _, _, meta, _, _, tr, _ = small_table()
    mu, sd = mode_tables(tr, _names(meta).index("serror_rate"))
    req = pc.request({"serror_rate": {"min": 0.95, "max": 0.95}}, 10)
    m = req["drv_opt"].numel()
    assert m == 2 and req["drv_cum"].tolist() == [0.5, 1.0]
    with pytest.raises(ValueError, match="span counts"):
        _, _, _, meta, vocabs, _, tr, _ = small_table()
        build_request(tr, meta, vocabs, pc.SERROR, 10, "cpu")


def test_parse_where_ranges():
    assert parse_where(["a=b"], None) == {"a": "b"}                     # the two-argument form is unchanged
    w = parse_where(["p=tcp"], '{"c": ["x", "y"]}', ["s=0.9:1", "b=100:", "d=:5e3"])
    assert w == {"c": ["x", "y"], "p": "tcp", "s": {"min": 0.9, "max": 1.0}, "b": {"min": 100.0}, "d": {"max": 5000.0}}
    for bad in ("s", "s=1", "s=:", "s=1:2:3", "s=a:2", "=1:2"):
        with pytest.raises(ValueError, match="where_range"):
            parse_where([], None, [bad])


# ----------------------------------------------------------------------------- the reference ops
def test_ref_pred_mark_by_hand():
    nan, inf = math.nan, math.inf
    #        col0 (range)  col1 (set, codes 0..3)  col2 (open range)
    out = torch.tensor([[0.5, 1.0, 7.0],      # passes everything
                        [0.0, 3.0, -2.0],     # bounds are inclusive; code 3 allowed
                        [1.0, 0.0, 9.0],      # upper bound inclusive
                        [nan, 1.0, 7.0],      # NaN is outside every range -> predicate 0
                        [0.5, 1.5, 7.0],      # a non-integer code -> predicate 1
                        [0.5, 4.0, 7.0],      # a code past the table -> predicate 1
                        [0.5, -1.0, 7.0],     # a negative code -> predicate 1
                        [0.5, 2.0, 7.0],      # a code the set does not list -> predicate 1
                        [2.0, 2.0, 7.0],      # fails 0 and 1: counted for 0 alone
                        [0.5, 1.0, 11.0],     # -> predicate 2
                        [0.5, nan, 11.0],     # NaN code -> predicate 1 (before 2)
                        [9.0, 9.0, 99.0],     # fails all, but has no target: untouched, uncounted
                        [0.5, inf, 7.0]],     # an infinite code -> predicate 1
                       dtype=torch.float64)
    preds = [(0, RANGE, 0.0, 1.0), (1, SET, [1, 1, 0, 1]), (2, RANGE, -inf, 10.0)]
    req = pc.make_preds(preds)
    tgt = torch.zeros(13, dtype=torch.int32)
    tgt[11] = -1
    tgt[2] = 5                   # any non-negative target is a live row; the value survives a pass
    TorchOps().pred_mark(req, out, tgt)
    assert tgt.tolist() == [0, 0, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1]
    assert req["pred_stats"].tolist() == [12, 9, 2, 6, 1] + [0] * (PRED_MAX - 3)
    first = pc.reference_pass(out.numpy(), preds)
    assert [int(f) for f in first[:11]] == [-1, -1, -1, 0, 1, 1, 1, 1, 0, 2, 1]
    # a second call continues the counters and leaves cleared rows alone
    TorchOps().pred_mark(req, out, tgt)
    assert req["pred_stats"].tolist()[:5] == [15, 9, 2, 6, 1]
    # a predicate that points outside the table fails every live row
    bad = pc.make_preds([(3, RANGE, -inf, inf)])
    t2 = torch.zeros(13, dtype=torch.int32)
    TorchOps().pred_mark(bad, out, t2)
    assert bool((t2 == -1).all()) and bad["pred_stats"].tolist()[:3] == [13, 13, 13]


def test_ref_pred_mark_matches_the_plain_rule():
    ops = TorchOps()
    for seed, (m, n_cols, P) in enumerate([(1, 1, 1), (65, 3, 2), (257, 5, 16), (300, 42, 7)]):
        req, out, tgt = pc.mark_case(m, n_cols, P, seed)
        preds = []
        for k in range(P):
            if req["pred_kind"][k] == RANGE:
                preds.append((int(req["pred_j"][k]), RANGE, float(req["pred_lo"][k]), float(req["pred_hi"][k])))
            else:
                o, ln = int(req["pred_lut_off"][k]), int(req["pred_lut_len"][k])
                preds.append((int(req["pred_j"][k]), SET, req["pred_lut"][o:o + ln].tolist()))
        first = pc.reference_pass(out.numpy(), preds)
        live = tgt.numpy() >= 0
        ops.pred_mark(req, out, tgt)
        assert (tgt.numpy() == np.where(live & (first < 0), 0, -1)).all()
        st = req["pred_stats"].tolist()
        assert st[0] == live.sum() and st[1] == (live & (first >= 0)).sum()
        assert st[2:2 + P] == [int((live & (first == k)).sum()) for k in range(P)]


def test_ref_pred_request_draws_by_weight():
    torch.manual_seed(0)
    ops = TorchOps()
    m = 8000
    cond = {"cond_offset": torch.tensor([0, 3, 7], dtype=torch.int32), "cond_width": torch.tensor([3, 4, 5], dtype=torch.int32)}
    req = {"drv": torch.tensor([2, 1], dtype=torch.int32), "drv_opt": torch.tensor([4, 0, 1], dtype=torch.int32),
           "drv_cum": torch.tensor([3 / 8, 4 / 8, 1.0], dtype=torch.float64),
           "quota": torch.tensor([10 ** 6]), "filled": torch.tensor([0])}
    col = torch.zeros(m, dtype=torch.int32)
    opt = torch.ones(m, dtype=torch.int32)
    tgt = torch.full((m,), -5, dtype=torch.int32)
    h = torch.zeros(m, 2 + 12)
    h[:, 2 + 0 + 1] = 1.0
    ops.pred_request(req, col, opt, tgt, cond, h=h, c_col0=2)
    assert bool((tgt == 0).all()) and bool((col == 2).all())
    freq = torch.bincount(opt.long(), minlength=5).double() / m
    assert torch.allclose(freq, torch.tensor([1 / 8, 4 / 8, 0, 0, 3 / 8], dtype=torch.float64), atol=0.03)
    assert torch.equal(h[:, 2:].sum(1), torch.ones(m)) and bool((h[torch.arange(m), 2 + 7 + opt.long()] == 1.0).all())
    req["filled"].copy_(req["quota"])
    c0, o0, h0 = col.clone(), opt.clone(), h.clone()
    ops.pred_request(req, col, opt, tgt, cond, h=h, c_col0=2)
    assert bool((tgt == -1).all()) and torch.equal(col, c0) and torch.equal(opt, o0) and torch.equal(h, h0)


# ----------------------------------------------------------------------------- engine end to end
def _engine(seed=3, wired=False, **cfg):
    _, _, _, _, _, _, tr, X = small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200, **cfg), "cpu", backend="torch", seed=seed)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    if wired:
        pc.wire_generator_modes(eng, tr)
    return eng, tr


def test_engine_wired_range_drives():
    eng, tr = _engine(wired=True)
    torch.manual_seed(1)
    pc.scenario_wired_range(eng, tr, "cpu")


def test_engine_wired_range_filters_behind_weighted_class():
    eng, tr = _engine(wired=True)
    torch.manual_seed(2)
    pc.scenario_wired_filter(eng, tr, "cpu")


def test_engine_random_init_two_ranges():
    eng, tr = _engine(seed=5)
    torch.manual_seed(5)
    pc.scenario_random_init(eng, tr, "cpu")
    # requests without predicates are served as before, from their own entries
    _, _, _, meta, vocabs, _, _, _ = small_table()
    req = build_request(tr, meta, vocabs, {"class": "smurf."}, 40, "cpu")
    assert eng.generate_decoded_where(40, req, chunk=1024).shape[0] == 40
    assert "predicates" not in eng.last_conditional


def test_engine_set_drives_in_the_models_proportions():
    _, _, _, meta, vocabs, _, _, _ = small_table()
    eng, tr = _engine(wired=True)
    torch.manual_seed(3)
    req = pc.request({"protocol_type": ["tcp", "udp"], "serror_rate": {"max": 0.5}}, 400)
    tab = eng.generate_decoded_where(400, req, chunk=256)
    jp = _names(meta).index("protocol_type")
    got = set(tab[:, jp].tolist())
    assert got == {float(_code(vocabs, "protocol_type", v)) for v in ("tcp", "udp")} and pc.inside(tab, req)
    # the wired generator obeys the drawn option: the set predicate rejects nothing
    assert eng.last_conditional["predicates"][0]["rejected"] == 0


def test_starvation_names_a_predicate():
    eng, tr = _engine(seed=5)
    torch.manual_seed(7)
    req = pc.request(pc.TWO_RANGES, 5000)
    with pytest.raises(ConditionalSamplingError, match=r"predicate (serror_rate|src_bytes) in \[.*rejected \d+ of") as ei:
        eng.generate_decoded_where(5000, req, max_passes=1, chunk=128)
    assert ei.value.quotas == [5000] and sum(ei.value.filled) <= 128
    assert "src_bytes in [100.0, 1000.0]" in str(ei.value) or "serror_rate in [0.9, 1.0]" in str(ei.value)


def test_guard_combined_with_a_range():
    eng, _ = _engine(seed=9)
    torch.manual_seed(23)
    pc.scenario_guard_range(eng, torch.device("cpu"))


# ----------------------------------------------------------------------------- public interfaces
def test_synthesizer_sample_ranges_and_sets():
    from fed_tgan_amd.models.synthesizer import CTGANSynthesizer
    rng = np.random.default_rng(0)
    data = np.stack([rng.normal(size=400), rng.integers(0, 3, 400).astype(float)], 1)
    syn = CTGANSynthesizer(embedding_dim=16, gen_dim=(32,), dis_dim=(32,), batch_size=100, epochs=1, device="cpu",
                           backend="torch", seed=0, verbose=False).fit(data, categorical_columns=(1,))
    out = syn.sample(60, where={0: {"min": -0.5, "max": 0.75}})
    assert out.shape == (60, 2) and (out[:, 0] >= -0.5).all() and (out[:, 0] <= 0.75).all()
    out = syn.sample(60, where={1: [2.0, 0.0]})
    assert out.shape == (60, 2) and set(out[:, 1].tolist()) <= {2.0, 0.0}
    out = syn.sample(30, where={1: {2.0: 2, 0.0: 1}, 0: {"max": 0.0}})
    assert (out[:20, 1] == 2.0).all() and (out[20:, 1] == 0.0).all() and (out[:, 0] <= 0.0).all()
    with pytest.raises(ValueError, match="continuous"):
        syn.sample(5, where={0: 1.0})
    with pytest.raises(ValueError, match="not among the model's options"):
        request_from_codes(syn.transformer, [(1, [7.0])], 5, "cpu")


def test_cli_where_range_and_json(tmp_path, capsys):
    from fed_tgan_amd.models.generator_io import export_generator
    import dtds.sample
    _, _, _, meta, vocabs, _, tr, X = small_table()
    eng, _ = _engine(seed=5)
    path = str(tmp_path / "g.pt")
    export_generator(path, eng, tr, CondTables.from_encoded(X, tr.layout), meta, vocabs, "Intrusion")
    tol = lambda v: 1e-12 * abs(v) + 1e-12      # noqa: E731   (log1p and exp, each good to about an ulp)
    p1 = str(tmp_path / "a.csv")
    dtds.sample.main(["-model", path, "-n", "120", "-backend", "torch", "-out", p1, "-where_range",
                      "src_bytes=100:1000", "-where_range", "serror_rate=:0.5", "-where", "protocol_type=tcp"])
    df = pd.read_csv(p1)
    assert len(df) == 120 and (df["protocol_type"] == "tcp").all()
    assert (df["src_bytes"] >= 100 - tol(100)).all() and (df["src_bytes"] <= 1000 + tol(1000)).all()
    assert (df["serror_rate"] <= 0.5).all()
    line = capsys.readouterr().out
    assert "src_bytes in [100.0, 1000.0] rejected" in line and "serror_rate in [-inf, 0.5] rejected" in line
    p2 = str(tmp_path / "b.csv")
    dtds.sample.main(["-model", path, "-n", "90", "-backend", "torch", "-out", p2, "-where_json",
                      '{"protocol_type": ["tcp", "udp"], "dst_bytes": {"min": 10}, "flag": "SF"}'])
    df = pd.read_csv(p2)
    assert len(df) == 90 and set(df["protocol_type"]) <= {"tcp", "udp"} and (df["flag"] == "SF").all()
    assert (df["dst_bytes"] >= 10 - tol(10)).all()
    with pytest.raises(SystemExit):
        dtds.sample.main(["-model", path, "-n", "5", "-backend", "torch", "-where_range", "src_bytes=1"])
