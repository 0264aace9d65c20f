"""Conditional generation on the CPU path (torch backend): request resolution, the reference request / partition ops
on hand-made tables, the engine end to end with a wired and with the random-init generator, and the saved-generator
interface (LoadedGenerator, the CSV writer, ``python -m dtds.sample``)."""
import numpy as np
import pandas as pd
import pytest
import torch

from fed_tgan_amd.models.conditional import (MAX_BINS, ConditionalSamplingError, apportion, build_request,
                                             request_from_codes)
from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
from fed_tgan_amd.models.samplers import CondTables
from fed_tgan_amd.ops.ref import TorchOps
from cond_helpers import check_table as _check_table, code as _code, make_request as _req, names as _names, \
    wire_generator
from helpers import small_table

POISON = -777.0


# ----------------------------------------------------------------------------- request resolution
def test_request_resolution():
    _, _, _, meta, vocabs, _, tr, _ = small_table()
    names = _names(meta)
    req = build_request(tr, meta, vocabs, {"class": {"back.": 2, "satan.": 1}, "protocol_type": "tcp"}, 300, "cpu")
    jc, jp = names.index("class"), names.index("protocol_type")
    assert req["quota"].tolist() == [200, 100] and req["seg_off"].tolist() == [0, 200]
    assert req["filled"].tolist() == [0, 0] and req["stats"].tolist() == [0, 0]
    span, dj = req["drive"].tolist()
    assert dj == jc
    # the driving span is class's cond span: its offset in the conditional vector counts every earlier option
    lay = tr.layout
    assert lay.cond_width[span] == len(tr.meta[jc]["i2s"])
    assert lay.cond_start[span] + lay.cond_width[span] == lay.data_dim     # class is the last column's span
    for b, label in enumerate(["back.", "satan."]):
        code = _code(vocabs, "class", label)
        assert req["bin_code"][b].item() == float(code)
        assert tr.meta[jc]["i2s"][req["bin_opt"][b].item()] == code
    assert req["fixed_j"].tolist() == [jp]
    assert req["fixed_code"].tolist() == [float(_code(vocabs, "protocol_type", "tcp"))]
    assert req["values"] == ["back.", "satan."] and req["quotas"] == [200, 100]
    # protocol_type: i2s = [1, 2, 0] over the vocabulary icmp, tcp, udp -> udp is option 1
    assert list(tr.meta[jp]["i2s"]) == [1, 2, 0]
    r2 = build_request(tr, meta, vocabs, {"protocol_type": "udp"}, 10, "cpu")
    assert r2["drive"].tolist() == [jp, jp] and r2["bin_opt"].tolist() == [1] and r2["bin_code"].tolist() == [2.0]
    assert r2["quota"].tolist() == [10] and r2["fixed_j"].numel() == 0
    # the weighted column drives even when it is not first
    r3 = build_request(tr, meta, vocabs, {"protocol_type": "tcp", "class": {"back.": 1}}, 5, "cpu")
    assert r3["drive"].tolist()[1] == jc and r3["fixed_j"].tolist() == [jp]


def test_apportionment():
    assert apportion(100, [1, 1, 1]) == [34, 33, 33]
    assert apportion(300, [2, 1]) == [200, 100]
    assert apportion(7, [1, 0, 1]) == [4, 0, 3]
    assert apportion(0, [1, 2]) == [0, 0]
    assert apportion(10, [0.5]) == [10]
    _, _, _, meta, vocabs, _, tr, _ = small_table()
    req = build_request(tr, meta, vocabs, {"class": {"back.": 1, "satan.": 1, "smurf.": 1}}, 100, "cpu")
    assert req["quota"].tolist() == [34, 33, 33] and req["seg_off"].tolist() == [0, 34, 67]


@pytest.mark.parametrize("where, match", [
    ({"no_such_column": "x"}, "unknown column"),
    ({"duration": "1"}, "continuous"),
    ({"protocol_type": "ipx"}, "not in the vocabulary"),
    ({"class": {"back.": -1, "satan.": 2}}, "non-negative"),
    ({"class": {"back.": 0, "satan.": 0}}, "sum to zero"),
    ({"class": {"back.": 1}, "protocol_type": {"tcp": 1}}, "at most one column"),
    ({"class": {f"v{i}": 1 for i in range(MAX_BINS + 1)}}, f"bin limit is {MAX_BINS}"),
    ({}, "non-empty"),
])
def test_request_value_errors(where, match):
    _, _, _, meta, vocabs, _, tr, _ = small_table()
    with pytest.raises(ValueError, match=match):
        build_request(tr, meta, vocabs, where, 10, "cpu")


def test_request_value_outside_model_options():
    """A value the vocabulary knows but the model has no option for (absent from transformer.meta[j]["i2s"])."""
    import copy
    _, _, _, meta, vocabs, _, tr, _ = small_table()
    tr2 = copy.copy(tr)
    tr2.meta = copy.deepcopy(tr.meta)
    jp = _names(meta).index("protocol_type")
    tr2.meta[jp]["i2s"] = [1, 0]          # codes: icmp 0, tcp 1, udp 2 -- this model never saw udp
    with pytest.raises(ValueError, match="not among the model's options"):
        build_request(tr2, meta, vocabs, {"protocol_type": "udp"}, 10, "cpu")


# ----------------------------------------------------------------------------- the reference ops
def _table(drive_vals, fixed_vals=()):
    """[m, 1 + len(fixed) + 1] float64: column 0 the driving code, then the fixed columns, last a row id."""
    m = len(drive_vals)
    cols = [torch.tensor(drive_vals, dtype=torch.float64)]
    cols += [torch.tensor(v, dtype=torch.float64) for v in fixed_vals]
    cols.append(torch.arange(m, dtype=torch.float64) + 1000.0)
    return torch.stack(cols, 1).contiguous()


def _partition(req, out, tgt):
    n = int(req["quota"].sum())
    dst = torch.full((n, out.shape[1]), POISON, dtype=torch.float64)
    TorchOps().cond_partition(req, out, torch.tensor(tgt, dtype=torch.int32), dst)
    return dst


def test_ref_partition_keep_none_all_alternating():
    out = _table([5.0] * 6)
    req = _req([10], [0], 0, [7.0])
    dst = _partition(req, out, [0] * 6)                                  # none carries code 7
    assert req["filled"].tolist() == [0] and req["stats"].tolist() == [6, 0] and bool((dst == POISON).all())
    req = _req([10], [0], 0, [5.0])
    dst = _partition(req, out, [0] * 6)                                  # all do
    assert req["filled"].tolist() == [6] and req["stats"].tolist() == [6, 6]
    assert torch.equal(dst[:6], out) and bool((dst[6:] == POISON).all())
    out = _table([5.0, 1.0, 5.0, 1.0, 5.0, 1.0])
    req = _req([10], [0], 0, [5.0])
    dst = _partition(req, out, [0] * 6)                                  # alternating, order kept
    assert req["filled"].tolist() == [3] and dst[:3, -1].tolist() == [1000.0, 1002.0, 1004.0]
    assert bool((dst[3:] == POISON).all())


def test_ref_partition_quota_prefill_zero_and_untargeted():
    # bins: code 5 (quota 2, reached in mid-table), code 6 (quota 3, one delivered before), code 7 (zero quota)
    drive = [5.0, 6.0, 5.0, 5.0, 7.0, 6.0, 5.0, 6.0, 6.0]
    tgt = [0, 1, 0, 0, 2, 1, -1, 1, 0]        # row 6 has no target; row 8 carries 6 but was asked for bin 0
    out = _table(drive)
    req = _req([2, 3, 0], [0, 1, 0], 0, [5.0, 6.0, 7.0])
    dst = _partition(req, out, tgt)
    assert req["filled"].tolist() == [2, 3, 0]
    assert req["stats"].tolist() == [9, 7]                # rows 0 1 2 3 4 5 7 pass the predicate
    assert dst[0:2, -1].tolist() == [1000.0, 1002.0]      # bin 0: rows 0, 2 (row 3 is over quota)
    assert bool((dst[2] == POISON).all())                 # bin 1's first slot was filled before this pass
    assert dst[3:5, -1].tolist() == [1001.0, 1005.0]      # bin 1 continues at seg_off + filled (row 7 over quota)
    assert dst.shape[0] == 5


@pytest.mark.parametrize("k", [0, 1, 2])
def test_ref_partition_fixed_columns(k):
    drive = [5.0, 5.0, 5.0, 5.0]
    f1 = [1.0, 2.0, 1.0, 1.0]
    f2 = [9.0, 9.0, 8.0, 9.0]
    out = _table(drive, [f1, f2][:k])
    req = _req([4], [0], 0, [5.0], fixed=[(1, 1.0), (2, 9.0)][:k])
    dst = _partition(req, out, [0, 0, 0, 0])
    want = {0: [0, 1, 2, 3], 1: [0, 2, 3], 2: [0, 3]}[k]
    assert req["filled"].tolist() == [len(want)]
    assert dst[:len(want), -1].tolist() == [1000.0 + r for r in want]
    assert bool((dst[len(want):] == POISON).all())


def test_ref_request_draws_only_open_bins():
    torch.manual_seed(0)
    ops = TorchOps()
    m = 4000
    cond = {"cond_offset": torch.tensor([0, 3, 7], dtype=torch.int32), "cond_width": torch.tensor([3, 4, 5], dtype=torch.int32)}
    req = _req([30000, 10000, 500, 40000], [0, 0, 500, 0], 0, [0.0, 1.0, 2.0, 3.0], span=2, bin_opt=[4, 0, 2, 1])
    col = torch.zeros(m, dtype=torch.int32)
    opt = torch.ones(m, dtype=torch.int32)
    tgt = torch.full((m,), -5, dtype=torch.int32)
    h = torch.zeros(m, 2 + 12)
    h[:, 2 + 0 + 1] = 1.0                     # the sampler's one-hot: span 0, option 1
    ops.cond_request(req, col, opt, tgt, cond, h=h, c_col0=2)
    assert not bool((tgt == 2).any()) and int(tgt.min()) >= 0          # the full bin is never drawn
    freq = torch.bincount(tgt.long(), minlength=4).double() / m
    assert torch.allclose(freq, torch.tensor([3 / 8, 1 / 8, 0.0, 4 / 8], dtype=torch.float64), atol=0.04)
    assert bool((col == 2).all())
    assert torch.equal(opt.long(), torch.tensor([4, 0, 2, 1])[tgt.long()])
    assert torch.equal(h[:, 2:].sum(1), torch.ones(m))
    assert bool((h[torch.arange(m), 2 + 7 + opt.long()] == 1.0).all())
    # every quota full: no targets, conditions untouched
    req["filled"].copy_(req["quota"])
    col0, opt0, h0 = col.clone(), opt.clone(), h.clone()
    ops.cond_request(req, col, opt, tgt, cond, h=h, c_col0=2)
    assert bool((tgt == -1).all()) and torch.equal(col, col0) and torch.equal(opt, opt0) and torch.equal(h, h0)


# ----------------------------------------------------------------------------- engine end to end
def _engine(seed=3, wired=False, **cfg):
    _, _, _, _, _, _, tr, X = small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200, **cfg), "cpu", backend="torch", seed=seed)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    if wired:
        wire_generator(eng, tr)
    return eng, tr


def test_engine_wired_generator_exact_counts():
    _, _, _, meta, vocabs, _, _, _ = small_table()
    eng, tr = _engine(wired=True)
    where = {"class": {"back.": 2, "satan.": 1, "pod.": 1}}
    req = build_request(tr, meta, vocabs, where, 300, "cpu")
    torch.manual_seed(1)
    tab = eng.generate_decoded_where(300, req, chunk=128)
    lc = eng.last_conditional
    _check_table(tab, req, meta, vocabs, where)
    assert lc["filled"] == [150, 75, 75] and lc["values"] == ["back.", "satan.", "pod."]
    # the generator obeys its condition: while quotas are open every generated row is kept, so 300 rows take
    # exactly ceil(300 / 128) passes, and every generated row passes the predicate (rows kept == rows generated; the
    # last pass's surplus over the quotas is dropped after the compare)
    assert lc["passes"] == 3 and lc["generated"] == 3 * 128 and lc["kept"] == lc["generated"]
    # a fixed column the wired generator answers at random is enforced by rejection alone
    where2 = {"class": "neptune.", "flag": "SF"}
    req2 = build_request(tr, meta, vocabs, where2, 50, "cpu")
    tab2 = eng.generate_decoded_where(50, req2, chunk=256)
    _check_table(tab2, req2, meta, vocabs, where2)
    assert eng.generate_decoded_where(0, build_request(tr, meta, vocabs, where, 0, "cpu")).shape == (0, len(_names(meta)))


def test_engine_random_init_single_value_reproducible():
    _, _, _, meta, vocabs, _, _, _ = small_table()
    where = {"protocol_type": "udp"}
    tabs = []
    for _ in range(2):
        eng, tr = _engine(seed=5)
        req = build_request(tr, meta, vocabs, where, 300, "cpu")
        torch.manual_seed(11)
        tabs.append(eng.generate_decoded_where(300, req, chunk=1024))
        _check_table(tabs[-1], req, meta, vocabs, where)
        assert eng.last_conditional["filled"] == [300]
    assert torch.equal(tabs[0], tabs[1])


def test_engine_random_init_three_classes():
    _, _, _, meta, vocabs, _, _, _ = small_table()
    eng, tr = _engine(seed=5)
    where = {"class": {"normal.": 1, "smurf.": 1, "teardrop.": 1}}
    req = build_request(tr, meta, vocabs, where, 300, "cpu")
    torch.manual_seed(12)
    tab = eng.generate_decoded_where(300, req, chunk=4096)
    _check_table(tab, req, meta, vocabs, where)
    lc = eng.last_conditional
    assert lc["filled"] == [100, 100, 100] and lc["generated"] == lc["passes"] * 4096 and lc["kept"] >= 300


def test_engine_max_passes_raises_with_counts():
    _, _, _, meta, vocabs, _, _, _ = small_table()
    eng, tr = _engine(seed=5)
    req = build_request(tr, meta, vocabs, {"class": {"normal.": 1, "smurf.": 1}}, 600, "cpu")
    torch.manual_seed(13)
    with pytest.raises(ConditionalSamplingError) as ei:
        eng.generate_decoded_where(600, req, max_passes=1, chunk=256)
    assert len(ei.value.filled) == 2 and sum(ei.value.filled) <= 256 and ei.value.quotas == [300, 300]
    assert ei.value.values == ["normal.", "smurf."]
    with pytest.raises(ValueError, match="built for"):
        eng.generate_decoded_where(10, req)


def test_synthesizer_sample_where():
    from fed_tgan_amd.models.synthesizer import CTGANSynthesizer
    rng = np.random.default_rng(0)
    data = np.stack([rng.normal(size=400), rng.integers(0, 3, 400).astype(float)], 1)
    syn = CTGANSynthesizer(embedding_dim=16, gen_dim=(32,), dis_dim=(32,), batch_size=100, epochs=1, device="cpu",
                           backend="torch", seed=0, verbose=False).fit(data, categorical_columns=(1,))
    out = syn.sample(60, where={1: {2.0: 2, 0.0: 1}})
    assert out.shape == (60, 2) and (out[:40, 1] == 2.0).all() and (out[40:, 1] == 0.0).all()
    with pytest.raises(ValueError, match="continuous"):
        syn.sample(5, where={0: 1.0})
    with pytest.raises(ValueError, match="not among the model's options"):
        request_from_codes(syn.transformer, [(1, 7.0)], 5, "cpu")


# ----------------------------------------------------------------------------- the saved generator
def test_saved_generator_where(tmp_path, capsys):
    from fed_tgan_amd.models.generator_io import export_generator, load_generator
    import dtds.sample
    _, _, _, meta, vocabs, _, tr, X = small_table()
    eng, _ = _engine(seed=5)
    path = str(tmp_path / "g.pt")
    export_generator(path, eng, tr, CondTables.from_encoded(X, tr.layout), meta, vocabs, "Intrusion")
    gen = load_generator(path, torch.device("cpu"), backend="torch", seed=0)
    jp = _names(meta).index("protocol_type")
    vals = gen.sample(200, where={"protocol_type": "udp"})
    assert vals.shape == (200, len(meta["columns"])) and (vals[:, jp] == _code(vocabs, "protocol_type", "udp")).all()
    assert gen.sample(20).shape == (20, len(meta["columns"]))             # the unconditional form is unchanged
    p1 = str(tmp_path / "a.csv")
    gen.write_csv(p1, 200, where={"protocol_type": "udp", "flag": "SF"})
    df = pd.read_csv(p1)
    assert len(df) == 200 and (df["protocol_type"] == "udp").all() and (df["flag"] == "SF").all()
    p2 = str(tmp_path / "b.csv")
    dtds.sample.main(["-model", path, "-n", "200", "-where", "protocol_type=udp", "-backend", "torch", "-out", p2])
    df = pd.read_csv(p2)
    assert len(df) == 200 and (df["protocol_type"] == "udp").all()
    line = capsys.readouterr().out
    assert "passes" in line and "accepted" in line
    p3 = str(tmp_path / "c.csv")
    dtds.sample.main(["-model", path, "-n", "90", "-backend", "torch", "-out", p3, "-max_passes", "64", "-where_json",
                      '{"class": {"normal.": 2, "smurf.": 1}, "protocol_type": "tcp"}'])
    df = pd.read_csv(p3)
    assert df["class"].tolist() == ["normal."] * 60 + ["smurf."] * 30 and (df["protocol_type"] == "tcp").all()
