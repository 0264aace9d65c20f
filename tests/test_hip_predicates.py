"""Range and set predicates on the HIP backend: pred_mark bit for bit against the reference op, pred_request's draw
(frequencies, and exactly against the numpy Philox oracle), and the engine end to end (wired and random-init
generator, every generation path, hipGraph replay against eager launches, the guard, the bounds-checked build)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fed_tgan_amd.models.conditional import build_request, driver_table
from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
from fed_tgan_amd.models.samplers import CondTables
from fed_tgan_amd.ops.ref import TorchOps
from helpers import small_table
import pred_cases as pc
import rng_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = TorchOps()
STREAM_ID = 25


@pytest.fixture(scope="module")
def hip():
    from fed_tgan_amd.ops import native
    from fed_tgan_amd.ops.hip import HipOps
    native.require()
    return HipOps(DEV, seed=1234)


# ----------------------------------------------------------------------------- pred_mark
@pytest.mark.parametrize("P", [1, 2, 16])
def test_mark_matches_reference_bitwise(hip, P):
    seed = 100 * P
    for m in (1, 63, 64, 65, 255, 256, 257, 1025):
        for n_cols in (1, 3, 42, 65):
            seed += 1
            req, out, tgt = pc.mark_case(m, n_cols, P, seed)
            dreq, dout, dtgt = pc.to_device(req, DEV), out.to(DEV), tgt.to(DEV)
            for _ in range(2):          # the second call continues the counters over the rows that are left
                REF.pred_mark(req, out, tgt)
                hip.pred_mark(dreq, dout, dtgt)
                tag = (m, n_cols, P)
                assert torch.equal(dtgt.cpu(), tgt), tag
                assert dreq["pred_stats"].tolist() == req["pred_stats"].tolist(), tag
            assert req["pred_stats"][0].item() >= (tgt >= 0).sum().item()


def test_mark_rejects_something_and_keeps_something(hip):
    """The cases above are not vacuous: rows pass, rows fail at more than one predicate, cleared rows stay uncounted."""
    req, out, tgt = pc.mark_case(1025, 42, 16, 7)
    live = int((tgt >= 0).sum())
    dreq, dtgt = pc.to_device(req, DEV), tgt.to(DEV)
    hip.pred_mark(dreq, out.to(DEV), dtgt)
    st = dreq["pred_stats"].tolist()
    assert st[0] == live < 1025 and 0 < st[1] < live and sum(1 for x in st[2:] if x) >= 3 and sum(st[2:]) == st[1]
    assert int((dtgt >= 0).sum()) == live - st[1]


# ----------------------------------------------------------------------------- pred_request
COND = {"cond_offset": [0, 3, 7], "cond_width": [3, 4, 5]}


def _driver(options, weights, span=2, dj=1, quota=10 ** 6, filled=0):
    opt, cum = driver_table(options, weights)
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=DEV)      # noqa: E731
    return {"drv": t([span, dj], torch.int32), "drv_opt": t(opt, torch.int32), "drv_cum": t(cum, torch.float64),
            "quota": t([quota], torch.int64), "filled": t([filled], torch.int64)}


def _setup(m, seed=0):
    g = torch.Generator().manual_seed(seed)
    cond = {k: torch.tensor(v, dtype=torch.int32, device=DEV) for k, v in COND.items()}
    col = torch.randint(0, 3, (m,), generator=g)
    opt = (torch.rand(m, generator=g) * torch.tensor(COND["cond_width"])[col]).long()
    h = torch.zeros(m, 4 + 12)
    h[torch.arange(m), 4 + torch.tensor(COND["cond_offset"])[col] + opt] = 1.0
    h[:, :4] = 0.5
    return cond, col.to(torch.int32).to(DEV), opt.to(torch.int32).to(DEV), h.to(DEV)


def _oracle_k(hip, m, cum):
    step = int(hip.ctr.cpu()[0])
    x, y, _, _ = rc.philox4(hip.seed, STREAM_ID * 16, step, np.arange(m))
    u = rc.u01d(x, y)
    return np.minimum(np.searchsorted(np.asarray(cum, dtype=np.float64), u, side="right"), len(cum) - 1)


def test_request_kernel_draw(hip):
    m = 40960
    req = _driver([4, 0, 2, 1], [3, 1, 0, 4])           # option order: 0 (w 1), 1 (w 4), 4 (w 3); option 2 left out
    assert req["drv_opt"].tolist() == [0, 1, 4] and req["drv_cum"].tolist() == [1 / 8, 5 / 8, 1.0]
    cond, col, opt, h = _setup(m)
    tgt = torch.full((m,), -5, dtype=torch.int32, device=DEV)
    hip.pred_request(req, col, opt, tgt, cond, h=h, c_col0=4, stream_id=STREAM_ID)
    o = opt.long().cpu()
    assert bool((tgt == 0).all()) and bool((col == 2).all()) and not bool((o == 2).any())
    freq = torch.bincount(o, minlength=5).double() / m
    # 8 standard errors at this m (0.5 / sqrt(40,960) = 0.0025)
    want = torch.tensor([1 / 8, 4 / 8, 0.0, 0.0, 3 / 8], dtype=torch.float64)
    assert (freq - want).abs().max().item() < 0.02, freq
    # exactly the oracle's draws: philox4 / u01d with the op's seed, stream 25, the counter and the row index
    k = _oracle_k(hip, m, req["drv_cum"].tolist())
    assert np.array_equal(o.numpy(), np.asarray([0, 1, 4])[k])
    # fp32 activations: one hot element per row, at cond_off[span] + opt; the other columns untouched
    hc = h.cpu()
    assert torch.equal(hc[:, 4:].sum(1), torch.ones(m)) and bool((hc[:, :4] == 0.5).all())
    assert bool((hc[torch.arange(m), 4 + 7 + o] == 1.0).all())
    # the same counter gives the same draws, a bumped one others
    _, col2, opt2, _ = _setup(m)
    tgt2 = torch.empty_like(tgt)
    hip.pred_request(req, col2, opt2, tgt2, cond, h=None, stream_id=STREAM_ID)
    assert torch.equal(opt2, opt) and torch.equal(tgt2, tgt)
    hip.L.rng_bump(hip.ctr)
    _, col3, opt3, _ = _setup(m)
    hip.pred_request(req, col3, opt3, tgt2, cond, h=None, stream_id=STREAM_ID)
    assert (opt3 != opt).float().mean().item() > 0.3
    assert np.array_equal(opt3.cpu().numpy(), np.asarray([0, 1, 4])[_oracle_k(hip, m, req["drv_cum"].tolist())])
    # a full quota: no targets, conditions and activations as they were
    req["filled"].copy_(req["quota"])
    c0, o0, h0 = col.clone(), opt.clone(), h.clone()
    hip.pred_request(req, col, opt, tgt, cond, h=h, c_col0=4, stream_id=STREAM_ID)
    assert bool((tgt == -1).all()) and torch.equal(col, c0) and torch.equal(opt, o0) and torch.equal(h, h0)


def test_request_kernel_wide_driver_table(hip):
    """M is bounded by the span width alone: 5,000 options of one wide span, searched by bisection."""
    M, m = 5000, 4096
    w = np.random.default_rng(0).random(M) + 0.01
    req = _driver(list(range(0, 2 * M, 2)), w.tolist(), span=0)
    cond = {"cond_offset": torch.tensor([0], dtype=torch.int32, device=DEV),
            "cond_width": torch.tensor([2 * M], dtype=torch.int32, device=DEV)}
    col = torch.zeros(m, dtype=torch.int32, device=DEV)
    opt = torch.zeros(m, dtype=torch.int32, device=DEV)
    tgt = torch.full((m,), -5, dtype=torch.int32, device=DEV)
    hip.pred_request(req, col, opt, tgt, cond, h=None, stream_id=STREAM_ID)
    o = opt.cpu().numpy()
    assert bool((tgt == 0).all()) and (o % 2 == 0).all() and o.min() >= 0 and o.max() < 2 * M
    assert np.array_equal(o, 2 * _oracle_k(hip, m, req["drv_cum"].tolist()))
    assert len(np.unique(o)) > 1000


@pytest.mark.parametrize("m", [1, 255, 257])
def test_request_kernel_edges(hip, m):
    """Row counts around the workgroup size: every row gets its target, nothing past the rows is written."""
    req = _driver([4, 0, 2, 1], [3, 1, 0, 4])
    cond, col, opt, h = _setup(m + 3)
    tgt = torch.full((m + 3,), -5, dtype=torch.int32, device=DEV)
    c0, o0, h0 = col.clone(), opt.clone(), h.clone()
    hip.pred_request(req, col, opt, tgt[:m], cond, h=h[:m], c_col0=4, stream_id=STREAM_ID)
    assert bool((tgt[:m] == 0).all()) and bool((tgt[m:] == -5).all())
    assert torch.equal(col[m:], c0[m:]) and torch.equal(opt[m:], o0[m:]) and torch.equal(h[m:], h0[m:])
    assert torch.equal(h[:m, 4:].sum(1), torch.ones(m, device=DEV)) and bool((col[:m] == 2).all())


# ----------------------------------------------------------------------------- engine end to end
def _engine(seed=3, wired=False, **cfg):
    _, _, _, _, _, _, tr, X = small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200, **cfg), DEV, backend="hip", seed=seed)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    if wired:
        pc.wire_generator_modes(eng, tr)
    return eng, tr


CFGS = [{}, {"precision": "fp32"}, {"gen_bf16": False}]
CFG_IDS = ["bf16", "fp32", "bf16-h32"]


@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_engine_wired_generator(cfg):
    tabs = []
    for use_graph in (True, False):
        eng, tr = _engine(wired=True, **cfg)
        assert eng.gen16 == (cfg == {})
        a = pc.scenario_wired_range(eng, tr, DEV, use_graph=use_graph)
        b = pc.scenario_wired_filter(eng, tr, DEV, use_graph=use_graph)
        tabs.append((a, b))
        eng.release()
    # equal seeds and states: a replayed pass and eagerly issued launches give the same tables bit for bit
    assert torch.equal(tabs[0][0], tabs[1][0]) and torch.equal(tabs[0][1], tabs[1][1])


@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_engine_random_init(cfg):
    tabs = []
    for use_graph in (True, False):
        eng, tr = _engine(seed=5, **cfg)
        tabs.append(pc.scenario_random_init(eng, tr, DEV, use_graph=use_graph))
        eng.release()
    assert torch.equal(tabs[0], tabs[1])


def test_engine_guard_with_a_range():
    tabs = []
    for use_graph in (True, False):
        eng, _ = _engine(seed=9)
        tabs.append(pc.scenario_guard_range(eng, DEV, use_graph=use_graph))
        eng.release()
    assert torch.equal(tabs[0], tabs[1])


def test_predicate_request_leaves_other_requests_alone():
    """generate_decoded and a plain one-value request return, after a predicate request, what they return when run
    first on a fresh engine of the same seed (the predicate request only advances the RNG counter, which is put
    back)."""
    _, _, _, meta, vocabs, _, _, _ = small_table()
    got = []
    for predicates_first in (False, True):
        eng, tr = _engine(seed=5)
        plain = build_request(tr, meta, vocabs, {"class": "smurf."}, 200, DEV)
        if predicates_first:
            ctr0 = eng.ops.ctr.clone()
            pc.scenario_random_init(eng, tr, DEV)
            eng.ops.ctr.copy_(ctr0)
        got.append((eng.generate_decoded(300), eng.generate_decoded_where(200, plain, chunk=1024),
                    dict(eng.last_conditional)))
        eng.release()
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert got[0][2] == got[1][2] and "predicates" not in got[0][2]


CHECKED_SCRIPT = r"""
import sys, torch
sys.path[:0] = [{root!r}, {tests!r}]
from fed_tgan_amd.ops import native
from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
from fed_tgan_amd.models.samplers import CondTables
from helpers import small_table
import pred_cases as pc
L = native.require()
assert native.CHECKED and L.is_checked(), "checked library not loaded"
_, _, _, meta, vocabs, _, tr, X = small_table()
dev = torch.device("cuda:0")
eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), dev, backend="hip", seed=3)
eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
pc.wire_generator_modes(eng, tr)
pc.scenario_wired_range(eng, tr, dev)
pc.scenario_wired_filter(eng, tr, dev)
print("CLEAN")
flagged = 0
for key, value in (("pred_j", 4000), ("drv", 4000)):
    req = pc.request(pc.SERROR, 120, dev)
    req[key][0] = value          # a column / a span outside the tables: flagged, never used as an index
    try:
        eng.generate_decoded_where(120, req, chunk=512, max_passes=1, use_graph=False)
    except RuntimeError as e:
        print("CHECK", key, ":", e)
        flagged += "conditional request index outside its tables" in str(e)
print("FLAGGED", flagged)
sys.exit(0 if flagged == 2 else 3)
"""


def test_checked_build_predicates():
    env = dict(os.environ, FEDTGAN_CHECKED="1")
    script = CHECKED_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert r.returncode == 0 and "CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "FLAGGED 2" in r.stdout, r.stdout[-2000:]
