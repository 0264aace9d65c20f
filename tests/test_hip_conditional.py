"""Conditional generation on the HIP backend: the partition kernels bit for bit against the reference op, the request
kernel's draw, and the engine end to end (wired and random-init generator, both generation paths, hipGraph replay
against eager launches, the bounds-checked build)."""
import os
import subprocess
import sys

import pytest
import torch

from fed_tgan_amd.models.conditional import build_request
from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
from fed_tgan_amd.models.samplers import CondTables
from fed_tgan_amd.ops.ref import TorchOps
from cond_helpers import check_table, make_request, request_to, wire_generator
from helpers import small_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = TorchOps()
POISON = -777.0


@pytest.fixture(scope="module")
def hip():
    from fed_tgan_amd.ops import native
    from fed_tgan_amd.ops.hip import HipOps
    native.require()
    return HipOps(DEV, seed=1234)


# ----------------------------------------------------------------------------- partition kernels
def _quotas(mode, m, B):
    """(quota, filled) per bin.  A workgroup holds 256 rows and about a quarter of the rows are kept, spread over the
    bins, so `inside` ends every quota within the first workgroup's rows once m exceeds a few rows per bin."""
    if mode == "ample":
        return [m + 1] * B, [0] * B
    if mode == "inside":
        return [max(1, min(m, 256) // (8 * B))] * B, [0] * B
    if mode == "zero":
        return [0 if b % 2 else m + 1 for b in range(B)], [0] * B
    q = [2 + m // (2 * B) + b for b in range(B)]        # prefilled: some bins nearly full, some already full
    return q, [min(q[b], (b % 3) * (q[b] // 2)) for b in range(B)]


def _case(m, n_cols, B, k, mode, seed):
    g = torch.Generator().manual_seed(seed)
    out = torch.rand(m, n_cols, generator=g, dtype=torch.float64) + 100.0       # no cell equals a code by chance
    tgt = torch.randint(-1, B, (m,), generator=g, dtype=torch.int64)
    dj = n_cols - 1
    # the driving column carries the target's code on ~70 % of the rows, another bin's or none otherwise
    carried = torch.where(torch.rand(m, generator=g) < 0.7, tgt.clamp_min(0), torch.randint(0, B, (m,), generator=g))
    out[:, dj] = carried.double() * 3.0 + 1.0
    if n_cols >= 3:
        fixed = [(0, 4.0), (n_cols // 2, 9.0)][:k]
        for j, c in fixed:
            out[:, j] = torch.where(torch.rand(m, generator=g) < 0.8, torch.tensor(c, dtype=torch.float64),
                                    torch.tensor(c + 1.0, dtype=torch.float64))
    else:           # too few columns for separate ones: the fixed columns repeat the driving one (bin 0's code)
        fixed = [(dj, 1.0)] * k
    quota, filled = _quotas(mode, m, B)
    req = make_request(quota, filled, dj, [b * 3.0 + 1.0 for b in range(B)], fixed=fixed)
    return req, out, tgt.to(torch.int32)


@pytest.mark.parametrize("mode", ["ample", "inside", "zero", "prefilled"])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_partition_matches_reference_bitwise(hip, mode, B):
    seed = 0
    for m in (1, 63, 64, 65, 255, 256, 257, 1025):
        for n_cols in (1, 3, 42, 65):
            for k in (0, 2):
                seed += 1
                req, out, tgt = _case(m, n_cols, B, k, mode, seed)
                n = max(1, int(req["quota"].sum()))
                dst = torch.full((n, n_cols), POISON, dtype=torch.float64)
                dreq, dout, dtgt, ddst = request_to(req, DEV), out.to(DEV), tgt.to(DEV), dst.to(DEV)
                REF.cond_partition(req, out, tgt, dst)
                hip.cond_partition(dreq, dout, dtgt, ddst)
                tag = (m, n_cols, B, k, mode)
                assert torch.equal(ddst.cpu(), dst), tag        # poison beyond filled included
                assert dreq["filled"].tolist() == req["filled"].tolist(), tag
                assert dreq["stats"].tolist() == req["stats"].tolist(), tag
                if mode == "inside" and m >= 256 and n_cols >= 3:      # quotas were indeed reached: rows were dropped
                    assert int(req["stats"][1]) > int(req["filled"].sum()), tag


def test_partition_second_pass_continues_segments(hip):
    """Two passes into the same segments: the second starts at the counters the first left."""
    req, out, tgt = _case(700, 5, 3, 1, "ample", 7)
    req["quota"].fill_(300)
    req["seg_off"].copy_(torch.tensor([0, 300, 600]))
    dst = torch.full((900, 5), POISON, dtype=torch.float64)
    dreq, ddst = request_to(req, DEV), dst.to(DEV)
    for s in (1, 2, 3):
        _, out2, tgt2 = _case(700, 5, 3, 1, "ample", 7 + s)
        REF.cond_partition(req, out2, tgt2, dst)
        hip.cond_partition(dreq, out2.to(DEV), tgt2.to(DEV), ddst)
    assert torch.equal(ddst.cpu(), dst) and dreq["filled"].tolist() == req["filled"].tolist()
    assert dreq["stats"].tolist() == req["stats"].tolist() and req["stats"][0].item() == 2100
    assert max(req["filled"].tolist()) == 300          # at least one quota was reached on the way


# ----------------------------------------------------------------------------- request kernel
COND = {"cond_offset": [0, 3, 7], "cond_width": [3, 4, 5]}


def _request_setup(m, seed=0):
    g = torch.Generator().manual_seed(seed)
    cond = {k: torch.tensor(v, dtype=torch.int32, device=DEV) for k, v in COND.items()}
    col = torch.randint(0, 3, (m,), generator=g)
    opt = (torch.rand(m, generator=g) * torch.tensor(COND["cond_width"])[col]).long()
    h = torch.zeros(m, 4 + 12)
    h[torch.arange(m), 4 + torch.tensor(COND["cond_offset"])[col] + opt] = 1.0
    h[:, :4] = 0.5
    req = make_request([30000, 10000, 500, 40000], [0, 0, 500, 0], 0, [0.0, 1.0, 2.0, 3.0], span=2,
                       bin_opt=[4, 0, 2, 1], device=DEV)
    return req, cond, col.to(torch.int32).to(DEV), opt.to(torch.int32).to(DEV), h.to(DEV)


def test_request_kernel_draw(hip):
    m = 40960
    req, cond, col, opt, h = _request_setup(m)
    tgt = torch.full((m,), -5, dtype=torch.int32, device=DEV)
    hip.cond_request(req, col, opt, tgt, cond, h=h, c_col0=4, stream_id=24)
    t = tgt.long().cpu()
    assert int(t.min()) >= 0 and not bool((t == 2).any())           # remaining [3, 1, 0, 4] x 10,000: bin 2 is full
    freq = torch.bincount(t, minlength=4).double() / m
    # 8 standard errors at this m (0.5 / sqrt(40,960) = 0.0025)
    assert (freq - torch.tensor([3 / 8, 1 / 8, 0.0, 4 / 8], dtype=torch.float64)).abs().max().item() < 0.02, freq
    assert bool((col == 2).all())
    assert torch.equal(opt.long().cpu(), torch.tensor([4, 0, 2, 1])[t])
    # fp32 activations: one hot element per row, at cond_off[span] + opt; the other columns untouched
    hc = h.cpu()
    assert torch.equal(hc[:, 4:].sum(1), torch.ones(m)) and bool((hc[:, :4] == 0.5).all())
    assert bool((hc[torch.arange(m), 4 + 7 + opt.long().cpu()] == 1.0).all())
    # the same counter gives the same targets, a bumped one others
    req2, _, col2, opt2, _ = _request_setup(m)
    tgt2 = torch.empty_like(tgt)
    hip.cond_request(req2, col2, opt2, tgt2, cond, h=None, stream_id=24)
    assert torch.equal(tgt2, tgt) and torch.equal(opt2, opt)
    hip.L.rng_bump(hip.ctr)
    tgt3 = torch.empty_like(tgt)
    hip.cond_request(req2, col2, opt2, tgt3, cond, h=None, stream_id=24)
    assert int(tgt3.min()) >= 0 and (tgt3 != tgt).float().mean().item() > 0.3
    # every quota full: no targets, conditions and activations as they were
    req["filled"].copy_(req["quota"])
    c0, o0, h0 = col.clone(), opt.clone(), h.clone()
    hip.cond_request(req, col, opt, tgt, cond, h=h, c_col0=4, stream_id=24)
    assert bool((tgt == -1).all()) and torch.equal(col, c0) and torch.equal(opt, o0) and torch.equal(h, h0)


@pytest.mark.parametrize("m", [1, 255, 257])
def test_request_kernel_edges(hip, m):
    """Row counts around the workgroup size: every row gets a target, nothing past the rows is written."""
    req, cond, col, opt, h = _request_setup(m + 3)
    tgt = torch.full((m + 3,), -5, dtype=torch.int32, device=DEV)
    c0, o0, h0 = col.clone(), opt.clone(), h.clone()
    hip.cond_request(req, col, opt, tgt[:m], cond, h=h[:m], c_col0=4, stream_id=24)
    assert bool((tgt[:m] >= 0).all()) and bool((tgt[m:] == -5).all())
    assert torch.equal(col[m:], c0[m:]) and torch.equal(opt[m:], o0[m:]) and torch.equal(h[m:], h0[m:])
    assert torch.equal(h[:m, 4:].sum(1), torch.ones(m, device=DEV))


# ----------------------------------------------------------------------------- engine end to end
def _engine(seed=3, wired=False, **cfg):
    _, _, _, _, _, _, tr, X = small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200, **cfg), DEV, backend="hip", seed=seed)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    if wired:
        wire_generator(eng, tr)
    return eng, tr


@pytest.mark.parametrize("cfg", [{}, {"precision": "fp32"}, {"gen_bf16": False}], ids=["bf16", "fp32", "bf16-h32"])
def test_engine_wired_generator(cfg):
    _, _, _, meta, vocabs, _, _, _ = small_table()
    where = {"class": {"back.": 2, "satan.": 1, "pod.": 1}}
    tabs = []
    for use_graph in (True, False):
        eng, tr = _engine(wired=True, **cfg)
        assert eng.gen16 == (cfg == {})
        req = build_request(tr, meta, vocabs, where, 300, DEV)
        tab = eng.generate_decoded_where(300, req, chunk=128, use_graph=use_graph)
        lc = eng.last_conditional
        check_table(tab, req, meta, vocabs, where)
        assert lc["filled"] == [150, 75, 75]
        # the generator obeys its condition: rows kept == rows generated, ceil(300 / 128) passes
        assert lc["passes"] == 3 and lc["generated"] == 3 * 128 and lc["kept"] == lc["generated"]
        # a fixed column the wired generator answers at random is enforced by rejection alone
        where2 = {"class": "neptune.", "flag": "SF"}
        req2 = build_request(tr, meta, vocabs, where2, 50, DEV)
        tab2 = eng.generate_decoded_where(50, req2, chunk=256, use_graph=use_graph)
        check_table(tab2, req2, meta, vocabs, where2)
        tabs.append((tab, tab2))
        eng.release()
    # equal seeds and states: a replayed pass and eagerly issued launches give the same tables bit for bit
    assert torch.equal(tabs[0][0], tabs[1][0]) and torch.equal(tabs[0][1], tabs[1][1])


def test_engine_bf16_pass_leaves_activations_to_the_sampler():
    """bf16 generation: the request kernel is given no activation buffer (H holds no one-hot block)."""
    eng, tr = _engine()
    _, _, _, meta, vocabs, _, _, _ = small_table()
    req = build_request(tr, meta, vocabs, {"protocol_type": "udp"}, 64, DEV)
    ent = eng._cond_entry(256, 1, 0, 64)
    for k in ("drive", "bin_opt", "bin_code", "quota", "seg_off"):
        ent["req"][k].copy_(req[k])
    assert eng.gen16 and ent["H"].dtype == torch.bfloat16
    eng.ops.sample_gen(eng.gen_cond, ent["H"], eng.c_cols, eng.z_cols, col_out=ent["col"], opt_out=ent["opt"],
                       stream_id=21)
    h0 = ent["H"].clone()
    eng.ops.cond_request(ent["req"], ent["col"], ent["opt"], ent["tgt"], eng.gen_cond, h=None, stream_id=24)
    assert torch.equal(ent["H"], h0) and bool((ent["tgt"] == 0).all())
    assert bool((ent["col"] == req["drive"][0]).all()) and bool((ent["opt"] == 1).all())


def test_engine_random_init_several_passes():
    _, _, _, meta, vocabs, _, _, _ = small_table()
    eng, tr = _engine(seed=5)
    where = {"class": "smurf."}
    req = build_request(tr, meta, vocabs, where, 600, DEV)
    tab = eng.generate_decoded_where(600, req, chunk=1024)
    check_table(tab, req, meta, vocabs, where)
    lc = eng.last_conditional
    assert lc["filled"] == [600] and lc["passes"] >= 2 and lc["generated"] == lc["passes"] * 1024
    assert 600 <= lc["kept"] <= lc["generated"]
    assert bool(torch.isfinite(tab).all())
    # the unconditional pass is untouched by the conditional buffers
    assert eng.generate_decoded(300).shape == (300, len(meta["columns"]))


CHECKED_SCRIPT = r"""
import sys, torch
sys.path[:0] = [{root!r}, {tests!r}]
from fed_tgan_amd.ops import native
from fed_tgan_amd.models.conditional import build_request
from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
from fed_tgan_amd.models.samplers import CondTables
from cond_helpers import check_table, wire_generator
from helpers import small_table
L = native.require()
assert native.CHECKED and L.is_checked(), "checked library not loaded"
_, _, _, meta, vocabs, _, tr, X = small_table()
dev = torch.device("cuda:0")
eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), dev, backend="hip", seed=3)
eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
wire_generator(eng, tr)
where = {{"class": {{"back.": 2, "satan.": 1}}, "flag": "SF"}}
req = build_request(tr, meta, vocabs, where, 120, dev)
tab = eng.generate_decoded_where(120, req, chunk=512)
check_table(tab, req, meta, vocabs, where)
print("CLEAN")
req["drive"][0] = 4000          # a span outside the tables: flagged, never used as an index
try:
    eng.generate_decoded_where(120, req, chunk=512, max_passes=1, use_graph=False)
except RuntimeError as e:
    print("CHECK:", e)
    sys.exit(0)
sys.exit(3)
"""


def test_checked_build_conditional():
    env = dict(os.environ, FEDTGAN_CHECKED="1")
    script = CHECKED_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert r.returncode == 0 and "CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "conditional request index outside its tables" in r.stdout, r.stdout[-2000:]
