"""Completion of partial rows on the HIP backend: known_request and known_match against the torch ops (bit for bit
on exact cases, within one rounding per term on random ones), and the engine end to end (eager against replayed
passes, the wired generator, candidates re-matched on the CPU, the bounds-checked build)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import known_cases as kc
from cond_helpers import wire_generator
from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
from fed_tgan_amd.models.known import build_known
from fed_tgan_amd.models.samplers import CondTables
from fed_tgan_amd.ops.ref import TorchOps
from helpers import small_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = TorchOps()
TRIES = (1, 2, 63, 64, 65, 256, 1024)
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def hip():
    from fed_tgan_amd.ops import native
    from fed_tgan_amd.ops.hip import HipOps
    native.require()
    return HipOps(DEV, seed=1234)


def _to(state):
    return {k: v.to(DEV) for k, v in state.items()}


# ----------------------------------------------------------------------------- request kernel
@pytest.mark.parametrize("q", [1, 3, 64])
def test_request_matches_reference_bitwise(hip, q):
    assert hip.KNOWN_MAX_TRIES == REF.KNOWN_MAX_TRIES == 1024
    changed = kept = 0
    for R in TRIES:
        assert q * R <= 65536
        for with_h in (True, False):
            case = kc.request_case(q, R, seed=q * 2000 + R)
            m = q * R
            # three rows past the pass carry a poison that has to survive
            pad = lambda t, v: torch.cat([t, torch.full((3,) + t.shape[1:], v, dtype=t.dtype)])      # noqa: E731
            col, opt, h = case["col"].clone(), case["opt"].clone(), case["h"].clone()
            REF.known_request(case["qidx"], case["drv_span"], case["drv_opt"], R, col, opt, case["cond"],
                              h=h if with_h else None, c_col0=4)
            dcol, dopt, dh = pad(case["col"], -9).to(DEV), pad(case["opt"], -9).to(DEV), pad(case["h"], 7.0).to(DEV)
            cond = {k: v.to(DEV) for k, v in case["cond"].items()}
            hip.known_request(case["qidx"].to(DEV), case["drv_span"].to(DEV), case["drv_opt"].to(DEV), R, dcol, dopt,
                              cond, h=dh if with_h else None, c_col0=4)
            tag = (q, R, with_h)
            assert torch.equal(dcol[:m].cpu(), col) and torch.equal(dopt[:m].cpu(), opt), tag
            assert torch.equal(dh[:m].cpu(), h if with_h else case["h"]), tag
            assert bool((dcol[m:] == -9).all()) and bool((dopt[m:] == -9).all()) and bool((dh[m:] == 7.0).all()), tag
            live = (case["qidx"] >= 0).repeat_interleave(R)
            drv = case["drv_span"][case["qidx"].long().clamp_min(0)].repeat_interleave(R) >= 0
            same = (col == case["col"]) & (opt == case["opt"])
            assert bool(same[~(live & drv)].all()), tag              # untouched rows stay bit-equal
            changed += int((~same).sum())
            kept += int((~(live & drv)).sum())
    assert changed > 0 and (kept > 0 or q == 1)


# ----------------------------------------------------------------------------- match kernel, exact cases
def _exact_variants():
    for R in TRIES:
        yield R, "random", "mixed"
    for R in (65, 256):
        for mm, sm in (("none", "mixed"), ("all", "mixed"), ("random", "cont"), ("random", "cat")):
            yield R, mm, sm


@pytest.mark.parametrize("n_cols", [1, 3, 42, 65, 130, 512])
def test_match_exact_cases_bitwise(hip, n_cols):
    ties = improved = stayed = 0
    for v, (R, mm, sm) in enumerate(_exact_variants()):
        q = 5 if R * n_cols <= 65536 else 3
        case = kc.exact_case(q, R, n_cols, mm, sm, seed=n_cols * 100 + v)
        N = case["N"]
        st, dst = kc.fresh_state(N), kc.fresh_dst(N, n_cols)
        dstate, ddst = _to(kc.fresh_state(N)), kc.fresh_dst(N, n_cols, DEV)
        # two consecutive passes over the same queries: the second has to beat the best so far strictly
        passes = kc.two_passes(case, n_cols * 100 + v + 5000)
        for p, cand in enumerate(passes):
            kc.run_match(REF, case, st, dst, cand=cand)
            kc.run_match(hip, case, dstate, ddst, cand=cand, device=DEV)
            tag = (n_cols, R, mm, sm, p)
            assert kc.state_equal(dstate, st), tag
            assert torch.equal(ddst.cpu().view(torch.int64), dst.view(torch.int64)), tag      # poison included
            if p == 0:
                d2 = kc.d2_matrix(case, cand)
                live = case["qidx"] >= 0
                ties += int(((d2[live] == d2[live].min(1, keepdim=True).values).sum(1) > 1).sum())
        live = case["qidx"][case["qidx"] >= 0].long()
        improved += int((st["pick"][live] >= R).sum())
        stayed += int((st["pick"][live] < R).sum())
        assert st["seen"][live].tolist() == [2 * R] * live.numel()
    # the cases are not vacuous: equal distances occur, and the second pass wins for some queries and not for others
    assert ties > 0 and improved > 0 and stayed > 0, (ties, improved, stayed)


# ----------------------------------------------------------------------------- match kernel, random cases
@pytest.mark.parametrize("n_cols, R", [(42, 64), (42, 65), (130, 256), (65, 1024), (512, 63)])
def test_match_random_cases_within_rounding(hip, n_cols, R):
    case = kc.random_case(6, R, n_cols, seed=n_cols + R)
    N = case["N"]
    n_cont = int((case["kind"] == 0).sum())
    bound = (n_cont + 1) * ULP          # one rounding per term: the fused multiply-add rounds once, the torch op twice
    st, dst = kc.fresh_state(N), kc.fresh_dst(N, n_cols)
    dstate, ddst = _to(kc.fresh_state(N)), kc.fresh_dst(N, n_cols, DEV)
    kc.run_match(REF, case, st, dst)
    kc.run_match(hip, case, dstate, ddst, device=DEV)
    hs = {k: v.cpu() for k, v in dstate.items()}
    kc.agree(case, hs, st, ddst.cpu(), dst, bound)
    rest = torch.ones(N, dtype=torch.bool)
    rest[case["qidx"][case["qidx"] >= 0].long()] = False
    assert bool((ddst.cpu()[rest] == kc.POISON).all()) and hs["seen"][rest].tolist() == [0] * int(rest.sum())


# ----------------------------------------------------------------------------- engine end to end
def _engine(seed=3, wired=False, **cfg):
    _, _, _, _, _, _, tr, X = small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200, **cfg), DEV, backend="hip", seed=seed)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    if wired:
        wire_generator(eng, tr)
    return eng, tr


def _partial(n, seed, p_known=0.5):
    _, _, _, _, _, enc, _, _ = small_table()
    rng = np.random.default_rng(seed)
    enc = np.asarray(enc)
    known = np.ascontiguousarray(enc[np.arange(n) % len(enc)], dtype=np.float64)
    return known, (rng.random(known.shape) < p_known).astype(np.uint8)


def test_engine_eager_against_replayed_bitwise():
    """chunk 384 = 24 slots of 16 tries: N = 1 leaves 23 slots idle, N = 100 takes 5 passes (the last with 4 live
    slots), N = 1025 takes 43."""
    engines = [_engine(seed=5)[0] for _ in range(2)]
    for N in (1, 100, 1025):
        known, mask = _partial(N, N)
        got = []
        for eng, use_graph in zip(engines, (True, False)):
            out = eng.generate_decoded_known(known, mask, tries=16, retries=1, chunk=384, use_graph=use_graph)
            st = eng._known_ent[(384, 16)]["state"]
            got.append((out, {k: v[:N].clone() for k, v in st.items()}, dict(eng.last_known)))
        assert torch.equal(got[0][0].view(torch.int64), got[1][0].view(torch.int64)), N
        assert kc.state_equal(got[0][1], got[1][1]) and got[0][2] == got[1][2], N
        lk = got[0][2]
        assert lk["rows"] == N and lk["generated"] == sum(-(-n // 24) for n in [N] + lk["open"][:-1]) * 384
        on = torch.from_numpy(mask != 0)
        assert torch.equal(got[0][0].cpu()[on].view(torch.int64), torch.from_numpy(known)[on].view(torch.int64))
        assert bool(torch.isfinite(got[0][0]).all())
    assert engines[0]._known_ent[(384, 16)]["graph"] is not None and engines[1]._known_ent[(384, 16)]["graph"] is None
    for eng in engines:
        eng.release()


@pytest.mark.parametrize("cfg", [{}, {"precision": "fp32"}], ids=["bf16", "fp32"])
def test_engine_wired_generator(cfg):
    eng, tr = _engine(wired=True, **cfg)
    known, mask = _partial(90, 0)
    mask[0] = 0
    mask[1] = 1
    cat = [j for j, m in enumerate(tr.meta) if m["type"] != "continuous"]
    for r in range(2, 12):                           # rows that know exactly one category: their driver
        mask[r, cat] = 0
        mask[r, cat[r % len(cat)]] = 1
    out = eng.generate_decoded_known(known, mask, tries=4, retries=1, chunk=64).cpu().numpy()
    lk = eng.last_known
    on = mask != 0
    assert np.array_equal(out[on].view(np.int64), known[on].view(np.int64)) and np.array_equal(out[1], known[1])
    tab = build_known(tr, eng.gen_counts, known, mask)
    drove = np.isin(tab["drv_span"], cat)
    miss = eng._known_ent[(64, 4)]["state"]["miss"][:90].cpu().numpy()
    n_cat = on[:, cat].sum(1)
    # the generator obeys its condition: a row whose only known category is its driver misses none
    assert (n_cat == 1).sum() > 0 and (miss[n_cat == 1] == 0).all() and (miss[drove] < n_cat[drove]).all()
    assert lk["sweeps"] == len(lk["open"]) <= 2 and lk["d_p50"] <= lk["d_p95"] <= lk["d_max"]
    # nothing known: candidate 0 of the row's slot in the first pass, which is what plain generation puts there
    eng2, _ = _engine(wired=True, **cfg)
    plain = eng2.generate_decoded(64, use_graph=False)
    assert np.array_equal(out[0], plain[0].cpu().numpy())
    eng.release()
    eng2.release()


def test_engine_one_categorical_column_is_exact_without_retry():
    from fed_tgan_amd.features.transformer import VGMTransformer
    rng = np.random.default_rng(0)
    data = np.stack([rng.normal(size=600), rng.integers(0, 4, 600).astype(float), rng.normal(size=600) * 3], 1)
    tr = VGMTransformer().fit(data, (1,), (), seed=0, backend="sklearn")
    X = tr.transform(data, np.random.default_rng(0))
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=100, gen_dims=(32,), dis_dims=(32,), embedding_dim=16), DEV,
                      backend="hip", seed=1)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    wire_generator(eng, tr)
    known = data[:70].copy()
    mask = np.zeros((70, 3), dtype=np.uint8)
    mask[:, 1] = 1
    out = eng.generate_decoded_known(known, mask, tries=8, retries=2, chunk=200).cpu().numpy()
    lk = eng.last_known
    assert (out[:, 1] == known[:, 1]).all() and lk["exact_categorical"] == 1.0
    assert lk["open"] == [0] and lk["sweeps"] == 1 and lk["generated"] == 3 * 200
    eng.release()


def test_engine_pass_rematched_on_the_cpu():
    """The candidates of one HIP pass, judged again by the torch op on the CPU, under the random-case rule."""
    eng, tr = _engine(seed=7)
    N, R, q = 40, 16, 24
    known, mask = _partial(N, 11)
    tab = build_known(tr, eng.gen_counts, known, mask)
    ent = eng._known_entry(q * R, R, N)
    for k in ("known", "mask", "drv_span", "drv_opt"):
        ent[k][:N].copy_(torch.from_numpy(tab[k]))
    ent["kind"].copy_(torch.from_numpy(tab["kind"]))
    ent["scale"].copy_(torch.from_numpy(tab["scale"]))
    ent["state"]["best"].fill_(float("inf"))
    ent["dst"].fill_(kc.POISON)
    g = torch.Generator().manual_seed(0)
    case = {"known": torch.from_numpy(tab["known"]), "mask": torch.from_numpy(tab["mask"]),
            "qidx": kc.slots(q, N, g), "tries": R, "kind": torch.from_numpy(tab["kind"]),
            "scale": torch.from_numpy(tab["scale"]), "N": N}
    ent["qidx"].copy_(case["qidx"])
    eng._known_pass(ent, q * R, R)
    case["cand"] = ent["out"].cpu()
    st, dst = kc.fresh_state(N), kc.fresh_dst(N, known.shape[1])
    kc.run_match(REF, case, st, dst)
    n_cont = int((case["kind"] == 0).sum())
    hs = {k: v[:N].cpu() for k, v in ent["state"].items()}
    kc.agree(case, hs, st, ent["dst"][:N].cpu(), dst, (n_cont + 1) * ULP)
    assert bool(torch.isfinite(case["cand"]).all())
    eng.release()


CHECKED_SCRIPT = r"""
import sys, numpy as np, torch
sys.path[:0] = [{root!r}, {tests!r}]
from fed_tgan_amd.ops import native
from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
from fed_tgan_amd.models.generator_io import LoadedGenerator
from fed_tgan_amd.models.samplers import CondTables
from helpers import small_table
L = native.require()
assert native.CHECKED and L.is_checked(), "checked library not loaded"
_, df, _, meta, vocabs, _, tr, X = small_table()
dev = torch.device("cuda:0")
eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), dev, backend="hip", seed=3)
eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
gen = LoadedGenerator("Intrusion", eng, tr, meta, vocabs)
part = df.iloc[:50].reset_index(drop=True).astype(object)
part = part.mask(np.random.default_rng(0).random(part.shape) < 0.5, "")
vals = gen.complete(part, tries=8, retries=1)
assert vals.shape == (50, len(meta["columns"])) and np.isfinite(vals).all()
print("CLEAN", eng.last_known["sweeps"])
"""


def test_checked_build_complete():
    env = dict(os.environ, FEDTGAN_CHECKED="1")
    script = CHECKED_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert r.returncode == 0 and "CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
