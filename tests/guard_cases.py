"""Shared cases of the privacy-guard tests (test_guard.py on the CPU with the torch ops, test_hip_guard.py on the GPU):
the numpy oracle of the radius test (privacy_cases.dist2), thresholds placed between the distances, integer tables
on which every implementation has to agree bit for bit, a decoded pass with a random ``near`` for guard_mark +
cond_partition, and the engine scenarios both backends run.
"""
from __future__ import annotations

import numpy as np
import torch

import privacy_cases as pc
from cond_helpers import check_table, make_request, request_to, wire_generator     # noqa: F401
from fed_tgan_amd.eval import DevicePrivacy, PrivacyGuard
from fed_tgan_amd.models.conditional import ConditionalSamplingError, build_request
from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
from fed_tgan_amd.models.samplers import CondTables

INF = float("inf")
POISON = -777.0

# ----------------------------------------------------------------------------- kernel vs oracle
WITHIN_LAYOUTS = {"cont": (1, 0), "cat": (0, 1), "small": (5, 4), "intrusion": (22, 20), "two-blocks": (30, 25)}
WITHIN_NQ = (1, 257)
WITHIN_NR = (1, 17, 2047, 2049, 4100)      # the LDS-tile edge, the chunk edge, three chunks
# random_packed seeds for which the input conditions below hold (searched on the CPU; 0 where not listed)
WITHIN_SEEDS = {("cont", 257, 2047): 13, ("cont", 257, 2049): 3, ("cont", 1, 2047): 1}
# One continuous column, 257 queries and 4,100 reference rows: the middle values of d1 are ~1e-8 with gaps of ~1e-10,
# and about twenty of the 10^6 pairs lie within 1e-9 of any threshold there, so no seed meets the conditions at the
# middle pair (none of 1,500 does).  There the threshold moves outward from the middle to the nearest pair of adjacent
# distinct d1 values that meets both conditions; everywhere else it sits between the two middle values.
WITHIN_OFF_MIDDLE = {("cont", 257, 4100)}
BAND = 1e-9


def oracle_near(d: np.ndarray, t2: float) -> np.ndarray:
    """the lowest index of a reference row with d2 <= t2, or -1, from the full distance matrix"""
    hit = d <= t2
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1).astype(np.int32)


def conditions(d: np.ndarray, lo: float, hi: float, t2: float):
    """the two input conditions of the kernel test: (the values t2 lies between are more than the band apart, no
    (query, reference) pair lies within the band of t2)"""
    band = BAND * (1.0 + t2)
    return bool(hi - lo > band), not bool((np.abs(d - t2) <= band).any())


def thresholds(d: np.ndarray, off_middle: bool = False):
    """[(lo, hi, t2)]: t2 the midpoint between the two middle distinct values of the sorted d1 (about half the rows
    are flagged).  off_middle: the nearest pair to the middle that meets ``conditions``.  A single distinct d1 (one
    query) has no middle pair: then one threshold above it (d1 + 0.5: flagged) and, where d1 > 0, one below (d1 / 2:
    kept)."""
    u = np.unique(d.min(axis=1))
    if len(u) < 2:
        v = float(u[0])
        return [(v, v + 1.0, v + 0.5)] + ([(0.0, v, 0.5 * v)] if v > 0 else [])
    k = len(u) // 2
    order = [k] if not off_middle else sorted(range(1, len(u)), key=lambda i: (abs(i - k), i))
    for i in order:
        lo, hi = float(u[i - 1]), float(u[i])
        t2 = 0.5 * (lo + hi)
        if not off_middle or all(conditions(d, lo, hi, t2)):
            return [(lo, hi, t2)]
    raise AssertionError("no pair of adjacent d1 values meets the input conditions")


def within_case(layout: str, nq: int, nr: int):
    """(packed arrays, the oracle's distance matrix, thresholds) of one kernel-vs-oracle case"""
    n_cont, n_cat = WITHIN_LAYOUTS[layout]
    packed = pc.random_packed(nq, nr, n_cont, n_cat, seed=WITHIN_SEEDS.get((layout, nq, nr), 0))
    d = pc.dist2(*packed)
    return packed, d, thresholds(d, (layout, nq, nr) in WITHIN_OFF_MIDDLE)


def _t(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)


def device_packed(packed, dev):
    q_cont, q_cat, r_cont, r_cat = packed
    return (_t(q_cont, torch.float64, dev), _t(q_cat, torch.int32, dev), _t(r_cont, torch.float64, dev),
            _t(r_cat, torch.int32, dev))


def run_within(ops, dev, packed, t2: float, guard: int = 3, tensors=None) -> np.ndarray:
    """nn_within of ops -> near (numpy); the output's tail and the scratch past nn_scratch carry a value that has to
    survive"""
    tq = tensors if tensors is not None else device_packed(packed, dev)
    nq, nr = tq[0].shape[0], tq[2].shape[0]
    near = torch.full((nq + guard,), -7, dtype=torch.int32, device=dev)
    used = ops.nn_scratch(nq, nr)
    scratch = torch.full((used + guard,), -7.0, dtype=torch.float64, device=dev)
    ops.nn_within(*tq, torch.tensor([t2], dtype=torch.float64, device=dev), near[:nq], scratch)
    assert bool((near[nq:] == -7).all()) and bool((scratch[used:] == -7.0).all())
    return near[:nq].cpu().numpy()


def check_within_case(ops, dev, layout: str, nq: int, nr: int, top2_ops=None):
    """near equals the oracle's for every row, at every threshold of the case; top2_ops: also (near >= 0) ==
    (d1 <= t2) against its nn_top2 on the same buffers"""
    packed, d, ts = within_case(layout, nq, nr)
    tensors = device_packed(packed, dev)
    for lo, hi, t2 in ts:
        apart, clear = conditions(d, lo, hi, t2)
        assert apart, ("input: the values around t2 are too close", layout, nq, nr, lo, hi)
        assert clear, ("input: a pair lies within the band of t2", layout, nq, nr, t2)
        want = oracle_near(d, t2)
        got = run_within(ops, dev, packed, t2, tensors=tensors)
        print(f"{layout} nq={nq} nr={nr} t2={t2:.6g}: flagged {int((want >= 0).sum())} of {nq}, "
              f"mismatches {int((got != want).sum())}")
        assert np.array_equal(got, want), (layout, nq, nr, t2, np.nonzero(got != want)[0][:8])
        if top2_ops is not None:
            d1 = torch.zeros(nq, dtype=torch.float64, device=dev)
            d2 = torch.zeros(nq, dtype=torch.float64, device=dev)
            i1 = torch.zeros(nq, dtype=torch.int32, device=dev)
            scratch = torch.zeros(top2_ops.nn_scratch(nq, nr), dtype=torch.float64, device=dev)
            top2_ops.nn_top2(*tensors, False, d1, d2, i1, scratch)
            assert np.array_equal(got >= 0, (d1 <= t2).cpu().numpy()), (layout, nq, nr, t2)


# ----------------------------------------------------------------------------- exact integer cases
EXACT_NR = 2 * 2048 + 5       # three chunks, the last one of 5 rows
# real row b copies real row a: in different chunks; in different LDS tiles of one chunk; inside the last chunk
EXACT_TWINS = ((3, 2048 + 7), (20, 20 + 3 * 16), (4096 + 1, 4096 + 3))
EXACT_T2 = (0.0, 1.0, 2.0, 3.0)


def exact_within_case():
    """(packed arrays, special query rows): privacy_cases.exact_case plus a copy of real row 0 and a copy of the last
    row of the last chunk, both rows made unique by a code of their own"""
    real, fake, kinds = pc.exact_case(EXACT_NR, EXACT_TWINS, nq=40, seed=1)
    real[0, 1], real[EXACT_NR - 1, 1] = 30, 31
    fake[-1], fake[-2] = real[0], real[EXACT_NR - 1]
    zero, one = np.zeros(int((kinds == pc.CONT).sum())), np.ones(int((kinds == pc.CONT).sum()))
    packed = pc.pack(fake, kinds, zero, one) + pc.pack(real, kinds, zero, one)
    packed = (packed[0], packed[1].astype(np.int32), packed[2], packed[3].astype(np.int32))
    return packed, {"copy_first": len(fake) - 1, "copy_last": len(fake) - 2}


def check_exact_within(ops, dev) -> dict:
    """integer data: near equals the numpy oracle bit for bit at t2 = 0, 1, 2, 3; returns {t2: near}"""
    packed, rows = exact_within_case()
    d = pc.dist2(*packed)
    assert set(np.unique(d)) <= set(float(i) for i in range(64))           # every distance an exact small integer
    out = {}
    for t2 in EXACT_T2:
        want = oracle_near(d, t2)
        at = (d == t2).any(axis=1)
        assert at.any() and (want[at] >= 0).all()               # a pair at exactly d2 == t2 is flagged: <= is inclusive
        if t2 <= 1.0:                                           # ... also where nothing is closer
            assert (d.min(axis=1) == t2).any()
        got = run_within(ops, dev, packed, t2)
        assert np.array_equal(got, want), (t2, np.nonzero(got != want)[0][:8])
        out[t2] = got
    near0 = out[0.0]
    assert near0[rows["copy_first"]] == 0 and near0[rows["copy_last"]] == EXACT_NR - 1
    for t, (a, b) in enumerate(EXACT_TWINS):
        assert near0[t] == a                            # a copy of a duplicated record: the lower index
        k = len(EXACT_TWINS) + t                        # one categorical column off a twin
        assert near0[k] == -1 and out[1.0][k] == a
    return out


def check_infinite_radius_and_huge_value(ops, dev):
    packed = pc.random_packed(300, 2100, 5, 4, seed=4)
    assert (run_within(ops, dev, packed, INF) == 0).all()
    q_cont = packed[0].copy()
    q_cont[::3, 2] = 1e200                  # the squared difference overflows to +inf: within no finite radius
    near = run_within(ops, dev, (q_cont,) + packed[1:], 3.0)
    assert (near[::3] == -1).all()
    with np.errstate(over="ignore"):
        assert np.array_equal(near, oracle_near(pc.dist2(q_cont, *packed[1:]), 3.0))


# ----------------------------------------------------------------------------- guard_mark + partition
MARK_ROWS = (257, 1500)
MARK_COLS = 7


def mark_case(m: int, mode: str, with_request: bool, seed: int):
    """A random decoded pass with a random ``near``: (req, out, tgt, near, any_value, rows kept in row order per
    bin).  Quotas: ``ample`` (every kept row fits) or ``inside`` (cut mid-pass)."""
    g = torch.Generator().manual_seed(seed)
    out = torch.rand(m, MARK_COLS, generator=g, dtype=torch.float64) + 100.0
    near = torch.where(torch.rand(m, generator=g) < 0.4, torch.randint(0, 5000, (m,), generator=g),
                       torch.full((m,), -1, dtype=torch.int64)).to(torch.int32)
    B = 3 if with_request else 1
    dj = MARK_COLS - 1
    if with_request:
        tgt = torch.randint(-1, B, (m,), generator=g, dtype=torch.int64)
        carried = torch.where(torch.rand(m, generator=g) < 0.7, tgt.clamp_min(0), torch.randint(0, B, (m,), generator=g))
        out[:, dj] = carried.double() * 3.0 + 1.0
        passes = (tgt >= 0) & (out[:, dj] == tgt.clamp_min(0).double() * 3.0 + 1.0)
    else:
        tgt = torch.zeros(m, dtype=torch.int64)
        passes = torch.ones(m, dtype=torch.bool)
    keep = passes & (near < 0)
    kept = [torch.nonzero(keep & (tgt == b)).view(-1) for b in range(B)]
    quota = [m + 1] * B if mode == "ample" else [max(1, int(k.numel()) // 2) for k in kept]
    req = make_request(quota, [0] * B, dj, [b * 3.0 + 1.0 for b in range(B)])
    return req, out, tgt.to(torch.int32), near, not with_request, kept


def check_mark_partition(ops, dev, m: int, mode: str, with_request: bool, seed: int):
    """dst equals the numpy filter in row order, guard_stats is exact, slots beyond the kept rows keep their poison;
    returns (dst, filled, stats, guard_stats, tgt) for the bitwise comparison between backends"""
    req, out, tgt, near, any_value, kept = mark_case(m, mode, with_request, seed)
    quota = req["quota"].tolist()
    n = int(sum(quota))
    want = np.full((n, MARK_COLS), POISON)
    pos = 0
    for q, k in zip(quota, kept):
        rows = k[:q].numpy()
        want[pos:pos + len(rows)] = out.numpy()[rows]
        pos += q
    dreq, dout, dtgt, dnear = request_to(req, dev), out.to(dev), tgt.to(dev), near.to(dev)
    ddst = torch.full((n, MARK_COLS), POISON, dtype=torch.float64, device=dev)
    gstats = torch.tensor([5, 7], dtype=torch.int64, device=dev)        # the counters add to what they held
    ops.guard_mark(dnear, dtgt, gstats)
    ops.cond_partition(dreq, dout, dtgt, ddst, any_value=any_value)
    tag = (m, mode, with_request)
    assert np.array_equal(ddst.cpu().numpy(), want), tag
    assert gstats.tolist() == [5 + m, 7 + int((near >= 0).sum())], tag
    assert dreq["filled"].tolist() == [min(q, int(k.numel())) for q, k in zip(quota, kept)], tag
    assert dreq["stats"].tolist() == [m, int(sum(k.numel() for k in kept))], tag
    assert torch.equal(dtgt.cpu(), torch.where(near >= 0, torch.full_like(tgt, -1), tgt)), tag
    if mode == "inside":
        assert any(int(k.numel()) > q for q, k in zip(quota, kept)), tag        # rows were indeed dropped
    return ddst.cpu(), dreq["filled"].cpu(), dreq["stats"].cpu(), gstats.cpu(), dtgt.cpu()


# ----------------------------------------------------------------------------- engine scenarios
def make_engine(dev, backend: str, seed: int = 3, wired: bool = False):
    _, _, _, _, _, _, tr, X = pc.small_table()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200), dev, backend=backend, seed=seed)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    if wired:
        wire_generator(eng, tr)
    return eng, tr


def unmatched_real_row():
    """a one-row real table carrying a category code no vocabulary holds: no generated row is within T = 0 of it"""
    _, _, _, meta, _, enc, _, _ = pc.small_table()
    row = np.asarray(enc, dtype=np.float64)[:1].copy()
    j = next(j for j, c in enumerate(meta["columns"]) if c["type"] == "categorical")
    row[0, j] = 10000.0
    return row


def deterministic_rejection(dev, backend: str, use_graph, where=None, n: int = 300, chunk: int = 128):
    """Run 1 guards against a row nothing matches: the table X.  Run 2, a fresh engine from the same seed, guards
    against X[0::2] at T = 0.  Returns (X, out) on the CPU after the checks that hold on every backend."""
    _, _, _, meta, vocabs, _, _, _ = pc.small_table()
    tabs = []
    for run in (1, 2):
        torch.manual_seed(17)           # (the torch backend draws from torch's global generator)
        eng, tr = make_engine(dev, backend, wired=where is not None)
        real = unmatched_real_row() if run == 1 else tabs[0][0::2].cpu().numpy()
        guard = PrivacyGuard(real, meta, vocabs, dev, min_dcr=0.0, ops=eng.ops)
        req = build_request(tr, meta, vocabs, where, n, dev) if where is not None else None
        tab = eng.generate_decoded_guarded(n, guard, request=req, chunk=chunk, use_graph=use_graph)
        lg = eng.last_guard
        assert tab.shape == (n, len(meta["columns"])) and lg["kept"] == n
        assert lg["generated"] == lg["passes"] * chunk
        if req is not None:
            check_table(tab, req, meta, vocabs, where)
            assert eng.last_conditional["filled"] == req["quotas"] and eng.last_conditional["passes"] == lg["passes"]
        if run == 1:
            assert lg["rejected"] == 0
            assert len(np.unique(tab.cpu().numpy(), axis=0)) == n, "input: X has duplicate rows"
        else:
            X = tabs[0]
            ev = DevicePrivacy(real, meta, vocabs, dev, ops=eng.ops, max_rows=n, baseline=False)
            s = ev.score(tab)
            assert float(s.floats()["copies"]) == 0.0 and bool((ev.d1[:n] > 0).all())
            if where is None:
                assert torch.equal(tab[:n // 2], X[1::2])
                assert lg["rejected"] >= n // 2
            else:
                assert lg["rejected"] > 0
        tabs.append(tab)
        if hasattr(eng, "release"):
            eng.release()
    return tabs[0].cpu(), tabs[1].cpu()


def radius_scenario(dev, backend: str, n: int = 300):
    """T = the median unguarded DCR against small_table's real rows: every kept row is scored at d1 > t2"""
    _, _, _, meta, vocabs, enc, _, _ = pc.small_table()
    torch.manual_seed(23)
    eng, _ = make_engine(dev, backend, seed=9)
    ev = DevicePrivacy(np.asarray(enc, dtype=np.float64), meta, vocabs, dev, ops=eng.ops, max_rows=n, baseline=False)
    T = float(ev.score(eng.generate_decoded(n)).rows()[0].median())
    assert T > 0
    guard = ev.guard(T)
    assert guard.r_cont is ev.r_cont and guard.r_cat is ev.r_cat and float(guard.t2) == T * T
    tab = eng.generate_decoded_guarded(n, guard)
    lg = eng.last_guard
    assert tab.shape[0] == n and lg["kept"] == n and lg["rejected"] > 0
    assert lg["generated"] - lg["rejected"] >= n
    ev.score(tab)
    assert bool((ev.d1[:n] > guard.t2).all())
    flagged, near = guard.near(tab)
    assert not bool(flagged.any()) and bool((near == -1).all())
    if hasattr(eng, "release"):
        eng.release()


def exhaustion_scenario(dev, backend: str, m: int = 128):
    _, _, _, meta, vocabs, enc, _, _ = pc.small_table()
    eng, _ = make_engine(dev, backend)
    guard = PrivacyGuard(np.asarray(enc, dtype=np.float64)[:200], meta, vocabs, dev, min_dcr=1e3, ops=eng.ops)
    tab = None
    try:
        tab = eng.generate_decoded_guarded(50, guard, max_passes=2, chunk=m)
    except ConditionalSamplingError as e:
        assert "rejected 256 of 256" in str(e) and "100.0 %" in str(e), str(e)
    else:
        raise AssertionError("no ConditionalSamplingError")
    assert tab is None
    lg = eng.last_guard
    assert lg["rejected"] == lg["generated"] == 2 * m and lg["kept"] == 0 and lg["passes"] == 2
    if hasattr(eng, "release"):
        eng.release()
