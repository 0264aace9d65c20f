"""The privacy guard on the HIP backend: nn_within against the numpy oracle on every row and against nn_top2 on the same
buffers, the integer cases bit for bit between HIP, torch and numpy, guard_mark + the partition against the reference
ops, and CTGANEngine.generate_decoded_guarded end to end (replayed hipGraph against eager launches, with a request, a
radius, exhaustion, the bounds-checked build)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guard_cases as gc
import privacy_cases as pc
from fed_tgan_amd.ops.ref import TorchOps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = TorchOps()


@pytest.fixture(scope="module")
def hip():
    from fed_tgan_amd.ops import native
    from fed_tgan_amd.ops.hip import HipOps
    native.require()
    return HipOps(DEV, seed=1234)


# ----------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("nr", gc.WITHIN_NR)
@pytest.mark.parametrize("layout", list(gc.WITHIN_LAYOUTS))
def test_within_matches_oracle_on_every_row(hip, layout, nr):
    """The threshold sits between the two middle distinct values of the oracle's d1 (guard_cases.thresholds; the one
    case that cannot is listed there), both input conditions are asserted first, then near must equal the oracle's
    for every row and (near >= 0) == (d1 <= t2) with the HIP nn_top2's d1."""
    for nq in gc.WITHIN_NQ:
        gc.check_within_case(hip, DEV, layout, nq, nr, top2_ops=hip)


def test_exact_cases_bitwise(hip):
    got = gc.check_exact_within(hip, DEV)            # against numpy
    want = gc.check_exact_within(REF, "cpu")
    for t2 in gc.EXACT_T2:
        assert np.array_equal(got[t2], want[t2]), t2


def test_within_is_deterministic(hip):
    packed, d, ts = gc.within_case("intrusion", 257, 4100)
    a = gc.run_within(hip, DEV, packed, ts[0][2])
    b = gc.run_within(hip, DEV, packed, ts[0][2])
    assert a.tobytes() == b.tobytes()


def test_infinite_radius_and_huge_value(hip):
    gc.check_infinite_radius_and_huge_value(hip, DEV)


@pytest.mark.parametrize("with_request", [False, True], ids=["plain", "request"])
@pytest.mark.parametrize("mode", ["ample", "inside"])
def test_mark_and_partition_bitwise(hip, mode, with_request):
    for seed, m in enumerate(gc.MARK_ROWS):
        got = gc.check_mark_partition(hip, DEV, m, mode, with_request, seed)
        want = gc.check_mark_partition(REF, "cpu", m, mode, with_request, seed)
        for g, w in zip(got, want):
            assert torch.equal(g, w), (m, mode, with_request)


# ----------------------------------------------------------------------------- engine
def test_engine_deterministic_rejection_graph_and_eager():
    tabs = [gc.deterministic_rejection(DEV, "hip", use_graph=g) for g in (True, False)]
    # equal seeds and states: a replayed pass and eagerly issued launches give the same tables bit for bit
    assert torch.equal(tabs[0][0], tabs[1][0]) and torch.equal(tabs[0][1], tabs[1][1])


def test_engine_deterministic_rejection_with_request():
    where = {"class": {"back.": 2, "satan.": 1}}
    tabs = [gc.deterministic_rejection(DEV, "hip", use_graph=g, where=where) for g in (True, False)]
    assert torch.equal(tabs[0][0], tabs[1][0]) and torch.equal(tabs[0][1], tabs[1][1])


def test_engine_radius():
    gc.radius_scenario(DEV, "hip")


def test_engine_exhaustion():
    gc.exhaustion_scenario(DEV, "hip")


def test_unguarded_paths_are_untouched():
    """a guarded run in between changes nothing of the plain and the conditional tables of an engine"""
    _, _, _, meta, vocabs, _, _, _ = pc.small_table()
    where = {"class": "smurf."}
    tabs = []
    for guarded in (False, True):
        eng, tr = gc.make_engine(DEV, "hip", seed=5)
        if guarded:
            ctr = eng.ops.ctr.clone()
            guard = gc.PrivacyGuard(gc.unmatched_real_row(), meta, vocabs, DEV, ops=eng.ops)
            eng.generate_decoded_guarded(100, guard, chunk=128)
            eng.ops.ctr.copy_(ctr)
        req = gc.build_request(tr, meta, vocabs, where, 200, DEV)
        tabs.append((eng.generate_decoded(300), eng.generate_decoded_where(200, req, chunk=512)))
        eng.release()
    assert torch.equal(tabs[0][0], tabs[1][0]) and torch.equal(tabs[0][1], tabs[1][1])


CHECKED_SCRIPT = r"""
import sys, torch
sys.path[:0] = [{root!r}, {tests!r}]
from fed_tgan_amd.ops import native
import guard_cases as gc
import privacy_cases as pc
L = native.require()
assert native.CHECKED and L.is_checked(), "checked library not loaded"
_, _, _, meta, vocabs, enc, _, _ = pc.small_table()
dev = torch.device("cuda:0")
eng, tr = gc.make_engine(dev, "hip", wired=True)
where = {{"class": {{"back.": 2, "satan.": 1}}, "flag": "SF"}}
req = gc.build_request(tr, meta, vocabs, where, 120, dev)
guard = gc.PrivacyGuard(enc[:500].astype("float64"), meta, vocabs, dev, min_dcr=0.25, ops=eng.ops)
tab = eng.generate_decoded_guarded(120, guard, request=req, chunk=512)
gc.check_table(tab, req, meta, vocabs, where)
assert not bool(guard.near(tab)[0].any())
tab = eng.generate_decoded_guarded(120, guard, chunk=256)
assert tab.shape[0] == 120 and not bool(guard.near(tab)[0].any())
print("CLEAN")
"""


def test_checked_build_guard():
    env = dict(os.environ, FEDTGAN_CHECKED="1")
    script = CHECKED_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert r.returncode == 0 and "CLEAN" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
