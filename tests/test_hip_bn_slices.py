"""Sliced training BatchNorm (set_tuning("bn_slices", S)): every output bit-identical to the one-workgroup kernel
(bn_slices = 1), outputs fully written, padding untouched, and the cases that must fall back to that kernel."""
import pytest
import torch

from fed_tgan_amd.data.demo import small_table
from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENT = -12345.0
NAMES = ("out", "nhat", "mean", "invstd", "rm", "rv")


@pytest.fixture(scope="module")
def hip():
    from fed_tgan_amd.ops import native
    from fed_tgan_amd.ops.hip import HipOps
    native.require()
    return HipOps(DEV, seed=1234)


def _inputs(rows, cols, scale, offset, pad):
    g = torch.Generator(device="cpu").manual_seed(rows * 1000 + cols)
    abuf = (torch.randn(rows, cols + pad, generator=g) * scale + offset).to(DEV)
    gamma = (torch.rand(cols, generator=g) + 0.5).to(DEV)
    beta = torch.randn(cols, generator=g).to(DEV)
    rm0 = torch.randn(cols, generator=g).to(DEV)
    rv0 = (torch.rand(cols, generator=g) + 0.5).to(DEV)
    return abuf, gamma, beta, rm0, rv0


def _run(hip, inp, cols, pad, slices, groups=2, threads=512, alias=False):
    """One launch under bn_slices = slices on sentinel-filled outputs; returns the six tensors and the out / nhat
    buffers with their padding columns."""
    abuf, gamma, beta, rm0, rv0 = inp
    rows = abuf.shape[0]
    abuf = abuf.clone()
    a = abuf[:, :cols]
    obuf = abuf if alias else torch.full((rows, cols + 2 * pad), SENT, device=DEV)
    nbuf = torch.full((rows, cols + 3 * pad), SENT, device=DEV)
    out, nhat = obuf[:, :cols], nbuf[:, :cols]
    mean = torch.full((groups, cols), SENT, device=DEV)
    inv = torch.full((groups, cols), SENT, device=DEV)
    rm, rv = rm0.clone(), rv0.clone()
    prev_s = torch.ops.fedtgan.set_tuning("bn_slices", slices)
    prev_t = torch.ops.fedtgan.set_tuning("bn_threads", threads)
    try:
        hip.bn_relu_fwd(a, gamma, beta, out, nhat, mean, inv, rm, rv, True, 0.1, 1e-5, groups=groups)
        torch.cuda.synchronize()
    finally:
        torch.ops.fedtgan.set_tuning("bn_threads", prev_t)
        torch.ops.fedtgan.set_tuning("bn_slices", prev_s)
    return (out, nhat, mean, inv, rm, rv), (obuf, nbuf)


SHAPES = {
    "partial": (2 * 37, 20, 3.0, 1.0, 0),        # partial column block, rows no multiple of the row groups
    "padded": (2 * 250, 300, 3.0, 1.0, 5),       # padded leading dimensions (a, out and nhat each their own)
    "illcond": (2 * 40, 8, 0.05, 50.0, 0),       # tiny spread around a large mean
}
_base = {}


def _baseline(hip, key):
    # the bn_slices = 1 result of a shape: computed once, shared by the cases, never modified
    if key not in _base:
        rows, cols, scale, offset, pad = SHAPES[key]
        inp = _inputs(rows, cols, scale, offset, pad)
        _base[key] = (inp, _run(hip, inp, cols, pad, 1))
    return _base[key]


@pytest.mark.parametrize("slices", [2, 4])
@pytest.mark.parametrize("key", list(SHAPES))
def test_sliced_equals_unsliced(hip, key, slices):
    rows, cols, scale, offset, pad = SHAPES[key]
    inp, (want, _) = _baseline(hip, key)
    got, (obuf, nbuf) = _run(hip, inp, cols, pad, slices)
    for nm, x, y in zip(NAMES, got, want):
        assert not bool((x == SENT).any()), nm            # fully written
        assert torch.equal(x, y), (nm, float((x - y).abs().max()))
    assert bool((obuf[:, cols:] == SENT).all()) and bool((nbuf[:, cols:] == SENT).all())   # padding untouched


@pytest.mark.parametrize("case", ["groups1", "rows600", "threads1024", "alias"])
def test_fallbacks_equal_unsliced(hip, case):
    rows, cols, groups, threads, alias = {
        "groups1": (500, 20, 1, 512, False),
        "rows600": (2 * 600, 20, 2, 512, False),     # more than 16 rows per thread
        "threads1024": (2 * 250, 20, 2, 1024, False),
        "alias": (2 * 250, 20, 2, 512, True),        # out written over a
    }[case]
    inp = _inputs(rows, cols, 3.0, 1.0, 0)
    want, _ = _run(hip, inp, cols, 0, 1, groups, threads, alias)
    got, _ = _run(hip, inp, cols, 0, 2, groups, threads, alias)
    for nm, x, y in zip(NAMES, got, want):
        assert not bool((x == SENT).any()), nm
        assert torch.equal(x, y), nm


def test_engine_steps_bit_identical():
    """16 captured steps (two replays of the 8-step graph): parameters and Adam moments of G and D are the same
    bits under bn_slices = 1 and 2.  (The logged metrics are float atomics and differ between two runs of one
    build, so they are not compared.)"""
    from fed_tgan_amd.ops import native
    native.require()
    _, _, _, _, _, _, tr, X = small_table()
    res = []
    for slices in (1, 2):
        prev = torch.ops.fedtgan.set_tuning("bn_slices", slices)
        try:
            torch.manual_seed(0)
            eng = CTGANEngine(tr.layout, EngineConfig(batch_size=500), DEV, backend="hip", seed=3)
            eng.set_training_data(X)
            eng.train_steps(16, use_graph=True)
            torch.cuda.synchronize()
        finally:
            torch.ops.fedtgan.set_tuning("bn_slices", prev)
        res.append([t.clone() for t in (eng.flat, eng.mD, eng.vD, eng.mG, eng.vG)])
    for nm, x, y in zip(("flat", "mD", "vD", "mG", "vG"), *res):
        assert bool(torch.isfinite(x).all()), nm
        assert torch.equal(x, y), nm
