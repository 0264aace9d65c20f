"""Operands that a kernel requests before the work they follow (clamped addresses, masked afterwards) at the shapes
where an early load can go wrong, on the normal and on the bounds-checked library.

activate_rowblk_kernel requests the fused slerp's condition columns and its interpolation draw with the logits,
ahead of the softmax's barriers: a row narrower than a workgroup (lanes past D, condition block narrower than the
threads), rows with and without an interpolate in one launch.
chain_epilogue_kernel (prefetching instantiations) requests the tail epilogue's bias, mask or head-seed factors and
dropout counter with the tail weights: an odd row count, so the last two-row workgroup's second row is past the
end."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from fed_tgan_amd.ops import native
    from fed_tgan_amd.ops.hip import HipOps
    L = native.require()
    assert bool(L.is_checked()) == native.CHECKED
    return HipOps(DEV, seed=1234)


# D = 70 (two 64-column blocks, the second 6 wide; a softmax span across the block edge), 9 condition columns
SPANS_70 = [(0, 1, 0), (1, 7, 1), (8, 1, 0), (9, 13, 1), (22, 1, 0), (23, 36, 1), (59, 1, 0), (60, 10, 1)]


def test_activation_with_slerp_narrow_rows(hip):
    """5 rows of which 3 are interpolated: the fused launch equals activation followed by the standalone slerp
    (same Philox stream), to the exactness tests/test_hip_ops.py holds the Intrusion-sized case to; rows without an
    interpolate and every column outside the launch's outputs stay as they were."""
    D, nc, rows, nsl = 70, 9, 5, 3
    assert sum(w for _, w, _ in SPANS_70) == D
    g = torch.Generator(device="cpu").manual_seed(7)
    logits = (torch.randn(rows, D, generator=g) * 2).to(DEV)
    xd = torch.randn(2 * rows + nsl, D + nc + 3, generator=g).to(DEV)    # [fake | real | interp], 3 padding columns
    xd2 = xd.clone()
    Din = D + nc
    fake, real, interp = xd[0:rows, :Din], xd[rows:2 * rows, :Din], xd[2 * rows:, :Din]
    hip.activate(logits, fake[:, :D], SPANS_70, 0.2, stream_id=2, slerp=(real[:nsl], fake, interp, 3))
    fake2, real2, interp2 = xd2[0:rows, :Din], xd2[rows:2 * rows, :Din], xd2[2 * rows:, :Din]
    hip.activate(logits, fake2[:, :D], SPANS_70, 0.2, stream_id=2)
    hip.slerp(real2[:nsl], fake2[:nsl], interp2, stream_id=3)
    torch.cuda.synchronize()
    assert torch.equal(xd[0:2 * rows], xd2[0:2 * rows])          # activation, condition columns, real rows, padding
    assert torch.equal(xd[2 * rows:, Din:], xd2[2 * rows:, Din:])
    assert bool(torch.isfinite(interp).all())
    assert torch.allclose(interp, interp2, atol=2e-6, rtol=1e-5)


def _chain(hip, kind, M, splitk, pre, rows):
    """Head [M, 256] = epi(x W0^T [+ b0]) with the tail [M, 256] chained into its reduction launch: the D0 -> D1
    forward (bias, LeakyReLU + dropout, the head seed A1) or the R0 -> R1 link (mask products)."""
    from fed_tgan_amd.ops.hip import EPI_LRELU_DROPOUT, EPI_MASK
    g = torch.Generator(device="cpu").manual_seed(11 * M)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    x, W0, b0, W1, b1, coef, v = r(M, 200), r(256, 200), r(256), r(256, 256), r(256), r(M), r(256)
    m0 = (torch.rand(M, 256, generator=g) > 0.5).float().to(DEV) * 2
    m1 = (torch.rand(M, 256, generator=g) > 0.5).float().to(DEV) * 0.4
    dl0, dl1, A1 = (torch.full((M, 256), -7.0, device=DEV) for _ in range(3))
    p0 = torch.ops.fedtgan.set_tuning("chain_pre", pre)
    r0 = torch.ops.fedtgan.set_tuning("chain_rows", rows)
    try:
        if kind == "d":
            ms0, ms1 = torch.zeros(M, 256, device=DEV), torch.zeros(M, 256, device=DEV)
            hip.gemm(dl0, W1, dl1, tb=True, bias=b1, epi=EPI_LRELU_DROPOUT, ms=ms1, stream_id=5, head=(coef, v, A1),
                     group=4)
            hip.gemm(x, W0, dl0, tb=True, bias=b0, epi=EPI_LRELU_DROPOUT, ms=ms0, stream_id=4, chain=True,
                     splitk=splitk)
        else:
            ms0, ms1 = m0, m1
            hip.gemm(dl0, W1, dl1, tb=True, epi=EPI_MASK, ms=ms1, group=4)
            hip.gemm(x, W0, dl0, tb=True, epi=EPI_MASK, ms=ms0, chain=True, splitk=splitk)
        torch.cuda.synchronize()
    finally:
        torch.ops.fedtgan.set_tuning("chain_pre", p0)
        torch.ops.fedtgan.set_tuning("chain_rows", r0)
    return dl0, ms0, dl1, ms1, A1


# M = 3: one head row per workgroup; M = 131: 524 one-row workgroups are too many for the prefetch, so two rows per
# workgroup, and the second row of the last pair is past the end
@pytest.mark.parametrize("kind", ["d", "r"])
@pytest.mark.parametrize("M,splitk,pre,rows", [(3, 2, 2, 1), (3, 1, 2, 1), (131, 2, 1, 2)])
def test_chained_tail_epilogue_operands(hip, kind, M, splitk, pre, rows):
    """chain_epilogue_kernel with the tail's weights and epilogue operands requested up front equals the plain
    chain (chain_pre = 0: operands loaded where they are used) bit for bit, as tests/test_hip_engine.py holds the
    engine's chains to."""
    want = _chain(hip, kind, M, splitk, 0, 1)
    got = _chain(hip, kind, M, splitk, pre, rows)
    for nm, a, b in zip(("head", "ms0", "tail", "ms1", "A1"), got, want):
        assert torch.equal(a, b), (nm, float((a - b).abs().max()))
    assert bool((got[2] != -7.0).any())


def test_same_cases_on_the_checked_library():
    """The cases above in a process that loads the bounds-checked build (one native library per process)."""
    env = dict(os.environ, FEDTGAN_CHECKED="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "not checked_library"], env=env, capture_output=True, text=True, timeout=150, cwd=ROOT)
    assert r.returncode == 0 and "passed" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
