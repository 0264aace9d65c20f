"""The numpy restatement of the step's Philox draws (tests/rng_cases.py) checked on the CPU: against Random123's known
answer, against the tree evaluator's independent Python-integer Philox, and at the edges the GPU tests rely on."""
import numpy as np
import pytest

import rng_cases as rc


def test_philox_known_answer():
    """Random123 kat_vectors: philox4x32-10 of the zero counter under the zero key"""
    w = rc.philox4(0, 0, 0, 0)
    assert [int(v) for v in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_philox_matches_python_integer_restatement():
    """50 mixed counters, some with step >= 2^32 (the key's high word) and idx >= 2^32 (the counter's second word)"""
    from forest_cases import philox_word
    rng = np.random.default_rng(7)
    seen_step_hi = seen_idx_hi = 0
    for k in range(50):
        seed = int(rng.integers(0, 1 << 62))
        stream = int(rng.integers(0, 1 << 32))
        step = int(rng.integers(0, 1 << 20)) + ((int(rng.integers(1, 1 << 20)) << 32) if k % 3 == 0 else 0)
        idx = int(rng.integers(0, 1 << 30)) + ((int(rng.integers(1, 1 << 12)) << 32) if k % 4 == 0 else 0)
        seen_step_hi += step >= 1 << 32
        seen_idx_hi += idx >= 1 << 32
        key = seed ^ ((step >> 32) << 32)        # (seed lo, seed hi ^ step hi)
        want = philox_word(key, stream, step & 0xFFFFFFFF, idx >> 32, idx & 0xFFFFFFFF)
        assert int(rc.philox4(seed, stream, step, idx)[0]) == want, (seed, stream, step, idx)
    assert seen_step_hi >= 10 and seen_idx_hi >= 10


def test_philox_vectorised_equals_scalar():
    idx = np.array([0, 1, 63, (5 << 20) + 64, (1 << 32) + 3], dtype=np.int64)
    step = (1 << 32) + 5
    words = rc.philox4(99, 32, step, idx)
    for k, i in enumerate(idx):
        assert [int(w[k]) for w in words] == [int(w) for w in rc.philox4(99, 32, step, int(i))]
    # the step's high word enters the key: it changes the draw
    assert int(rc.philox4(99, 32, 5, 0)[0]) != int(rc.philox4(99, 32, step, 0)[0])


def test_u01_range():
    """u01 covers [2^-25, 1.0]: the top 256 words round up to exactly 1.0 (the consumers clamp)"""
    assert rc.u01(0xFFFFFFFF) == np.float32(1.0) and rc.u01(0xFFFFFF00) == np.float32(1.0)
    assert rc.u01(0xFFFFFEFF) < np.float32(1.0)
    assert rc.u01(0) == np.float32(2.0 ** -25) and rc.u01(255) == np.float32(2.0 ** -25)
    assert rc.u01(np.uint32(0x80000000)).dtype == np.float32
    assert rc.u01d(0xFFFFFFFF, 0xFFFFFFFF) <= 1.0 and rc.u01d(0, 0) == 2.0 ** -54
    # the guards: the clamped Gumbel value is finite, and Box-Muller of a top-of-range word is finite and tiny
    assert np.isclose(rc.gumbel(0xFFFFFFFF), rc.GUMBEL_TOP) and np.isfinite(rc.gumbel(0))
    c, s = rc.box_muller(0xFFFFFFFF, 0xFFFFFFFF)
    assert abs(c) < 1e-14 and abs(s) < 1e-14


@pytest.mark.parametrize("n", [1, 2, 3, 37, 64, 65, 500])
def test_feistel_is_a_bijection(n):
    for seed in (1, 2, 3):
        key = [int(w) for w in rc.philox4(seed, 17, 5, 0)]
        assert sorted(rc.feistel_perm(b, n, key) for b in range(n)) == list(range(n))


def test_edge_seeds_reach_the_top_of_the_range():
    """The constants the GPU tests use: word x (y) of (stream 16, step 0, idx 0) has its top 24 bits set"""
    for s in rc.EDGE_SEEDS_X:
        assert int(rc.philox4(s, rc.EDGE_STREAM, 0, 0)[0]) >> 8 == 0xFFFFFF
        assert rc.u01(rc.philox4(s, rc.EDGE_STREAM, 0, 0)[0]) == np.float32(1.0)
    for s in rc.EDGE_SEEDS_Y:
        assert int(rc.philox4(s, rc.EDGE_STREAM, 0, 0)[1]) >> 8 == 0xFFFFFF


def test_cond_request_oracle_skips_full_bins():
    quota, filled = np.array([3, 0, 5, 2, 0]), np.array([3, 0, 1, 0, 0])
    t = rc.cond_request(11, 384, 0, 500, quota, filled)
    assert set(np.unique(t)) == {2, 3}
    assert (rc.cond_request(11, 384, 0, 9, quota, quota) == -1).all()


def test_near_tie_share_of_the_gpu_cases():
    """The argmax checks of the GPU tests leave out spans whose top two perturbed logits are closer than 1e-3 in the
    oracle; that share must stay below 1% (asserted on the oracle alone, for the cases' own logits)."""
    import hip_rng_cases as hc
    for name, share in hc.near_tie_shares():
        assert share <= 0.01, (name, share)


# effective streams of every call site that is not a D dropout GEMM (docs/ARCHITECTURE.md): stream_id * 16, the sampler + 0..3
OTHER_STREAMS = ({16, 17, 18, 19, 32, 48} | {176, 177, 178, 179, 192} | {336, 337, 338, 339, 352, 368, 384})


@pytest.mark.parametrize("depth", range(1, 9))
def test_d_dropout_streams_are_distinct_up_to_eight_layers(depth):
    from fed_tgan_amd.models.engine import d_dropout_stream
    d = [d_dropout_stream(4, i) for i in range(depth)]
    g = [d_dropout_stream(14, i) for i in range(depth)]
    assert len(set(d + g)) == 2 * depth and not set(d + g) & OTHER_STREAMS
    # the default two-layer D keeps the streams it always had
    assert d[:2] == [4, 5][:depth] and g[:2] == [14, 15][:depth]
