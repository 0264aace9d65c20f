"""The training step's and the generation pass's Philox draws, restated in plain numpy from csrc/kernels/common.h and
the kernels' comments: which counter, which of the four words and which stream every kernel body reads, and what the
draw decides.

Nothing here uses torch or a project kernel.  Almost everything a draw decides is integer arithmetic or exactly
reproducible IEEE fp32 / fp64 (u01, u01 * n_col, cdf > u, the Feistel network, u01d * cnt, the dropout keep bit), so
the tests demand equality for those; the Gumbel / Box-Muller values are evaluated here in fp64 and compared within a
tolerance that only a wrong counter can miss.

Streams are the EFFECTIVE stream numbers a kernel receives (HipOps passes ``stream_id * 16`` to every kernel except the
GEMM, which gets ``stream_id`` raw).
"""
from __future__ import annotations

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
U64 = np.uint64


# ----------------------------------------------------------------------------- Philox4x32-10 (common.h rng4)
def philox4(seed, stream, step, idx):
    """Four uint32 arrays: the words of counter (idx lo, idx hi, stream, step lo) under the key
    (seed lo, seed hi ^ step hi).  Vectorised over any of the arguments (broadcast)."""
    seed, stream, step, idx = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) for v in (seed, stream, step, idx)))
    c0, c1, c2, c3 = idx & M32, idx >> U64(32), stream & M32, step & M32
    k0, k1 = seed & M32, ((seed >> U64(32)) ^ (step >> U64(32))) & M32
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c0, U64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> U64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + U64(0x9E3779B9)) & M32, (k1 + U64(0xBB67AE85)) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def u01(x):
    """fp32, exactly as written: (float(x >> 8) + 0.5f) * 2^-24.  Range [2^-25, 1.0]: for x >> 8 == 0xFFFFFF the sum
    16777215.5 is a tie and rounds to 16777216, so the value is exactly 1.0 (probability 2^-24)."""
    x = np.asarray(x, dtype=np.uint32)
    return ((x >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def u01d(a, b):
    """fp64: ((a << 21 ^ b) mod 2^53 + 0.5) * 2^-53"""
    v = ((np.asarray(a, dtype=np.uint64) << U64(21)) ^ np.asarray(b, dtype=np.uint64)) & U64((1 << 53) - 1)
    return (v.astype(np.float64) + 0.5) * (2.0 ** -53)


def neg_log_u(x):
    return np.maximum(-np.log(u01(x).astype(np.float64)), 1e-30)


def gumbel(x):
    return -np.log(neg_log_u(x))


GUMBEL_TOP = -np.log(1e-30)     # the clamped value a top-of-range word (u01 == 1.0) gives


def box_muller(a, b):
    r = np.sqrt(2.0 * neg_log_u(a))
    th = 2.0 * np.pi * u01(b).astype(np.float64)
    return r * np.cos(th), r * np.sin(th)


def _component(words, comp):
    """words[comp[...]][...] for a tuple of four same-shape arrays"""
    return np.choose(comp, words)


# ----------------------------------------------------------------------------- sampler (sample_kernel)
def feistel_perm(x, n, key):
    """The keyed permutation of [0, n): 4 Feistel rounds on the smallest even number of bits covering n (at least 2),
    keyed by the four words ``key``, with cycle walking."""
    bits = 2
    while (1 << bits) < n:
        bits += 2
    h = bits // 2
    mask = (1 << h) - 1
    x = int(x)
    while True:
        L, R = x >> h, x & mask
        for r in range(4):
            f = ((R ^ int(key[r])) * 0x9E3779B1) & 0xFFFFFFFF
            f ^= f >> 15
            f = (f * 0x85EBCA77) & 0xFFFFFFFF
            f ^= f >> 13
            L, R = R, L ^ (f & mask)
        x = (L << h) | R
        if x < n:
            return x


def cond_draw(seed, stream, step, b, cdf, cond_w):
    """(col, opt) of batch rows ``b``: col from word x, u from word y of (stream, step, b); the option is the first
    i < w with cdf[col, i] > u (an fp32 compare), else w - 1."""
    b = np.asarray(b, dtype=np.int64)
    n_col = len(cond_w)
    x, y, _, _ = philox4(seed, stream, step, b)
    col = np.minimum((u01(x) * np.float32(n_col)).astype(np.int32), n_col - 1)
    u = u01(y)
    opt = np.empty_like(col)
    for k in range(len(b)):
        w = int(cond_w[col[k]])
        hit = np.nonzero(np.asarray(cdf[col[k], :w], dtype=np.float32) > u[k])[0]
        opt[k] = hit[0] if len(hit) else w - 1
    return col, opt


def noise(seed, stream, step, B, E):
    """z [B, E] in fp64: z[b, 2i], z[b, 2i+1] = Box-Muller of words x, y of (stream + 2, step, b * E + i)"""
    half = (E + 1) // 2
    idx = np.arange(B, dtype=np.int64)[:, None] * E + np.arange(half, dtype=np.int64)[None, :]
    x, y, _, _ = philox4(seed, stream + 2, step, idx)
    c, s = box_muller(x, y)
    z = np.empty((B, 2 * half))
    z[:, 0::2], z[:, 1::2] = c, s
    return z[:, :E]


def sampler(seed, stream, step, B, E, cdf, cond_w, n_real=0, row_off=None, row_cnt=None, rows=None):
    """One sampler launch.  Rows [0, n_real) also get a real row: row b serves the condition of fake row
    p = perm(b) (Feistel over n_real keyed by the four words of (stream + 1, step, 0)) and takes entry
    floor(u01d(x, y of (stream + 3, step, b)) * cnt), clamped, of that condition's CSR cell."""
    allb = np.arange(B)
    col, opt = cond_draw(seed, stream, step, allb, cdf, cond_w)
    out = {"col": col, "opt": opt, "z": noise(seed, stream, step, B, E)}
    if n_real:
        key = [int(w) for w in philox4(seed, stream + 1, step, 0)]
        perm = np.array([feistel_perm(b, n_real, key) for b in range(n_real)])
        pcol, popt = col[perm], opt[perm]
        x, y, _, _ = philox4(seed, stream + 3, step, np.arange(n_real))
        u = u01d(x, y)
        cnt = np.asarray(row_cnt)[pcol, popt].astype(np.int64)
        off = np.asarray(row_off)[pcol, popt].astype(np.int64)
        pick = (u * np.maximum(cnt, 1).astype(np.float64)).astype(np.int64)
        pick = np.where(pick >= cnt, np.where(cnt > 0, cnt - 1, 0), pick)
        out.update(perm=perm, pcol=pcol, popt=popt, row=np.asarray(rows)[off + pick])
    return out


# ----------------------------------------------------------------------------- activation (activate_* kernels)
def activation_words(seed, stream, step, R, D):
    """[R, D] uint32: element j of row r reads component (j // 64) % 4 of counter (r << 20) + (j // 256) * 64 + j % 64"""
    j = np.arange(D, dtype=np.int64)[None, :]
    r = np.arange(R, dtype=np.int64)[:, None]
    idx = (r << 20) + (j // 256) * 64 + j % 64
    return _component(philox4(seed, stream, step, idx), np.broadcast_to((j // 64) % 4, idx.shape))


def activate(x, spans, tau, seed, stream, step):
    """fp64 tanh / softmax((x + g) / tau) per span (kind 0 = tanh) and the perturbed logits (x + g) / tau"""
    x = np.asarray(x, dtype=np.float64)
    g = gumbel(activation_words(seed, stream, step, *x.shape))
    pert = (x + g) / tau
    out = np.empty_like(x)
    for s, w, k in spans:
        if k == 0:
            out[:, s:s + w] = np.tanh(x[:, s:s + w])
        else:
            p = pert[:, s:s + w]
            e = np.exp(p - p.max(1, keepdims=True))
            out[:, s:s + w] = e / e.sum(1, keepdims=True)
    return out, pert


def top_two_gap(v):
    """[R] gap between the largest and the second largest entry of each row (inf for one entry)"""
    if v.shape[1] < 2:
        return np.full(v.shape[0], np.inf)
    t = np.partition(v, v.shape[1] - 2, axis=1)
    return t[:, -1] - t[:, -2]


def slerp_alpha(seed, stream, step, R):
    """fused and standalone slerp: alpha of row r = u01(word x of (slerp stream, step, r)), fp32"""
    return u01(philox4(seed, stream, step, np.arange(R))[0])


def slerp(real, fake, alpha):
    """fp64 slerp of the rows (the reference's formula; linear when the angle degenerates)"""
    a, b = np.asarray(real, dtype=np.float64), np.asarray(fake, dtype=np.float64)
    al = np.asarray(alpha, dtype=np.float64)[:, None]
    cosw = (a * b).sum(1) / (np.sqrt((a * a).sum(1)) * np.sqrt((b * b).sum(1)))
    om = np.arccos(np.clip(cosw, -1.0, 1.0))[:, None]
    so = np.sin(om)
    with np.errstate(divide="ignore", invalid="ignore"):
        wa = np.where(so < 1e-6, 1.0 - al, np.sin((1.0 - al) * om) / so)
        wb = np.where(so < 1e-6, al, np.sin(al * om) / so)
    return wa * a + wb * b


# ----------------------------------------------------------------------------- GEMM dropout (gemm.hip apply_epi)
def dropout_keep(seed, stream, step, M, N, p):
    """[M, N] bool: keep iff u01(word x of (stream, step, m * N + n)) >= p (fp32 compare)"""
    idx = np.arange(M, dtype=np.int64)[:, None] * N + np.arange(N, dtype=np.int64)[None, :]
    return u01(philox4(seed, stream, step, idx)[0]) >= np.float32(p)


# ----------------------------------------------------------------------------- generation decode (sample_decode_*)
def decode_perturbed(x, cols, seed, stream, step):
    """Per output column (kind, start, width): the fp64 perturbed logits [R, width].  Position i of a span at offset
    off (the span start, + 1 for a continuous column: kind 0) reads component i & 3 of counter
    (r << 20) + off + (i & ~3)."""
    x = np.asarray(x, dtype=np.float64)
    R = x.shape[0]
    r = np.arange(R, dtype=np.int64)[:, None]
    res = []
    for kind, start, width in cols:
        off = start + 1 if kind == 0 else start
        i = np.arange(width, dtype=np.int64)[None, :]
        idx = (r << 20) + off + (i & ~3)
        w = _component(philox4(seed, stream, step, idx), np.broadcast_to(i & 3, idx.shape))
        res.append(x[:, off:off + width] + gumbel(w))
    return res


def decode_choice(x, cols, seed, stream, step):
    """([R, n_cols] argmax position, the first maximum winning; [R, n_cols] top-two gap)"""
    pert = decode_perturbed(x, cols, seed, stream, step)
    return (np.stack([p.argmax(1) for p in pert], 1), np.stack([top_two_gap(p) for p in pert], 1))


# ----------------------------------------------------------------------------- conditional request (cond_request_kernel)
def cond_request(seed, stream, step, B, quota, filled):
    """[B] target bin: r = floor(u01d(x, y of (stream, step, b)) * total), clamped, over the open quota
    (remaining_i = max(quota_i - filled_i, 0)); the first bin whose running remainder exceeds r.  -1 when all are full."""
    rem = np.maximum(np.asarray(quota, dtype=np.int64) - np.asarray(filled, dtype=np.int64), 0)
    total = int(rem.sum())
    if total <= 0:
        return np.full(B, -1, dtype=np.int64)
    x, y, _, _ = philox4(seed, stream, step, np.arange(B))
    r = np.minimum((u01d(x, y) * float(total)).astype(np.int64), total - 1)
    return np.searchsorted(np.cumsum(rem), r, side="right").astype(np.int64)


# ----------------------------------------------------------------------------- top-of-range words
# Seeds below 2^26 whose word of (stream 16, step 0, idx 0) has x >> 8 == 0xFFFFFF, i.e. u01 == 1.0 (found by an
# offline scan; tests/test_rng_oracle.py verifies them)
EDGE_STREAM = 16
EDGE_SEEDS_X = (20246534, 26093342)
EDGE_SEEDS_Y = (14165500, 17349328)
