"""Shared builders of the partial-row completion tests (CPU and HIP): cases of the known_request / known_match ops.

Exact cases live on a dyadic grid -- known values and candidates are small integers, scales 1 or 1/2 -- so every
term ((known - cand) * scale)^2 is a multiple of 1/4 below 16 and every sum of at most 1024 of them is exact in
float64, whatever rounds once or twice: the fused kernel and the torch op must agree bit for bit, and because only
four values occur, equal distances (ties) are everywhere.  Random cases use full-precision doubles."""
from __future__ import annotations

import torch

POISON = -777.0
STATE_KEYS = ("best", "dc", "miss", "seen", "pick")


def schema(n_cols, mode, g):
    """(kind int32, scale float64): mode 'mixed' (about half categorical), 'cont' or 'cat'."""
    if mode == "cont":
        kind = torch.zeros(n_cols, dtype=torch.int32)
    elif mode == "cat":
        kind = torch.ones(n_cols, dtype=torch.int32)
    else:
        kind = torch.randint(0, 2, (n_cols,), generator=g, dtype=torch.int32)
    scale = torch.where(torch.rand(n_cols, generator=g) < 0.5, 1.0, 0.5).double()
    return kind, scale


def masks(N, n_cols, mode, g):
    if mode == "none":
        return torch.zeros(N, n_cols, dtype=torch.uint8)
    if mode == "all":
        return torch.full((N, n_cols), 3, dtype=torch.uint8)       # any non-zero byte means known
    return (torch.rand(N, n_cols, generator=g) < 0.5).to(torch.uint8)


def slots(q, N, g, idle=True):
    """qidx int32 [q]: distinct queries in random order, about a quarter of the slots idle (at least one live)."""
    perm = torch.randperm(N, generator=g)[:q]
    qidx = torch.full((q,), -1, dtype=torch.int32)
    qidx[:perm.numel()] = perm.to(torch.int32)
    if idle and q > 1:
        off = torch.rand(q, generator=g) < 0.25
        off[0] = False
        qidx[off] = -1
    return qidx[torch.randperm(q, generator=g)]


def exact_case(q, R, n_cols, mask_mode="random", schema_mode="mixed", seed=0, N=None):
    g = torch.Generator().manual_seed(seed)
    N = N if N is not None else q + 3
    kind, scale = schema(n_cols, schema_mode, g)
    known = torch.randint(0, 4, (N, n_cols), generator=g).double()
    mask = masks(N, n_cols, mask_mode, g)
    known = torch.where(mask != 0, known, torch.full_like(known, float("nan")))     # unknown cells are never read
    return {"known": known, "mask": mask, "qidx": slots(q, N, g), "tries": R, "kind": kind, "scale": scale,
            "cand": exact_candidates(q, R, n_cols, seed + 1000), "N": N}


def exact_candidates(q, R, n_cols, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 4, (q * R, n_cols), generator=g).double()


def two_passes(case, seed):
    """(first, second) candidate tables of an exact case for the best-so-far checks.  The first pass's values lie
    in 4..7, off every known value (0..3), so a query that knows a cell starts with d2 > 0.  In the second pass an
    even slot sees its first candidates in reverse order -- the same smallest distance, which must not replace the
    best so far -- and an odd slot random candidates whose last row repeats the query's known cells (d2 = 0)."""
    q, R, n = case["qidx"].numel(), case["tries"], case["known"].shape[1]
    first = case["cand"] + 4.0
    second = exact_candidates(q, R, n, seed).view(q, R, n)
    second[0::2] = first.view(q, R, n)[0::2].flip(1)
    for s in range(1, q, 2):
        i = int(case["qidx"][s])
        if i >= 0:
            second[s, R - 1] = torch.nan_to_num(case["known"][i], nan=0.0)
    return first, second.reshape(q * R, n).contiguous()


def random_case(q, R, n_cols, seed=0, N=None):
    g = torch.Generator().manual_seed(seed)
    N = N if N is not None else q + 3
    kind, _ = schema(n_cols, "mixed", g)
    scale = torch.rand(n_cols, generator=g, dtype=torch.float64) + 0.25
    known = torch.randn(N, n_cols, generator=g, dtype=torch.float64)
    cand = torch.randn(q * R, n_cols, generator=g, dtype=torch.float64)
    cat = kind != 0
    known[:, cat] = torch.randint(0, 3, (N, int(cat.sum())), generator=g).double()
    cand[:, cat] = torch.randint(0, 3, (q * R, int(cat.sum())), generator=g).double()
    mask = masks(N, n_cols, "random", g)
    return {"known": known, "mask": mask, "qidx": slots(q, N, g), "tries": R, "kind": kind, "scale": scale,
            "cand": cand, "N": N}


def fresh_state(N, device="cpu"):
    return {"best": torch.full((N,), float("inf"), dtype=torch.float64, device=device),
            "dc": torch.zeros(N, dtype=torch.float64, device=device),
            "miss": torch.zeros(N, dtype=torch.int32, device=device),
            "seen": torch.zeros(N, dtype=torch.int64, device=device),
            "pick": torch.zeros(N, dtype=torch.int64, device=device)}


def fresh_dst(N, n_cols, device="cpu"):
    return torch.full((N, n_cols), POISON, dtype=torch.float64, device=device)


def run_match(ops, case, state, dst, cand=None, device="cpu"):
    """known_match of ``ops`` over a case (tensors moved to ``device``); state and dst are updated in place."""
    t = lambda k: case[k].to(device)      # noqa: E731
    ops.known_match(t("known"), t("mask"), t("qidx"), case["tries"], (case["cand"] if cand is None else cand).to(device),
                    t("kind"), t("scale"), state, dst)


def d2_of(case, i, row):
    """The torch-op distance of one candidate row to query i (float64, column order)."""
    acc, ms = torch.zeros((), dtype=torch.float64), 0
    for j in range(case["known"].shape[1]):
        if case["mask"][i, j] == 0:
            continue
        if case["kind"][j] == 0:
            d = (case["known"][i, j] - row[j]) * case["scale"][j]
            acc = acc + d * d
        else:
            ms += int(row[j] != case["known"][i, j])
    return float(acc + float(ms))


def state_equal(a, b):
    return all(torch.equal(a[k].cpu(), b[k].cpu()) for k in STATE_KEYS)


def request_case(q, R, seed=0, width=(3, 4, 5)):
    """A known_request case over three spans: (qidx, drv_span, drv_opt, col, opt, h, cond) on the CPU; h is the fp32
    activation buffer with 4 leading columns and the one-hot block of the sampler's draw."""
    g = torch.Generator().manual_seed(seed)
    N, m = q + 3, q * R
    off = [0]
    for w in width[:-1]:
        off.append(off[-1] + w)
    cond = {"cond_offset": torch.tensor(off, dtype=torch.int32), "cond_width": torch.tensor(width, dtype=torch.int32)}
    col = torch.randint(0, len(width), (m,), generator=g)
    opt = (torch.rand(m, generator=g) * torch.tensor(width)[col]).long()
    h = torch.zeros(m, 4 + sum(width))
    h[torch.arange(m), 4 + torch.tensor(off)[col] + opt] = 1.0
    h[:, :4] = 0.5
    drv_span = torch.randint(-1, len(width), (N,), generator=g)
    drv_opt = (torch.rand(N, generator=g) * torch.tensor(width)[drv_span.clamp_min(0)]).long()
    return {"qidx": slots(q, N, g), "drv_span": drv_span.to(torch.int32), "drv_opt": drv_opt.to(torch.int32),
            "tries": R, "col": col.to(torch.int32), "opt": opt.to(torch.int32), "h": h, "cond": cond}


def d2_matrix(case, cand=None):
    """The torch-op distances of every candidate of every slot, float64 [q, R] (idle slots: NaN), on the CPU."""
    cand = case["cand"] if cand is None else cand
    R, q, n = case["tries"], case["qidx"].numel(), case["known"].shape[1]
    i = case["qidx"].long().clamp_min(0)
    K, M = case["known"][i], case["mask"][i] != 0
    C = cand[:q * R].view(q, R, n)
    acc = torch.zeros(q, R, dtype=torch.float64)
    ms = torch.zeros(q, R, dtype=torch.float64)
    zero = torch.zeros((), dtype=torch.float64)
    for j, kd in enumerate(case["kind"].tolist()):
        if kd == 0:
            d = (K[:, j, None] - C[:, :, j]) * case["scale"][j]
            acc = acc + torch.where(M[:, j, None], d * d, zero)
        else:
            ms = ms + (M[:, j, None] & (C[:, :, j] != K[:, j, None])).double()
    d2 = acc + ms
    d2[case["qidx"] < 0] = float("nan")
    return d2


def agree(case, hip_state, ref_state, hip_dst, ref_dst, bound, seen0=None, cand=None):
    """The random-case rule after one pass from equal states: best and dc agree within the relative ``bound``; where
    the picks differ, the torch op's d2 of both picks agree within it (a near tie decided by rounding), and the HIP
    row is then the HIP pick's completed row.  Returns the number of differing picks."""
    cand = case["cand"] if cand is None else cand
    R = case["tries"]
    d2 = d2_matrix(case, cand)
    differ = 0
    for s, i in enumerate(case["qidx"].tolist()):
        if i < 0:
            continue
        for k in ("best", "dc"):
            a, b = float(hip_state[k][i]), float(ref_state[k][i])
            assert abs(a - b) <= bound * max(abs(a), abs(b)), (k, s, i, a, b)
        base = 0 if seen0 is None else int(seen0[i])
        ph, pr = int(hip_state["pick"][i]), int(ref_state["pick"][i])
        assert int(hip_state["seen"][i]) == int(ref_state["seen"][i])
        known = case["mask"][i] != 0
        if ph == pr:
            assert int(hip_state["miss"][i]) == int(ref_state["miss"][i])
            assert torch.equal(hip_dst[i], ref_dst[i]), (s, i)
            continue
        differ += 1
        assert base <= ph < base + R and base <= pr < base + R, (s, i, ph, pr)
        a, b = float(d2[s, ph - base]), float(d2[s, pr - base])
        assert abs(a - b) <= bound * max(abs(a), abs(b)), (s, i, ph, pr, a, b)
        want = torch.where(known, case["known"][i], cand[s * R + ph - base])
        assert torch.equal(hip_dst[i], want), (s, i)
    return differ
