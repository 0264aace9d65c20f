"""Every Philox draw of the training step and the generation pass against the numpy oracle (tests/rng_cases.py): which
counter, word and stream each kernel body reads.  What a draw decides in integers or exact fp32 / fp64 is compared for
equality; Gumbel / Box-Muller values against the oracle's fp64 within a tolerance only a wrong address can miss."""
import functools

import numpy as np
import pytest
import torch

import hip_rng_cases as hc
import rng_cases as rc
from helpers import small_table, table_spans

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPI_LRELU_DROPOUT = 1
# fp32 evaluation of a Gumbel / Box-Muller value or of the softmax over them is good to about 1e-5; a wrong counter,
# word or stream moves the value by O(1).  This is an addressing tolerance, not a precision claim.
ADDR_TOL = 1e-3
# slerp of O(1) rows with weights from fp32 sums over up to 7,045 columns: about 1e-5; a wrong alpha moves it by O(0.1)
SLERP_TOL = 1e-4


def new_ops(seed, step, precision="bf16"):
    from fed_tgan_amd.ops.hip import HipOps
    o = HipOps(DEV, seed=seed, precision=precision)
    o.ctr.fill_(step)
    return o


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def onehot(hot, C):
    out = np.zeros((len(hot), C), dtype=np.float32)
    out[np.arange(len(hot)), hot] = 1.0
    return out


# ============================================================================ sampler
S_WIDTHS = (3, 70, 130)          # 70 and 130: the CDF search continues past its first 64-entry chunk
S_ROWS = 400
S_OFF = np.concatenate([[0], np.cumsum(S_WIDTHS)[:-1]]).astype(np.int32)
S_C = int(sum(S_WIDTHS))
S_STREAM_ID = 1                  # effective streams 16..19


@functools.lru_cache(maxsize=None)
def sampler_tables(Dd):
    """Hand-built tables: cdf [3, 130] fp32 (entries past a column's width are 2.0: a search that ignored the width
    would stop there), a 400-row matrix and its CSR row lists per (column, option).  Column 0: option 0 holds 399
    rows, option 1 one row (cnt == 1) and option 2 none (cnt == 0; its offset points at the next column's first
    entry, inside the array)."""
    rng = np.random.default_rng(3)
    maxw = max(S_WIDTHS)
    cdf = np.full((len(S_WIDTHS), maxw), 2.0, dtype=np.float32)
    cats = []
    for c, w in enumerate(S_WIDTHS):
        p = rng.random(w) + 0.05
        cdf[c, :w] = (np.cumsum(p) / p.sum()).astype(np.float32)
        cdf[c, w - 1] = 1.0
        cats.append(rng.integers(0, w, S_ROWS))
    cdf[0, :3] = [1.0 / 3, 2.0 / 3, 1.0]
    cats[0][:] = 0
    cats[0][123] = 1
    row_off = np.zeros((len(S_WIDTHS), maxw), dtype=np.int64)
    row_cnt = np.zeros_like(row_off)
    rows, pos = [], 0
    for c in range(len(S_WIDTHS)):
        for o in range(maxw):
            r = np.nonzero(cats[c] == o)[0] if o < S_WIDTHS[c] else np.zeros(0, dtype=np.int64)
            row_off[c, o], row_cnt[c, o] = pos, len(r)
            rows.append(rng.permutation(r))
            pos += len(r)
    rows = np.concatenate(rows).astype(np.int64)
    assert row_cnt[0, 1] == 1 and row_cnt[0, 2] == 0 and row_off[0, 2] < len(rows)
    data = rng.standard_normal((S_ROWS, Dd)).astype(np.float32)
    return {"cdf": cdf, "row_off": row_off, "row_cnt": row_cnt, "rows": rows, "data": data}


def run_sampler(ops, B, E, Dd, n_real, zc=2, draws=1, bf16=False, step_init=7.0):
    """One sampler launch on the hand-built tables; returns the buffers as numpy (per draw, stacked)."""
    t = sampler_tables(Dd)
    L = ops.L
    cc = zc + E
    col = torch.full((draws * B,), -9, dtype=torch.int32, device=DEV)
    opt = torch.full((draws * B,), -9, dtype=torch.int32, device=DEV)
    cdf, coff, cw = dev(t["cdf"]), dev(S_OFF), dev(np.asarray(S_WIDTHS, dtype=np.int32))
    if bf16:
        h = torch.full((B, zc + E + (zc & 1)), 9.0, dtype=torch.bfloat16, device=DEV)
        L.sample(h, zc, cc, E, None, None, 0, cdf, coff, cw, None, None, None, None, col, opt, None, None, None, False,
                 ops.seed, ops.ctr, S_STREAM_ID * 16)
        torch.cuda.synchronize()
        return {"h": h.float().cpu().numpy(), "col": col.cpu().numpy(), "opt": opt.cpu().numpy()}
    W, Wx = cc + S_C, Dd + S_C
    h_all = torch.full((draws * B, W), 9.0, device=DEV)
    x_all = torch.full((draws * (n_real + B), Wx), 9.0, device=DEV)       # per draw: [real rows | fake rows]
    sc = torch.full((2, draws), 0.0, device=DEV)
    sc[:, draws - 1] = step_init                                           # the canonical (last) counter entries
    metrics = torch.ones(draws, 4, device=DEV)
    extra = (draws, B * W, (n_real + B) * Wx, B) if draws > 1 else ()
    L.sample(h_all[:B], zc, cc, E, x_all[n_real:n_real + B], x_all[:n_real] if n_real else None, Dd, cdf, coff, cw,
             dev(t["row_off"]), dev(t["row_cnt"]), dev(t["rows"]), dev(t["data"]), col[:B], opt[:B], sc[0], sc[1],
             metrics, True, ops.seed, ops.ctr, S_STREAM_ID * 16, *extra)
    torch.cuda.synchronize()
    x = x_all.view(draws, n_real + B, Wx).cpu().numpy()
    return {"h": h_all.view(draws, B, W).cpu().numpy(), "xr": x[:, :n_real], "xf": x[:, n_real:],
            "col": col.view(draws, B).cpu().numpy(), "opt": opt.view(draws, B).cpu().numpy(),
            "sc": sc.cpu().numpy(), "metrics": metrics.cpu().numpy()}


def check_sampler_draw(got, k, seed, step, B, E, Dd, n_real, zc=2):
    """Draw k of a launch against the oracle at ``step``."""
    t = sampler_tables(Dd)
    want = rc.sampler(seed, S_STREAM_ID * 16, step, B, E, t["cdf"], S_WIDTHS, n_real, t["row_off"], t["row_cnt"],
                      t["rows"])
    cc = zc + E
    assert np.array_equal(got["col"][k], want["col"]) and np.array_equal(got["opt"][k], want["opt"])
    h = got["h"][k]
    hot = onehot(S_OFF[want["col"]] + want["opt"], S_C)
    assert np.array_equal(h[:, cc:], hot)
    assert np.array_equal(h[:, :zc], np.full((B, zc), 9.0, dtype=np.float32))        # columns before z untouched
    assert np.abs(h[:, zc:cc] - want["z"]).max() <= ADDR_TOL
    assert np.array_equal(got["xf"][k][:, Dd:], hot)
    assert np.array_equal(got["xf"][k][:, :Dd], np.full((B, Dd), 9.0, dtype=np.float32))
    if n_real:
        assert sorted(want["perm"]) == list(range(n_real))
        assert np.array_equal(got["xr"][k][:, Dd:], onehot(S_OFF[want["pcol"]] + want["popt"], S_C))
        assert np.array_equal(got["xr"][k][:, :Dd], t["data"][want["row"]])
    return want


@pytest.mark.parametrize("B,n_real,E,Dd,step,seed", [(37, 21, 7, 13, hc.STEPS[0], 11), (256, 256, 128, 530, hc.STEPS[1], 12),
                                                    (37, 21, 128, 13, hc.STEPS[2], 13), (256, 100, 7, 530, hc.STEPS[0], 14)])
def test_sampler_matches_oracle(B, n_real, E, Dd, step, seed):
    ops = new_ops(seed, step)
    got = run_sampler(ops, B, E, Dd, n_real)
    want = check_sampler_draw(got, 0, ops.seed, step, B, E, Dd, n_real)
    # the launch's bookkeeping: both optimizer step counters bumped, the metrics zeroed, the RNG counter untouched
    assert np.array_equal(got["sc"], np.full((2, 1), 8.0, dtype=np.float32)) and not got["metrics"].any()
    assert int(ops.ctr.item()) == step
    if B == 256:
        # the cases the tables were built for really occur: wide spans past the first CDF chunk, and real rows drawn
        # from the one-row cell and the empty cell
        t = sampler_tables(Dd)
        assert (want["opt"] >= 64).any()
        cnt = t["row_cnt"][want["pcol"], want["popt"]]
        assert (cnt == 1).any() and (cnt == 0).any()


def test_sampler_multi_draw_matches_consecutive_steps():
    B, n_real, E, Dd, step, draws = 37, 21, 7, 13, hc.STEPS[1], 3
    ops = new_ops(21, step)
    got = run_sampler(ops, B, E, Dd, n_real, draws=draws)
    for k in range(draws):
        check_sampler_draw(got, k, ops.seed, step + k, B, E, Dd, n_real)
    # one thread writes every step's optimizer counters from the canonical last entry (7) and zeroes all metrics
    assert np.array_equal(got["sc"], np.array([[8.0, 9.0, 10.0]] * 2, dtype=np.float32))
    assert not got["metrics"].any() and int(ops.ctr.item()) == step


@pytest.mark.parametrize("B,E,zc,step", [(37, 7, 1, hc.STEPS[1]), (256, 128, 0, hc.STEPS[2])])
def test_sampler_bf16_buffer_matches_oracle(B, E, zc, step):
    """Generation into a bf16 activation buffer: only z is written (odd and even placement: single and packed stores)"""
    ops = new_ops(31, step)
    got = run_sampler(ops, B, E, 13, 0, zc=zc, bf16=True)
    t = sampler_tables(13)
    col, opt = rc.cond_draw(ops.seed, S_STREAM_ID * 16, step, np.arange(B), t["cdf"], S_WIDTHS)
    assert np.array_equal(got["col"], col) and np.array_equal(got["opt"], opt)
    z = rc.noise(ops.seed, S_STREAM_ID * 16, step, B, E)
    # the fp32 value (within ADDR_TOL of the oracle) rounded to bf16: half an ulp of 8 significant bits, 2^-8 relative
    assert (np.abs(got["h"][:, zc:zc + E] - z) <= ADDR_TOL + np.abs(z) * 2.0 ** -8).all()
    assert (got["h"][:, :zc] == 9.0).all() and (got["h"][:, zc + E:] == 9.0).all()


# ============================================================================ GEMM dropout
def run_dropout(ops, M, N, K, p, stream_id, tile=None, splitk=None, pair=False):
    """LeakyReLU + dropout GEMM into column-slice views (leading dimension != N); the keep bits as numpy"""
    g = torch.Generator().manual_seed(M + N)
    a, b, bias = (torch.randn(s, generator=g).to(DEV) for s in ((M, K), (N, K), (N,)))
    cbuf, msbuf = torch.zeros(M, N + 16, device=DEV), torch.full((M, N + 16), -1.0, device=DEV)
    c, ms = cbuf[:, 8:8 + N], msbuf[:, 8:8 + N]
    kw = dict(a=a, b=b, c=c, tb=True, bias=bias, epi=EPI_LRELU_DROPOUT, ms=ms, slope=0.2, p_drop=p, stream_id=stream_id,
              tile=tile, splitk=splitk)
    if pair:      # held weight gradient + this GEMM in one launch
        A, X = torch.randn(M, 64, generator=g).to(DEV), torch.randn(M, K, generator=g).to(DEV)
        ops.gemm(A, X, torch.zeros(64, K, device=DEV), ta=True, group=1)
        ops.gemm(**kw, group=2)
    else:
        ops.gemm(**kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(cbuf).all()) and bool((msbuf[:, :8] == -1).all()) and bool((msbuf[:, 8 + N:] == -1).all())
    vals = torch.unique(ms).cpu().numpy()
    keep = 1.0 / (1.0 - p)
    assert all(min(abs(v), abs(v - keep), abs(v - 0.2 * keep)) < 1e-6 for v in vals), vals
    return (ms != 0).cpu().numpy()


def check_dropout(ops, step, M, N, K, p, stream_id=5, **kw):
    got = run_dropout(ops, M, N, K, p, stream_id, **kw)
    want = rc.dropout_keep(ops.seed, stream_id, step, M, N, p)      # the GEMM receives its stream id as it is
    assert np.array_equal(got, want), (int((got != want).sum()), got.size)


@pytest.mark.parametrize("p", [0.5, 0.25])
@pytest.mark.parametrize("tile", [32, 64, 128])
def test_dropout_small_tiles(tile, p):
    step = hc.STEPS[tile // 64]
    check_dropout(new_ops(41, step), step, 37, 61, 150, p, tile=tile)


@pytest.mark.parametrize("p", [0.5, 0.25])
@pytest.mark.parametrize("splitk,inlaunch", [(1, 0), (5, 0), (5, 1), (1, 1)])
def test_dropout_split_k(splitk, inlaunch, p):
    step = hc.STEPS[1]
    ops = new_ops(42, step)
    ops.splitk_inlaunch = bool(inlaunch)
    check_dropout(ops, step, 150, 256, 1300, p, splitk=splitk)


@pytest.mark.parametrize("M,N,K,kw", [(37, 61, 150, {"tile": 32}), (150, 256, 1300, {"splitk": 5}), (150, 256, 1300, {})])
def test_dropout_fp32_ops(M, N, K, kw):
    step = hc.STEPS[2]
    check_dropout(new_ops(43, step, precision="fp32"), step, M, N, K, 0.5, **kw)


def test_dropout_pair_launch():
    step = hc.STEPS[0]
    check_dropout(new_ops(44, step), step, 50, 256, 1300, 0.5, pair=True)


def small_engine(seed=3, **cfg):
    from fed_tgan_amd.models.engine import CTGANEngine, EngineConfig
    tr, X, _, _ = table_spans()
    eng = CTGANEngine(tr.layout, EngineConfig(batch_size=200, **cfg), DEV, backend="hip", seed=seed)
    eng.set_training_data(X)
    return eng, tr, X


@pytest.mark.parametrize("cfg", [{"chain_d1": True}, {"chain_d1": False}, {"dis_dims": (64, 32, 16)}],
                         ids=["chain", "nochain", "three_layers"])
def test_dropout_through_the_engine(cfg):
    """One eager step: the D phase draws every layer's mask over the 3 nP stacked rows, then the G phase's D forward
    redraws rows [0, nP) on its own streams -- both at the same step value."""
    from fed_tgan_amd.models.engine import d_dropout_stream
    eng, _, _ = small_engine(**cfg)
    step = hc.STEPS[1]
    eng.ops.ctr.fill_(step)
    eng.train_steps(1, use_graph=False)
    torch.cuda.synchronize()
    assert int(eng.ops.ctr.item()) == step + 1
    nP, p = eng.nP, eng.cfg.dropout_p
    for i, h in enumerate(eng.ddims):
        got = (eng.ms[i] != 0).cpu().numpy()
        d = rc.dropout_keep(eng.ops.seed, d_dropout_stream(4, i), step, 3 * nP, h, p)
        g = rc.dropout_keep(eng.ops.seed, d_dropout_stream(14, i), step, nP, h, p)
        assert np.array_equal(got[nP:], d[nP:]) and np.array_equal(got[:nP], g), i
    assert [d_dropout_stream(b, i) for b in (4, 14) for i in (0, 1)] == [4, 5, 14, 15]


# ============================================================================ activation, slerp
ACT_MODES = [(0, 0), (1, 1), (2, 1), (2, 2)]      # (act_row_mode, act_rowreg_narrow)


def run_activation(name, mode, seed=hc.ACT_SEED, spans=None, logits=None, step=None, stream_id=hc.ACT_STREAM_ID,
                   slerp_id=hc.SLERP_STREAM_ID):
    """Activation with the fused slerp under one kernel setting -> (fake rows incl. condition columns, real, interp)"""
    if spans is None:
        spans, D, logits, step = hc.act_case(name)
    R, D = logits.shape
    Din, rs = D + hc.ACT_COND, min(hc.ACT_SLERP_ROWS, R)
    ops = new_ops(seed, step)
    fake = torch.zeros(R, Din, device=DEV)
    fake[:, D:] = dev(hc.normal32((R, hc.ACT_COND), 54))
    real = dev(hc.normal32((rs, Din), 53))
    interp = torch.zeros(rs, Din, device=DEV)
    prev = torch.ops.fedtgan.set_tuning("act_row_mode", mode[0])
    prev_n = torch.ops.fedtgan.set_tuning("act_rowreg_narrow", mode[1])
    try:
        ops.activate(dev(logits), fake[:, :D], spans, hc.TAU, stream_id=stream_id, slerp=(real, fake, interp, slerp_id))
        torch.cuda.synchronize()
    finally:
        torch.ops.fedtgan.set_tuning("act_row_mode", prev)
        torch.ops.fedtgan.set_tuning("act_rowreg_narrow", prev_n)
    return ops, fake.cpu().numpy(), real.cpu().numpy(), interp.cpu().numpy()


def check_fused_slerp(ops, step, fake, real, interp, slerp_id=hc.SLERP_STREAM_ID):
    alpha = rc.slerp_alpha(ops.seed, slerp_id * 16, step, len(real))
    want = rc.slerp(real, fake[:len(real)], alpha)       # the kernel's own activation output, the oracle's alpha
    assert np.abs(interp - want).max() <= SLERP_TOL
    return alpha


@pytest.mark.parametrize("mode", ACT_MODES, ids=lambda m: f"mode{m[0]}{m[1]}")
@pytest.mark.parametrize("name", list(hc.ACT_CASES))
def test_activation_matches_oracle(name, mode):
    spans, D, logits, step = hc.act_case(name)
    want, soft = hc.act_oracle(name)
    ops, fake, real, interp = run_activation(name, mode)
    out = fake[:, :D]
    assert np.isfinite(out).all() and np.abs(out - want).max() <= ADDR_TOL
    for s, w, arg, kept in soft:
        assert np.array_equal(out[:, s:s + w].argmax(1)[kept], arg[kept]), (s, w)
    assert np.array_equal(fake[:, D:], hc.normal32((hc.ACT_ROWS, hc.ACT_COND), 54))     # condition columns untouched
    check_fused_slerp(ops, step, fake, real, interp)


@pytest.mark.parametrize("step", hc.STEPS)
def test_standalone_slerp_matches_oracle(step):
    R, W, sid = 75, 600, 3
    ops = new_ops(61, step)
    real, fake = hc.normal32((R, W), 27), hc.normal32((R, W), 28)
    out = torch.zeros(R, W, device=DEV)
    ops.slerp(dev(real), dev(fake), out, stream_id=sid)
    torch.cuda.synchronize()
    want = rc.slerp(real, fake, rc.slerp_alpha(ops.seed, sid * 16, step, R))
    assert np.abs(out.cpu().numpy() - want).max() <= SLERP_TOL


# ============================================================================ generation decode
def decode_tables(cols):
    """Generation tables whose decoded value IS the chosen position: categorical codes 0..w-1, continuous modes
    with mean k and deviation 0 (so the tanh unit drops out)."""
    K = max([w for k, _, w in cols if k == 0] + [1])
    n_cont = sum(1 for k, _, _ in cols if k == 0)
    tc, c = [], 0
    for kind, start, width in cols:
        if kind == 0:
            tc.append((0, start, width, c, None))
            c += 1
        else:
            tc.append((1, start, width, -1, torch.arange(width, dtype=torch.float64, device=DEV)))
    mu = torch.arange(K, dtype=torch.float64).repeat(max(n_cont, 1), 1)
    return {"cols": tc, "mu": mu.to(DEV), "sd": torch.zeros_like(mu).to(DEV)}


def run_decode(ops, cols, logits, mode):
    out = torch.full((logits.shape[0], len(cols)), -7.0, dtype=torch.float64, device=DEV)
    prev = torch.ops.fedtgan.set_tuning("decode_rows", mode)
    try:
        ops.sample_decode(dev(logits), out, decode_tables(cols), stream_id=hc.DEC_STREAM_ID)
        torch.cuda.synchronize()
    finally:
        torch.ops.fedtgan.set_tuning("decode_rows", prev)
    return out.cpu().numpy()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(hc.DEC_CASES))
def test_decode_matches_oracle(name, mode):
    cols, D, logits, step = hc.dec_case(name)
    choice, kept = hc.dec_oracle(name)
    ops = new_ops(hc.DEC_SEED, step)
    out = run_decode(ops, cols, logits, mode)
    assert np.array_equal(out[kept], choice[kept].astype(np.float64))
    assert int(ops.ctr.item()) == step + 1         # the decode bumps the generation counter


# ============================================================================ conditional request
CR_OFF, CR_W, CR_SPAN, CR_STREAM_ID, CR_ROWS = (0, 3), (3, 70), 1, 24, 300


def cond_request_case(nb):
    rng = np.random.default_rng(nb)
    if nb == 1:
        return [10], [2], [5]
    if nb == 5:
        return [3, 0, 5, 2, 7], [3, 0, 1, 0, 2], [4, 0, 2, 1, 69]
    quota = rng.integers(0, 1000, nb) * (rng.random(nb) > 0.2)
    filled = (quota * rng.random(nb) * (rng.random(nb) > 0.3)).astype(np.int64)
    return quota.tolist(), filled.tolist(), rng.permutation(70)[:nb].tolist()


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("nb", [1, 5, 64])
def test_cond_request_matches_oracle(nb, full):
    from cond_helpers import make_request
    quota, filled, bin_opt = cond_request_case(nb)
    if full:
        filled = quota
    step = hc.STEPS[(nb + full) % 3]
    ops = new_ops(71, step)
    m, C = CR_ROWS, sum(CR_W)
    rng = np.random.default_rng(5)
    col0 = rng.integers(0, 2, m)
    opt0 = (rng.random(m) * np.asarray(CR_W)[col0]).astype(np.int64)
    h0 = np.full((m, 4 + C), 0.0, dtype=np.float32)
    h0[:, :4] = 0.5
    h0[np.arange(m), 4 + np.asarray(CR_OFF)[col0] + opt0] = 1.0
    req = make_request(quota, filled, 0, [float(i) for i in range(nb)], span=CR_SPAN, bin_opt=bin_opt, device=DEV)
    cond = {"cond_offset": dev(np.asarray(CR_OFF, dtype=np.int32)), "cond_width": dev(np.asarray(CR_W, dtype=np.int32))}
    col, opt, h = dev(col0, torch.int32), dev(opt0, torch.int32), dev(h0)
    tgt = torch.full((m + 3,), -5, dtype=torch.int32, device=DEV)
    ops.cond_request(req, col, opt, tgt[:m], cond, h=h, c_col0=4, stream_id=CR_STREAM_ID)
    torch.cuda.synchronize()
    want = rc.cond_request(ops.seed, CR_STREAM_ID * 16, step, m, quota, filled)
    assert np.array_equal(tgt[:m].cpu().numpy(), want) and bool((tgt[m:] == -5).all())
    if full:
        assert (want == -1).all()
        wcol, wopt, wh = col0, opt0, h0
    else:
        assert want.min() >= 0 and (np.asarray(quota)[want] > np.asarray(filled)[want]).all()
        wcol, wopt = np.full(m, CR_SPAN), np.asarray(bin_opt)[want]
        wh = h0.copy()
        wh[:, 4:] = onehot(CR_OFF[CR_SPAN] + wopt, C)          # the hot element moved, nothing else
    assert np.array_equal(col.cpu().numpy(), wcol) and np.array_equal(opt.cpu().numpy(), wopt)
    assert np.array_equal(h.cpu().numpy(), wh)
    assert int(ops.ctr.item()) == step


# ============================================================================ top-of-range draws (u01 == 1.0)
# Edge seeds: word x (y) of (stream 16, step 0, counter 0) has its top 24 bits set, so u01 of it is exactly 1.0 and
# the consumer's clamp decides.  Stream id 1 reaches stream 16 in every kernel but the GEMM, which takes 16 itself.
@pytest.mark.parametrize("seed", rc.EDGE_SEEDS_X)
def test_top_of_range_sampler_column(seed):
    B, n_real, E, Dd = 37, 21, 7, 13
    ops = new_ops(seed, 0)
    got = run_sampler(ops, B, E, Dd, n_real)
    assert got["col"][0][0] == len(S_WIDTHS) - 1           # u01 * n_col == n_col, clamped
    assert np.isfinite(got["h"]).all()
    check_sampler_draw(got, 0, ops.seed, 0, B, E, Dd, n_real)


@pytest.mark.parametrize("seed", rc.EDGE_SEEDS_Y)
def test_top_of_range_sampler_option(seed):
    B, n_real, E, Dd = 37, 21, 7, 13
    ops = new_ops(seed, 0)
    got = run_sampler(ops, B, E, Dd, n_real)
    assert got["opt"][0][0] == S_WIDTHS[got["col"][0][0]] - 1      # no cdf entry exceeds 1.0: the last option
    check_sampler_draw(got, 0, ops.seed, 0, B, E, Dd, n_real)


@pytest.mark.parametrize("seed", rc.EDGE_SEEDS_X)
def test_top_of_range_dropout_and_slerp(seed):
    ops = new_ops(seed, 0)
    assert run_dropout(ops, 37, 61, 150, 0.5, rc.EDGE_STREAM)[0, 0]           # 1.0 >= p: kept
    check_dropout(ops, 0, 37, 61, 150, 0.5, stream_id=rc.EDGE_STREAM)
    R, W = 75, 600
    real, fake = hc.normal32((R, W), 27), hc.normal32((R, W), 28)
    out = torch.zeros(R, W, device=DEV)
    ops.slerp(dev(real), dev(fake), out, stream_id=1)
    torch.cuda.synchronize()
    alpha = rc.slerp_alpha(ops.seed, rc.EDGE_STREAM, 0, R)
    assert alpha[0] == np.float32(1.0)
    out = out.cpu().numpy()
    assert np.abs(out[0] - fake[0]).max() <= 1e-5                             # alpha == 1: the fake row
    assert np.abs(out - rc.slerp(real, fake, alpha)).max() <= SLERP_TOL


EDGE_SPANS = [(0, 5, 1), (5, 1, 0), (6, 70, 1), (76, 1, 0), (77, 3, 1)]


@pytest.mark.parametrize("mode", ACT_MODES, ids=lambda m: f"mode{m[0]}{m[1]}")
def test_top_of_range_activation(mode):
    """Element (0, 0) draws the clamped Gumbel value -log(1e-30); every output stays finite"""
    seed, D = rc.EDGE_SEEDS_X[0], 80
    logits = hc.normal32((hc.ACT_ROWS, D), 91, 2.0)
    assert rc.gumbel(rc.activation_words(seed, rc.EDGE_STREAM, 0, 1, 1))[0, 0] == rc.GUMBEL_TOP
    ops, fake, real, interp = run_activation(None, mode, seed=seed, spans=EDGE_SPANS, logits=logits, step=0, stream_id=1,
                                             slerp_id=2)
    want, _ = rc.activate(logits, EDGE_SPANS, hc.TAU, ops.seed, rc.EDGE_STREAM, 0)
    out = fake[:, :D]
    assert np.isfinite(out).all() and np.isfinite(interp).all()
    assert np.abs(out - want).max() <= ADDR_TOL and out[0, 0] >= 1.0 - ADDR_TOL
    check_fused_slerp(ops, 0, fake, real, interp, slerp_id=2)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_top_of_range_decode(mode):
    seed = rc.EDGE_SEEDS_X[1]
    cols, D = hc.DEC_CUSTOM, 84
    for logits in (np.zeros((hc.DEC_ROWS, D), dtype=np.float32), hc.normal32((hc.DEC_ROWS, D), 120, 3.0)):
        ops = new_ops(seed, 0)
        ops_stream = 1
        out = torch.full((hc.DEC_ROWS, len(cols)), -7.0, dtype=torch.float64, device=DEV)
        prev = torch.ops.fedtgan.set_tuning("decode_rows", mode)
        try:
            ops.sample_decode(dev(logits), out, decode_tables(cols), stream_id=ops_stream)
            torch.cuda.synchronize()
        finally:
            torch.ops.fedtgan.set_tuning("decode_rows", prev)
        out = out.cpu().numpy()
        choice, gap = rc.decode_choice(logits, cols, ops.seed, rc.EDGE_STREAM, 0)
        kept = gap >= hc.NEAR_TIE
        assert kept.mean() >= 0.99 and np.isfinite(out).all()
        assert choice[0, 0] == 0 and out[0, 0] == 0.0          # position 0 of row 0 carries the clamped value: it wins
        assert np.array_equal(out[kept], choice[kept].astype(np.float64))


# ============================================================================ distinct streams
class RecordingLib:
    """Forwards every call to the native library and records the integers it was given."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not callable(f):
            return f

        def call(*a, **kw):
            self.calls.append((name, tuple("tensor" if torch.is_tensor(x) else x for x in a)))
            return f(*a, **kw)
        return call


def effective_streams(name, a):
    """The Philox streams a recorded launch draws from (positions: the op signatures in csrc/bindings.cpp)"""
    if name == "gemm":
        return {a[16]} if a[8] == EPI_LRELU_DROPOUT else set()
    if name == "sample":
        return {a[22] + k for k in range(4)}          # condition, permutation key, noise, row pick
    if name == "activate":
        return {a[10]} | ({a[14]} if a[11] is not None else set())
    if name == "slerp":
        return {a[5]}
    if name == "sample_decode":
        return {a[12]}
    if name == "cond_request":
        return {a[18]}
    return set()


def bumps_counter(name, a):
    return name == "rng_bump" or (name in ("adam", "adam_cs") and a[10] is not None)


@pytest.mark.parametrize("gen_dims", [(256, 256), (128,)])
@pytest.mark.parametrize("dis_dims", [(256, 256), (64, 32, 16)])
def test_call_sites_draw_from_distinct_streams(dis_dims, gen_dims):
    """One full training step and one generation pass (plain and conditional): launches that share a step value never
    share a stream, and no two call sites overlap at all (a later step of one reaches the counter value of another)."""
    from fed_tgan_amd.models.conditional import build_request
    from fed_tgan_amd.models.samplers import CondTables
    eng, tr, X = small_engine(dis_dims=dis_dims, gen_dims=gen_dims)
    rec = eng.ops.L = RecordingLib(eng.ops.L)
    eng.train_steps(1, use_graph=False)
    eng.set_generation_tables(CondTables.from_encoded(X, tr.layout), tr)
    eng.generate_decoded(300)
    _, _, _, meta, vocabs, _, _, _ = small_table()
    req = build_request(tr, meta, vocabs, {"protocol_type": "udp"}, 64, DEV)
    eng.generate_decoded_where(64, req, chunk=128, use_graph=False)
    torch.cuda.synchronize()
    sites, epoch, seen = {}, [], set()
    for name, a in rec.calls:
        s = effective_streams(name, a)
        if s:
            seen.add(name)
            for other_name, other in epoch:
                assert not (s & other), f"{name} and {other_name} share streams {s & other} at one step value"
            epoch.append((name, s))
            sites.setdefault((name, tuple(sorted(s))), s)
        if bumps_counter(name, a):
            epoch = []
    assert {"gemm", "sample", "activate", "sample_decode", "cond_request"} <= seen
    keys = list(sites)
    for i, k in enumerate(keys):
        for k2 in keys[i + 1:]:
            assert not (sites[k] & sites[k2]), f"call sites {k} and {k2} share streams"
    n_drop = sum(1 for name, a in rec.calls if name == "gemm" and a[8] == EPI_LRELU_DROPOUT)
    assert n_drop >= 2 * len(dis_dims)
