"""Eager-PyTorch reference implementations of every fused op the engine uses.

Each method here states the math of one fused HIP kernel in ``csrc/kernels`` with plain
PyTorch ops.  It is (a) the CPU execution path (gloo demos, CI without a GPU) and
(b) the numerics oracle the HIP kernels are tested against.  Signatures are shared with
:class:`fed_tgan_amd.ops.hip.HipOps`; outputs are written in place into (possibly
strided, column-sliced) views so that the engine's concat-free buffer layout works on
both paths.

Randomness comes from the global torch generator of the tensor's device (the HIP path
uses counter-based Philox streams instead, so the two paths agree in distribution, not
bitwise).
"""
from __future__ import annotations

import math

import numpy as np
import torch

EPI_NONE = 0
EPI_LRELU_DROPOUT = 1   # out = lrelu(acc + bias, slope) * M, M in {0, 1/(1-p)}; ms = lrelu'(.) * M
EPI_MASK = 2            # out = acc * ms
EPI_RELU = 3


def _code_or_overflow(v: torch.Tensor, K) -> torch.Tensor:
    """v where it lies in [0, K) (a code, still to be truncated), else (NaN included) the overflow bin K; K is a
    number or a tensor that broadcasts against v"""
    K = torch.as_tensor(K, dtype=v.dtype, device=v.device)
    return torch.where((v >= 0) & (v < K), v, K.expand_as(v))


def _balanced_weights(counts: torch.Tensor):
    """(n_valid / (present * count_c) per class and 0 for an absent class, n_valid, classes present), float64"""
    cd, live = counts.to(torch.float64), counts > 0
    nv, present = cd.sum(), live.sum().to(torch.float64)
    return torch.where(live, nv / (present * torch.where(live, cd, torch.ones_like(cd))), torch.zeros_like(cd)), nv, present


class TorchOps:
    adam_counts_steps = True     # eager Adam bumps its step counter (the HIP sampler does it there)
    name = "torch"

    # ------------------------------------------------------------------ GEMM
    def gemm_plan(self, M: int, N: int, K: int):
        return 32, 1

    @staticmethod
    def _bn_partials(v: torch.Tensor, part: torch.Tensor, rpg: int, tile: int):
        """Per row tile and batch: (count, mean, M2) of every column -- the GEMM epilogue's partials."""
        M, N = v.shape
        pv = part.view(-1, 2, 3, N)
        for t in range(-(-M // tile)):
            for b in range(2):
                lo, hi = max(t * tile, rpg if b else 0), min((t + 1) * tile, M if b else rpg)
                if hi <= lo:
                    pv[t, b].zero_()
                    continue
                x = v[lo:hi]
                mu = x.mean(0)
                pv[t, b, 0] = float(hi - lo)
                pv[t, b, 1] = mu
                pv[t, b, 2] = ((x - mu) ** 2).sum(0)

    def gemm(self, a, b, c, ta=False, tb=False, alpha=1.0, beta=0.0, bias=None, epi=EPI_NONE, ms=None,
             slope=0.2, p_drop=0.5, stream_id=0, head=None, group=0, onehot=None, bn_part=None, bn_rpg=0, tile=None,
             splitk=None, **_):
        """c = epi(alpha * op(a) @ op(b) + beta * c + bias [+ onehot]).

        onehot = (W_c [N, C], col [M], opt [M], cond_offset): a holds only the dense input columns and
        the one-hot conditional block adds W_c[:, cond_offset[col[m]] + opt[m]] to row m.
        bn_part (with bn_rpg, tile): also the per-tile BatchNorm partials of the stored output."""
        A = a.t() if ta else a
        B = b.t() if tb else b
        acc = torch.matmul(A, B)
        if alpha != 1.0:
            acc = acc * alpha
        if beta != 0.0:
            acc = acc + beta * c
        if bias is not None:
            acc = acc + bias
        if onehot is not None:
            w_c, col, opt, off = onehot[:4]
            if len(onehot) > 4 and onehot[4]:
                w_c = w_c.t()
            m = acc.shape[0]
            idx = (off.long()[col[:m].long()] + opt[:m].long())
            acc = acc + w_c[:, idx].t()
        if epi == EPI_LRELU_DROPOUT:
            keep = (torch.rand(acc.shape, device=acc.device) >= p_drop).to(acc.dtype) / (1.0 - p_drop)
            s = torch.where(acc > 0, torch.ones_like(acc), torch.full_like(acc, slope))
            ms.copy_(s * keep)
            acc = acc * ms
            if head is not None:      # D head seed: A_{L-1} = coef * v * MS_{L-1}
                coef, v, a_out = head
                a_out.copy_(coef.view(-1, 1) * v.view(1, -1) * ms)
        elif epi == EPI_MASK:
            acc = acc * ms
        elif epi == EPI_RELU:
            acc = torch.relu(acc)
        c.copy_(acc)
        if bn_part is not None:
            self._bn_partials(acc, bn_part, int(bn_rpg), int(tile or 32))

    # ------------------------------------------------------------------ samplers
    def sample_train(self, t, h, z_cols, c_cols, x_fake, x_real, Dd, col_out, opt_out, step_counter=None,
                     metrics=None, zero_metrics=False, stream_id=0):
        """Draw the training conditional batch, noise, permutation and real rows.

        h[:, z_cols] <- N(0,1); h[:, c_cols] <- c1; x_fake[:, Dd:] <- c1; x_real <- [data[row], c1[perm]].
        t: dict of device tables (cdf_log, cond_offset, cond_width, row_offset, row_count, rows, data).
        (step_counter / metrics are bookkeeping of the HIP backend; eager Adam counts its own steps.)
        When x_real covers only the leading rows, those rows are a D-phase batch and the rest a
        G-phase batch (no real rows) drawn in the same call.
        """
        if x_real is not None and x_real.shape[0] < h.shape[0]:
            n = x_real.shape[0]
            self.sample_train(t, h[:n], z_cols, c_cols, x_fake[:n], x_real, Dd, col_out[:n], opt_out[:n])
            self.sample_train(t, h[n:], z_cols, c_cols, x_fake[n:], None, Dd, col_out[n:], opt_out[n:])
            return
        dev = h.device
        B = h.shape[0]
        x_fake_c = x_fake[:, Dd:]
        n_col = t["cond_width"].numel()
        h[:, z_cols[0]:z_cols[1]].normal_()
        c1 = h[:, c_cols[0]:c_cols[1]]
        c1.zero_()
        if n_col == 0:
            if x_real is not None:
                idx = torch.randint(0, t["data"].shape[0], (B,), device=dev)
                x_real.copy_(t["data"][idx])
            return
        col = torch.randint(0, n_col, (B,), device=dev)
        u = torch.rand(B, 1, device=dev, dtype=t["cdf_log"].dtype)
        opt = (t["cdf_log"][col] > u).to(torch.int32).argmax(1)
        opt = torch.minimum(opt, t["cond_width"][col].long() - 1)
        c1.scatter_(1, (t["cond_offset"][col].long() + opt).view(-1, 1), 1.0)
        x_fake_c.copy_(c1)
        col_out.copy_(col.to(col_out.dtype))
        opt_out.copy_(opt.to(opt_out.dtype))
        if x_real is None:
            return
        perm = torch.argsort(torch.rand(B, device=dev))
        cp, op_ = col[perm], opt[perm]
        cnt = t["row_count"][cp, op_]
        pick = torch.floor(torch.rand(B, device=dev, dtype=torch.float64) * cnt.clamp_min(1)).long()
        pick = torch.minimum(pick, (cnt - 1).clamp_min(0))
        row = t["rows"][t["row_offset"][cp, op_] + pick]
        dd = t["data"].shape[1]
        x_real[:, :dd].copy_(t["data"][row])
        x_real[:, dd:].copy_(c1[perm])

    def sample_gen(self, t, h, c_cols, z_cols, col_out=None, opt_out=None, stream_id=0):
        """Generation draw (``sample_zero``): noise + c from the empirical option CDF."""
        dev = h.device
        B = h.shape[0]
        h[:, z_cols[0]:z_cols[1]].normal_()
        c = h[:, c_cols[0]:c_cols[1]]
        c.zero_()
        n_col = t["cond_width"].numel()
        if n_col == 0:
            return
        col = torch.randint(0, n_col, (B,), device=dev)
        u = torch.rand(B, 1, device=dev, dtype=t["cdf_emp"].dtype)
        opt = (t["cdf_emp"][col] > u).to(torch.int32).argmax(1)
        opt = torch.minimum(opt, t["cond_width"][col].long() - 1)
        c.scatter_(1, (t["cond_offset"][col].long() + opt).view(-1, 1), 1.0)
        if col_out is not None:
            col_out[:B].copy_(col.to(col_out.dtype))
            opt_out[:B].copy_(opt.to(opt_out.dtype))

    # ------------------------------------------------------------------ batch norm + relu
    def bn_relu_fwd(self, a, gamma, beta, out, nhat, mean, invstd, rmean, rvar, training=True, momentum=0.1,
                    eps=1e-5, groups=1):
        """groups > 1: the rows are that many consecutive batches, each normalised with its own
        statistics; running statistics are updated batch after batch; mean / invstd [groups, cols]."""
        if groups > 1:
            n = a.shape[0] // groups
            for g in range(groups):
                r = slice(g * n, (g + 1) * n)
                self.bn_relu_fwd(a[r], gamma, beta, out[r], None if nhat is None else nhat[r],
                                 None if mean is None else mean[g], None if invstd is None else invstd[g],
                                 rmean, rvar, training, momentum, eps)
            return
        if training:
            mu = a.mean(0)
            var = a.var(0, unbiased=False)
            n = a.shape[0]
            with torch.no_grad():
                rmean.mul_(1 - momentum).add_(momentum * mu)
                rvar.mul_(1 - momentum).add_(momentum * var * n / max(n - 1, 1))
        else:
            mu, var = rmean, rvar
        istd = torch.rsqrt(var + eps)
        nh = (a - mu) * istd
        if nhat is not None:
            nhat.copy_(nh)
            mean.copy_(mu)
            invstd.copy_(istd)
        out.copy_(torch.relu(nh * gamma + beta))

    def linear_bn_relu(self, x, W, b, gamma, beta, out, abuf, nhat, mean, invstd, rmean, rvar, training=True,
                       momentum=0.1, eps=1e-5, groups=1, onehot=None):
        """out = relu(BN(x @ W^T + b)); training mode uses batch statistics and updates running ones."""
        a = torch.addmm(b, x, W.t())
        if onehot is not None:
            w_c, col, opt, off = onehot[:4]
            if len(onehot) > 4 and onehot[4]:
                w_c = w_c.t()
            a = a + w_c[:, off.long()[col[:a.shape[0]].long()] + opt[:a.shape[0]].long()].t()
        self.bn_relu_fwd(a, gamma, beta, out, nhat, mean, invstd, rmean, rvar, training, momentum, eps, groups)

    def bn_relu_bwd(self, dr, r, nhat, gamma, invstd, da, dgamma, dbeta, dbias=None):
        dy = dr * (r > 0).to(dr.dtype)
        dg = (dy * nhat).sum(0)
        db = dy.sum(0)
        dgamma.copy_(dg)
        dbeta.copy_(db)
        n = dr.shape[0]
        da.copy_(gamma * invstd * (dy - db / n - nhat * (dg / n)))
        if dbias is not None:
            dbias.copy_(da.sum(0))

    # ------------------------------------------------------------------ activations
    def linear_activate(self, x, W, b, logits, out, spans, tau=0.2, stream_id=0, slerp=None, onehot=None, **kw):
        self.gemm(x, W, logits, tb=True, bias=b, onehot=onehot, **kw)
        self.activate(logits, out, spans, tau, stream_id=stream_id)
        if slerp is not None:
            real, fake_full, interp, sid = slerp
            self.slerp(real, fake_full, interp, stream_id=sid)

    def activate(self, logits, out, spans, tau=0.2, stream_id=0):
        """spans: list of (start, width, kind) host tuples (kind 0 tanh, 1 gumbel-softmax)."""
        for s, w, k in spans:
            x = logits[:, s:s + w]
            if k == 0:
                out[:, s:s + w].copy_(torch.tanh(x))
            else:
                u = torch.rand(x.shape, device=x.device, dtype=x.dtype).clamp_(1e-20, 1.0 - 1e-7)
                g = -torch.log(-torch.log(u))
                out[:, s:s + w].copy_(torch.softmax((x + g) / tau, dim=1))

    def act_bwd_ce(self, dact, act, logits, spans, cond_spans, col, opt, dlogits, loss_out, tau=0.2):
        """dlogits = d(act)/d(logits)^T dact + d(cond_loss)/d(logits); loss_out[0] <- cond_loss, or, when
        loss_out has one entry per row, the per-row terms (their sum is cond_loss)."""
        for s, w, k in spans:
            g = dact[:, s:s + w]
            y = act[:, s:s + w]
            if k == 0:
                dlogits[:, s:s + w].copy_(g * (1 - y * y))
            else:
                dlogits[:, s:s + w].copy_(y * (g - (g * y).sum(1, keepdim=True)) / tau)
        B = logits.shape[0]
        per_row = B > 1 and loss_out.numel() == B
        loss = torch.zeros(B if per_row else (), device=logits.device, dtype=logits.dtype)
        colL = col.long()
        optL = opt.long()
        for c, (s, w) in enumerate(cond_spans):
            sel = (colL == c).to(logits.dtype)
            x = logits[:, s:s + w]
            tgt = torch.clamp(optL, max=w - 1).view(-1, 1)
            lse = torch.logsumexp(x, dim=1)
            term = sel * (lse - x.gather(1, tgt).view(-1))
            loss = loss + (term if per_row else term.sum())
            sm = torch.softmax(x, dim=1)
            sm = sm - torch.zeros_like(sm).scatter_(1, tgt, 1.0)
            dlogits[:, s:s + w] += sm * (sel / B).view(-1, 1)
        if per_row:
            loss_out.copy_(loss / B)
        else:
            loss_out[0] = loss / B

    # ------------------------------------------------------------------ gradient penalty pieces
    def slerp(self, real, fake, out, stream_id=0):
        alpha = torch.rand(real.shape[0], 1, device=real.device, dtype=real.dtype)
        rn = real.norm(dim=1, keepdim=True)
        fn = fake.norm(dim=1, keepdim=True)
        cos = ((real / rn) * (fake / fn)).sum(1, keepdim=True).clamp(-1.0, 1.0)
        om = torch.acos(cos)
        so = torch.sin(om)
        lin = so < 1e-6
        wr = torch.where(lin, 1 - alpha, torch.sin((1 - alpha) * om) / torch.where(lin, torch.ones_like(so), so))
        wf = torch.where(lin, alpha, torch.sin(alpha * om) / torch.where(lin, torch.ones_like(so), so))
        out.copy_(wr * real + wf * fake)

    def gp_scale(self, g, out, lam, loss_out):
        n = g.norm(dim=1, keepdim=True)
        P = g.shape[0]
        if P > 1 and loss_out.numel() == P:       # per-pack terms (summed by a later column sum)
            loss_out.copy_(lam * ((n.view(-1) - 1) ** 2) / P)
        else:
            loss_out[0] = lam * ((n - 1) ** 2).mean()
        out.copy_(g * (lam * 2.0 * (n - 1) / (n.clamp_min(1e-30) * P)))

    # ------------------------------------------------------------------ discriminator head
    def d_head(self, d_last, ms_last, v, e, coef, wloss, y, a_last, loss_out):
        """y = d_last @ v + e;  a_last = coef[:,None] * v[None,:] * ms_last;  loss_out[0] = sum(wloss * y)."""
        y.copy_(d_last @ v + e)
        a_last.copy_(coef.view(-1, 1) * v.view(1, -1) * ms_last)
        loss_out[0] = (wloss * y).sum()

    def colsum(self, a, out, beta=0.0):
        if beta == 0.0:
            out.copy_(a.sum(0))
        else:
            out.mul_(beta).add_(a.sum(0))

    def colsum_many(self, srcs, outs, weights=None, dots=None):
        n = len(srcs)
        for a, o, w, d in zip(srcs, outs, weights or [None] * n, dots or [None] * n):
            s = (a * w.view(-1, 1)).sum(0) if w is not None else a.sum(0)
            if o is not None:
                o.copy_(s)
            if d is not None:
                v, e, loss = d[:3]
                u = d[3] if len(d) > 3 and d[3] is not None else w
                su = (a * u.view(-1, 1)).sum(0) if u is not None else a.sum(0)
                usum = u.sum() if u is not None else torch.tensor(float(a.shape[0]), device=a.device)
                loss.add_((su * v.view(-1)).sum() + e.view(-1)[0] * usum)

    # ------------------------------------------------------------------ optimizer
    def adam(self, p, g, m, v, step, lr, b1, b2, eps, wd, last_in_step=False, jobs=None):
        """torch.optim.Adam (L2 weight decay added to the gradient, not AdamW); step is a device counter.
        jobs: colsum_many arguments computed first (the HIP backend folds them into the launch)."""
        if jobs is not None:
            self.colsum_many(*jobs)
        step.add_(1)
        if wd != 0.0:
            g = g + wd * p
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        t = step.to(torch.float64)
        bc1 = 1 - torch.pow(torch.full_like(t, b1), t)
        bc2 = 1 - torch.pow(torch.full_like(t, b2), t)
        denom = (v.sqrt() / torch.sqrt(bc2).to(v.dtype)).add_(eps)
        p.sub_((lr / bc1).to(p.dtype) * (m / denom))

    # ------------------------------------------------------------------ generation decode
    def sample_decode(self, logits, out, tabs, stream_id=0):
        """Fused activate + VGM/categorical decode of generated rows.

        out: [N, n_cols] float64 (continuous columns: value; categorical: label code).
        tabs: dict with host lists 'cols' of (kind, data_start, width, j_cont, i2s_codes).
        """
        N = logits.shape[0]
        for j, (kind, s, w, c, codes) in enumerate(tabs["cols"]):
            if kind == 0:  # continuous: alpha = tanh(logit); mode = argmax(logits + gumbel)
                alpha = torch.tanh(logits[:, s]).clamp(-1, 1)
                x = logits[:, s + 1:s + 1 + w]
                u = torch.rand(x.shape, device=x.device, dtype=x.dtype).clamp_(1e-20, 1.0 - 1e-7)
                k = (x - torch.log(-torch.log(u))).argmax(1)
                mu = tabs["mu"][c][k]
                sd = tabs["sd"][c][k]
                out[:, j] = (alpha.double() * 4 * sd + mu)
            else:
                x = logits[:, s:s + w]
                u = torch.rand(x.shape, device=x.device, dtype=x.dtype).clamp_(1e-20, 1.0 - 1e-7)
                k = (x - torch.log(-torch.log(u))).argmax(1)
                out[:, j] = codes[k].double()
        return out

    # ------------------------------------------------------------------ conditional generation
    COND_MAX_BINS = 64     # the HIP kernels' bin limit; the same request runs on either backend

    def cond_request(self, req, col, opt, tgt, cond, h=None, c_col0=0, stream_id=0):
        """Replace the generation sampler's conditions by a request's (models/conditional.py).

        req: dict of tensors -- drive int32 [2] (cond-span index, output column of the driving column), and per bin
        bin_opt int32, bin_code f64, quota / filled / seg_off int64; fixed_j int32 / fixed_code f64 per other
        requested column; stats int64 [2].  Row b draws bin t with probability remaining_t / sum(remaining)
        (remaining = quota - filled) in integers -- r = floor(u * total), the first bin whose running sum exceeds r,
        so a full bin is never drawn -- and gets col[b] = drive[0], opt[b] = bin_opt[t], tgt[b] = t.  h (fp32
        activations whose one-hot block starts at column c_col0; cond = the span tables cond_offset / cond_width):
        the row's hot element moves with it.  Every quota full: tgt = -1, col / opt / h untouched."""
        m = tgt.shape[0]
        rem = (req["quota"] - req["filled"]).clamp_min(0)
        total = int(rem.sum())
        if total <= 0:
            tgt.fill_(-1)
            return
        u = torch.rand(m, dtype=torch.float64, device=tgt.device)
        r = torch.floor(u * total).long().clamp_(max=total - 1)
        t = torch.searchsorted(torch.cumsum(rem, 0), r, right=True).clamp_(max=rem.numel() - 1)
        span = req["drive"][0].long()
        o = req["bin_opt"].long()[t]
        if h is not None:
            rows = torch.arange(m, device=tgt.device)
            off = cond["cond_offset"].long()
            h[rows, c_col0 + off[col[:m].long()] + opt[:m].long()] = 0.0
            h[rows, c_col0 + off[span] + o] = 1.0
        col[:m] = span.to(col.dtype)
        opt[:m] = o.to(opt.dtype)
        tgt.copy_(t.to(tgt.dtype))

    def cond_partition(self, req, out, tgt, dst, any_value=False):
        """Move the rows of a decoded pass that carry every requested value into their bin's quota segment of dst.

        Row r is kept iff tgt[r] >= 0, out[r, drive[1]] == bin_code[tgt[r]] and out[r, fixed_j[k]] == fixed_code[k]
        for every k (exact float64 compares).  The kept rows of bin t, in row order, continue the bin's segment:
        the i-th of them goes to dst[seg_off[t] + filled[t] + i] while that index stays below seg_off[t] + quota[t];
        the rest are dropped.  Then filled[t] = min(quota[t], filled[t] + kept_t), stats[0] += rows and
        stats[1] += kept rows (dropped ones included).  Nothing else of dst is written.  any_value: no value is
        compared, a row is kept iff 0 <= tgt[r] < bins (the privacy guard without a request: one bin)."""
        m = out.shape[0]
        t = tgt[:m].long()
        nb = req["quota"].numel()
        keep = (t >= 0) & (t < nb)
        tc = t.clamp(0, nb - 1)
        if not any_value:
            keep &= out[:, int(req["drive"][1])] == req["bin_code"][tc]
            for j, code in zip(req["fixed_j"].tolist(), req["fixed_code"].tolist()):
                keep &= out[:, int(j)] == code
        for b in range(nb):
            idx = torch.nonzero(keep & (t == b)).view(-1)
            q, f = int(req["quota"][b]), int(req["filled"][b])
            take = idx[:max(0, q - f)]
            if take.numel():
                s = int(req["seg_off"][b]) + f
                dst[s:s + take.numel()] = out[take]
            req["filled"][b] = min(q, f + int(idx.numel()))
        req["stats"][0] += m
        req["stats"][1] += int(keep.sum())

    PRED_MAX = 16          # predicates per request (kernels/launch.h PRED_MAX)

    def pred_request(self, req, col, opt, tgt, cond, h=None, c_col0=0, stream_id=25):
        """cond_request for a request whose driver is a range or a set (models/conditional.py): one bin, and the
        options of the driving span drawn by weight.

        req: the request dict with drv int32 [2] (cond-span index, output column), drv_opt int32 [M] (the span's
        options with positive weight, in option order), drv_cum float64 [M] (their cumulative normalised weights,
        drv_cum[M - 1] == 1.0) and quota / filled int64 [1].  Row b draws u in (0, 1] and takes k = the number of
        entries with drv_cum[i] <= u, clamped to M - 1; col[b] = drv[0], opt[b] = drv_opt[k], tgt[b] = 0, and the
        hot element of h moves as in cond_request.  quota[0] - filled[0] <= 0: tgt = -1, col / opt / h untouched.
        A driver outside the span tables leaves the rows without a target."""
        m = tgt.shape[0]
        if int(req["quota"][0]) - int(req["filled"][0]) <= 0:
            tgt.fill_(-1)
            return
        cum = req["drv_cum"]
        u = torch.rand(m, dtype=torch.float64, device=tgt.device)
        k = torch.searchsorted(cum, u, right=True).clamp_(max=cum.numel() - 1)
        span = int(req["drv"][0])
        o = req["drv_opt"].long()[k]
        width = cond["cond_width"].long()
        if not 0 <= span < width.numel() or bool(((o < 0) | (o >= width[span])).any()):
            tgt.fill_(-1)
            return
        if h is not None:
            rows = torch.arange(m, device=tgt.device)
            off = cond["cond_offset"].long()
            h[rows, c_col0 + off[col[:m].long()] + opt[:m].long()] = 0.0
            h[rows, c_col0 + off[span] + o] = 1.0
        col[:m] = span
        opt[:m] = o.to(opt.dtype)
        tgt.zero_()

    def pred_mark(self, req, out, tgt):
        """Test the rows of a decoded pass against a request's predicates, after the decode and before any guard
        step and cond_partition.

        req: pred_j / pred_kind int32 [P] (output column; 0 range, 1 set), pred_lo / pred_hi float64 [P],
        pred_lut_off / pred_lut_len int32 [P], pred_lut uint8 (one byte per label code, 1 = allowed), pred_stats
        int64 [2 + PRED_MAX].  A row with tgt[r] < 0 is left alone and not counted.  Any other row is tested in
        request order: a range passes iff lo <= v <= hi (NaN fails), a set iff v == trunc(v), 0 <= v < lut_len and
        pred_lut[lut_off + int(v)] != 0; a predicate whose column or table slice lies outside its buffer fails.  The
        first failing predicate k sets tgt[r] = -1.  pred_stats[0] += rows tested, [1] += rows rejected, [2 + k] +=
        rows whose first failure is predicate k."""
        P = int(req["pred_j"].numel())
        if P > self.PRED_MAX:
            raise ValueError(f"{P} predicates; the limit is {self.PRED_MAX}")
        m = out.shape[0]
        if P == 0 or m == 0:
            return
        t = tgt[:m]
        live = t >= 0
        first = torch.full((m,), -1, dtype=torch.long, device=out.device)
        lut = req["pred_lut"]
        rows = zip(req["pred_j"].tolist(), req["pred_kind"].tolist(), req["pred_lo"].tolist(),
                   req["pred_hi"].tolist(), req["pred_lut_off"].tolist(), req["pred_lut_len"].tolist())
        for k, (j, kind, lo, hi, off, ln) in enumerate(rows):
            if not 0 <= j < out.shape[1]:
                ok = torch.zeros(m, dtype=torch.bool, device=out.device)
            elif kind == 0:
                v = out[:, j]
                ok = (v >= lo) & (v <= hi)
            elif off < 0 or ln < 0 or off + ln > lut.numel():
                ok = torch.zeros(m, dtype=torch.bool, device=out.device)
            else:
                v = out[:, j]
                ok = (v == torch.trunc(v)) & (v >= 0) & (v < ln)
                idx = torch.where(ok, v, torch.zeros_like(v)).long() + off
                ok &= lut[idx.clamp_(0, max(lut.numel() - 1, 0))] != 0 if lut.numel() else False
            first = torch.where(live & (first < 0) & ~ok, torch.full_like(first, k), first)
        rej = first >= 0
        t[rej] = -1
        st = req["pred_stats"]
        st[0] += int(live.sum())
        st[1] += int(rej.sum())
        st[2:2 + P] += torch.bincount(first[rej], minlength=P).to(st.dtype)

    # ------------------------------------------------------------------ completion of partial rows
    KNOWN_MAX_TRIES = 1024     # candidate rows per query and pass (kernels/launch.h KNOWN_MAX_TRIES)

    def _known_tries(self, tries) -> int:
        R = int(tries)
        if not 1 <= R <= self.KNOWN_MAX_TRIES:
            raise ValueError(f"tries must be 1..{self.KNOWN_MAX_TRIES}, got {tries}")
        return R

    def known_request(self, qidx, drv_span, drv_opt, tries, col, opt, cond, h=None, c_col0=0):
        """Replace the generation sampler's conditions by those of the known rows a pass serves (models/known.py).

        qidx int32 [q]: the query of slot s, -1 for an idle slot; slot s owns the rows s * tries .. s * tries + tries
        - 1 of the pass.  drv_span / drv_opt int32 [queries]: the cond-span and option that drive a query, span -1
        for none.  Every row of a slot with i = qidx[s] >= 0 and drv_span[i] >= 0 gets col = drv_span[i], opt =
        drv_opt[i], and the hot element of h moves as in cond_request.  Rows of idle slots and of queries without a
        driver keep what the sampler drew, and so do rows whose driver points outside the span tables.  No random
        numbers are drawn."""
        R = self._known_tries(tries)
        m = int(qidx.numel()) * R
        if m == 0:
            return
        i = qidx.long().repeat_interleave(R)
        nq = int(drv_span.numel())
        live = (i >= 0) & (i < nq)
        ic = i.clamp(0, max(nq - 1, 0))
        span = torch.where(live, drv_span.long()[ic], torch.full_like(i, -1)) if nq else torch.full_like(i, -1)
        o = drv_opt.long()[ic] if nq else torch.zeros_like(i)
        width = cond["cond_width"].long()
        ok = (span >= 0) & (span < width.numel())
        ok &= (o >= 0) & (o < width[span.clamp(0, width.numel() - 1)])
        rows = torch.nonzero(ok).view(-1)
        if rows.numel() == 0:
            return
        span, o = span[rows], o[rows]
        if h is not None:
            off = cond["cond_offset"].long()
            h[rows, c_col0 + off[col[:m].long()[rows]] + opt[:m].long()[rows]] = 0.0
            h[rows, c_col0 + off[span] + o] = 1.0
        col[rows] = span.to(col.dtype)
        opt[rows] = o.to(opt.dtype)

    def known_match(self, known, mask, qidx, tries, cand, kind, scale, state, dst):
        """Judge the candidates of a decoded pass against the known cells of the queries it serves.

        known float64 / mask uint8 [queries, n_cols] (cell (i, j) is known iff mask[i, j] != 0; an unknown cell's
        value is never read), qidx int32 [q], cand float64 [>= q * tries, n_cols], kind int32 [n_cols] (0
        continuous, 1 categorical), scale float64 [n_cols], state: dict of best / dc float64, miss int32, seen / pick
        int64, one entry per query.  For slot s with i = qidx[s] >= 0 and candidate t of its tries rows:
        dc_t = the sum over the known continuous columns, in column order, of ((known - cand) * scale)^2, ms_t = the
        known categorical columns whose codes differ, d2_t = dc_t + ms_t.  t* = the lowest t with the smallest d2
        (a NaN distance never wins).  Iff d2_t* < best[i]: best / dc / miss take t*'s values, pick[i] = seen[i] +
        t*, dst[i, j] = known[i, j] where known, else cand[t*, j].  In every case seen[i] += tries.  Idle slots write
        nothing."""
        R = self._known_tries(tries)
        q = int(qidx.numel())
        if q == 0:
            return
        n_cols = int(known.shape[1])
        slots = torch.nonzero((qidx >= 0) & (qidx < known.shape[0])).view(-1)
        if slots.numel() == 0:
            return
        i = qidx.long()[slots]
        K = known[i]
        M = mask[i] != 0
        C = cand[:q * R].view(q, R, n_cols)[slots]
        acc = torch.zeros(slots.numel(), R, dtype=torch.float64, device=known.device)
        ms = torch.zeros(slots.numel(), R, dtype=torch.int32, device=known.device)
        zero = torch.zeros((), dtype=torch.float64, device=known.device)
        for j, kd in enumerate(kind.tolist()):
            if not bool(M[:, j].any()):
                continue
            if kd == 0:
                d = (K[:, j, None] - C[:, :, j]) * scale[j]
                acc = acc + torch.where(M[:, j, None], d * d, zero)
            else:
                ms = ms + (M[:, j, None] & (C[:, :, j] != K[:, j, None])).to(torch.int32)
        d2 = acc + ms.double()
        d2 = torch.where(torch.isnan(d2), torch.full_like(d2, float("inf")), d2)
        least = d2.min(1).values
        t = torch.arange(R, device=known.device)
        ts = torch.where(d2 == least[:, None], t, torch.full_like(t, R)).min(1).values
        rows = torch.arange(slots.numel(), device=known.device)
        upd = least < state["best"][i]
        iu, ru, tu = i[upd], rows[upd], ts[upd]
        state["best"][iu] = least[upd]
        state["dc"][iu] = acc[ru, tu]
        state["miss"][iu] = ms[ru, tu]
        state["pick"][iu] = state["seen"][iu] + tu
        dst[iu] = torch.where(M[ru], K[ru], C[ru, tu])
        state["seen"][i] += R

    # ------------------------------------------------------------------ similarity evaluator
    SIM_SORT_TILE = 2048   # the HIP sort's tile; no meaning here beyond the shared attribute
    SIM_PLAIN, SIM_NONNEG, SIM_CAT = 0, 1, 2

    def sim_prepare(self, values, kind, slot, vocab, keys, valid, counts):
        """One pass over a decoded table values [n, n_cols] float64 (eval/device.py DeviceSimilarity).

        kind / slot int32 [n_cols]: a continuous column (SIM_PLAIN, or SIM_NONNEG = decoded by
        data/decode.py nonneg_inverse first, where exactly -1 is the CSV's blank field) becomes row slot of keys
        [n_cont, >= n] in the value space of the CSV, with +inf wherever the CSV carries no finite number, and
        valid[slot] counts its finite values; a categorical column (SIM_CAT) counts its codes into counts[slot]
        (int32 [n_cat, width]); codes outside [0, vocab[slot]) are ignored."""
        n = values.shape[0]
        counts.zero_()
        valid.zero_()
        width = counts.shape[1]
        vl = vocab.tolist()
        inf = float("inf")
        for c, (k, s) in enumerate(zip(kind.tolist(), slot.tolist())):
            col = values[:, c]
            if k == self.SIM_CAT:
                ok = (col >= 0) & (col < min(vl[s], width))
                counts[s] += torch.bincount(col[ok].long(), minlength=width)[:width].to(counts.dtype)
                continue
            v = col.clone()
            if k == self.SIM_NONNEG:
                # the CSV's values come from numpy's exp (data/decode.py); on the CPU use the same one
                e = torch.from_numpy(np.exp(v.numpy())) if v.device.type == "cpu" else torch.exp(v)
                v = e - 1.0
                v = torch.where(v < 0, torch.ceil(v), v)
                v = torch.where(v == -1.0, torch.full_like(v, inf), v)
            fin = torch.isfinite(v)
            keys[s, :n] = torch.where(fin, v, torch.full_like(v, inf))
            valid[s] = fin.sum()

    def sim_sort(self, keys, n, tmp=None):
        """keys[:, :n] ascending per row, in place."""
        if n > 0 and keys.shape[0] > 0:
            keys[:, :n] = torch.sort(keys[:, :n], dim=1).values

    @staticmethod
    def sim_w1_part(n_cont: int, n: int) -> int:
        return 1

    def sim_w1(self, real, n_real, fake, n_fake, max_fake, out, part=None):
        """out[c] = W1 between the first n_real[c] values of real[c] and the first n_fake[c] of fake[c] (both
        ascending), after the min-max scaling of the real values (scale 1 for a constant column): the integral of
        |F_real - F_fake| as fed/stats.py wasserstein_1d computes it.  No real or no fake value: NaN."""
        for c, (nr, m) in enumerate(zip(n_real.tolist(), n_fake.tolist())):
            if nr <= 0 or m <= 0:
                out[c] = float("nan")
                continue
            r, f = real[c, :nr], fake[c, :m]
            lo, hi = r[0], r[-1]
            scale = (hi - lo) if bool(hi > lo) else torch.ones_like(lo)
            u, v = (r - lo) / scale, (f - lo) / scale
            allv = torch.sort(torch.cat([u, v])).values
            grid = allv[:-1].contiguous()
            cu = torch.searchsorted(u.contiguous(), grid, right=True).double() / nr
            cv = torch.searchsorted(v.contiguous(), grid, right=True).double() / m
            out[c] = ((cu - cv).abs() * torch.diff(allv)).sum()

    def sim_jsd(self, real_counts, fake_counts, out):
        """out[c] = eval/similarity.py column_jsd from count vectors (int32 [n_cat, width]): frequencies over the
        real categories (real count > 0); a real category with fake count 0 is appended a second time to both
        vectors; other fake counts only enter the fake total; no real category in the fake column: 1."""
        for c in range(real_counts.shape[0]):
            r, f = real_counts[c].double(), fake_counts[c].double()
            isr = real_counts[c] > 0
            rp = r[isr] / r.sum()
            ff = f[isr]
            fv = torch.where(ff > 0, ff / f.sum().clamp_min(1.0), torch.zeros_like(ff))
            miss = ff == 0
            rv = torch.cat([rp, rp[miss]])
            fv = torch.cat([fv, torch.zeros_like(rp[miss])])
            if float(fv.sum()) == 0.0:
                out[c] = 1.0
                continue
            p, q = rv / rv.sum(), fv / fv.sum()
            mid = 0.5 * (p + q)
            kl = lambda a: (a[a > 0] * torch.log(a[a > 0] / mid[a > 0])).sum()   # noqa: E731
            js = 0.5 * (kl(p) + kl(q)) / math.log(2.0)
            out[c] = torch.sqrt(js.clamp_min(0.0))

    def sim_mean(self, scores, n_cat, n_cont):
        """scores = [avg_jsd, avg_wd, jsd x n_cat, wd x n_cont]: the first two from the rest (NaN: no such column)."""
        scores[0] = scores[2:2 + n_cat].mean() if n_cat else float("nan")
        scores[1] = scores[2 + n_cat:2 + n_cat + n_cont].mean() if n_cont else float("nan")

    # ------------------------------------------------------------------ privacy evaluator
    NN_CONT, NN_CAT = 0, 1
    NN_QUERY_TILE, NN_REF_TILE, NN_CHUNK_ROWS = 256, 16, 2048   # the HIP kernels' tiles; shared attributes only
    NN_PAIRS = 1 << 24                                           # d2 entries nn_top2 holds at a time

    @staticmethod
    def nn_chunks(nr: int) -> int:
        return 1

    @staticmethod
    def nn_scratch(nq: int, nr: int) -> int:
        return 1

    @staticmethod
    def nn_stats_part(n: int) -> int:
        return 1

    def nn_pack(self, values, kind, slot, lo, scale, cont, cat):
        """One pass over a decoded table values [n, n_cols] float64 (eval/privacy.py DevicePrivacy).

        kind / slot int32 [n_cols]: a continuous column (NN_CONT) becomes column slot of cont [>= n, n_cont] as
        (v - lo[slot]) * scale[slot], one subtraction and one product in float64; a categorical column (NN_CAT)
        becomes column slot of cat [>= n, n_cat] int32, its code truncated to an integer (a value outside
        [0, 2^31 - 1), or NaN: -1, which equals no code)."""
        n = values.shape[0]
        for c, (k, s) in enumerate(zip(kind.tolist(), slot.tolist())):
            v = values[:, c]
            if k == self.NN_CAT:
                ok = (v >= 0) & (v < 2147483647.0)
                cat[:n, s] = torch.where(ok, v, torch.full_like(v, -1.0)).to(cat.dtype)
            else:
                cont[:n, s] = (v - lo[s]) * scale[s]

    def nn_top2(self, q_cont, q_cat, r_cont, r_cat, exclude_self, d1, d2, i1, scratch=None):
        """Per query row i the two smallest squared distances d1[i] <= d2[i] to the reference rows, counted with
        multiplicity, and i1[i] (int32) the lowest index of a reference row at distance d1[i].

        d2(q, r) = sum over the continuous columns, in column order, of (q_c - r_c)^2 plus the number of
        categorical columns whose codes differ, in float64 from direct differences.  exclude_self: reference row
        i is no candidate of query i (a table against itself).  Fewer than two candidates: d2 = +inf; none:
        d1 = +inf, i1 = -1.  Works on blocks of queries, so the full distance matrix never exists."""
        nq, nr = q_cont.shape[0], r_cont.shape[0]
        dev = q_cont.device
        inf = float("inf")
        step = max(1, self.NN_PAIRS // max(nr, 1))
        cols = torch.arange(nr, device=dev)
        for q0 in range(0, nq, step):
            q1 = min(nq, q0 + step)
            dist = torch.zeros(q1 - q0, nr, dtype=torch.float64, device=dev)
            for c in range(q_cont.shape[1]):
                diff = q_cont[q0:q1, c, None] - r_cont[None, :, c]
                dist += diff * diff
            if q_cat.shape[1]:
                miss = torch.zeros(q1 - q0, nr, dtype=torch.int32, device=dev)
                for c in range(q_cat.shape[1]):
                    miss += (q_cat[q0:q1, c, None] != r_cat[None, :, c]).to(torch.int32)
                dist += miss.to(torch.float64)
            rows = torch.arange(q1 - q0, device=dev)
            if exclude_self:
                own = rows + q0
                ok = own < nr
                dist[rows[ok], own[ok]] = inf
            best = dist.min(dim=1).values
            first = torch.where(dist == best[:, None], cols[None, :], nr).min(dim=1).values     # lowest index of a tie
            none = torch.isinf(best)
            first = torch.where(none, torch.zeros_like(first), first)
            dist[rows, first] = inf
            d1[q0:q1] = best
            d2[q0:q1] = dist.min(dim=1).values
            i1[q0:q1] = torch.where(none, torch.full_like(first, -1), first).to(i1.dtype)

    def nn_within(self, q_cont, q_cat, r_cont, r_cat, t2, near, scratch=None):
        """The privacy guard's radius test: near[i] (int32) = the lowest index of a reference row r with
        d2(q_i, r) <= t2, or -1 where there is none.

        d2 is nn_top2's: the continuous squared differences in column order plus the number of differing categorical
        codes, in float64.  t2: a one-element float64 tensor on the queries' device (the squared radius; <= is
        inclusive, so t2 = 0 flags exact copies and t2 = +inf every row whose distances are not NaN, with near = 0).
        A distance that is NaN (a NaN query value, inf - inf) is within no radius.  Works on blocks of queries."""
        nq, nr = q_cont.shape[0], r_cont.shape[0]
        dev = q_cont.device
        step = max(1, self.NN_PAIRS // max(nr, 1))
        cols = torch.arange(nr, device=dev)
        for q0 in range(0, nq, step):
            q1 = min(nq, q0 + step)
            dist = torch.zeros(q1 - q0, nr, dtype=torch.float64, device=dev)
            for c in range(q_cont.shape[1]):
                diff = q_cont[q0:q1, c, None] - r_cont[None, :, c]
                dist += diff * diff
            if q_cat.shape[1]:
                miss = torch.zeros(q1 - q0, nr, dtype=torch.int32, device=dev)
                for c in range(q_cat.shape[1]):
                    miss += (q_cat[q0:q1, c, None] != r_cat[None, :, c]).to(torch.int32)
                dist += miss.to(torch.float64)
            first = torch.where(dist <= t2.reshape(()), cols[None, :], nr).min(dim=1).values
            near[q0:q1] = torch.where(first < nr, first, torch.full_like(first, -1)).to(near.dtype)

    def guard_mark(self, near, tgt, stats):
        """tgt[i] = -1 (no row of a conditional pass with that target is kept) wherever near[i] >= 0, for the
        tgt.numel() rows of a pass; stats (int64 [2]) += [rows tested, rows rejected]."""
        m = tgt.shape[0]
        rej = near[:m] >= 0
        tgt[rej] = -1
        stats[0] += m
        stats[1] += int(rej.sum())

    NN_MAX_SHARDS = 64                                           # kernels/launch.h: shards one merge folds

    def nn_merge_shards(self, parts, offsets, d1, d2, i1, owner, by_client):
        """The nearest-neighbour answers of K shards folded into the answer over their union (eval/fed_privacy.py).

        parts float64 [K, n, 3]: shard k's nn_top2 result per query row as (d1, d2, i1 as a float64; -1: no
        candidate); offsets int64 [K]: the exclusive prefix sums of the shard row counts.  The shards are folded in
        order with strict <, a shard's d2 competing with the others' d1, so d1 <= d2 are the two smallest distances
        over the union with multiplicity and i1 (int32) = offsets[k] + local is the lowest global index at distance
        d1; owner (int32) = that k, or -1 where no shard has a candidate (d1 = +inf, i1 = -1).  by_client int64
        [2, K] is overwritten: row 0 = query rows whose nearest record shard k holds, row 1 = query rows of which
        shard k holds an exact copy (its d1 == 0)."""
        K, n = int(parts.shape[0]), int(parts.shape[1])
        if K < 1 or K > self.NN_MAX_SHARDS:
            raise ValueError(f"nn_merge_shards: 1..{self.NN_MAX_SHARDS} shards, got {K}")
        dev = parts.device
        inf = float("inf")
        a1 = torch.full((n,), inf, dtype=torch.float64, device=dev)
        a2 = torch.full((n,), inf, dtype=torch.float64, device=dev)
        ai = torch.full((n,), -1, dtype=torch.int64, device=dev)
        ao = torch.full((n,), -1, dtype=torch.int64, device=dev)
        by_client.zero_()
        for k in range(K):
            b1, b2 = parts[k, :, 0], parts[k, :, 1]
            local = parts[k, :, 2].to(torch.int64)
            win = (b1 < a1) & (local >= 0)
            second = ~win & (b1 < a2)
            a2 = torch.where(win, torch.where(b2 < a1, b2, a1), torch.where(second, b1, a2))
            a1 = torch.where(win, b1, a1)
            ai = torch.where(win, offsets[k] + local, ai)
            ao = torch.where(win, torch.full_like(ao, k), ao)
            by_client[1, k] = (b1 == 0).sum()
        for k in range(K):
            by_client[0, k] = (ao == k).sum()
        d1[:n] = a1
        d2[:n] = a2
        i1[:n] = ai.to(i1.dtype)
        owner[:n] = ao.to(owner.dtype)

    def nn_within_merge_shards(self, near, offsets, near_out, owner):
        """The radius answers of K shards folded: near int32 [K, n] (shard k's lowest local hit or -1), offsets int64
        [K] -> near_out int32 [n] = offsets[k] + near[k] of the first shard with a hit (the lowest global index), or
        -1; owner int32 [n] = that k or -1."""
        K, n = int(near.shape[0]), int(near.shape[1])
        if K < 1 or K > self.NN_MAX_SHARDS:
            raise ValueError(f"nn_within_merge_shards: 1..{self.NN_MAX_SHARDS} shards, got {K}")
        hit = torch.full((n,), -1, dtype=torch.int64, device=near.device)
        own = torch.full((n,), -1, dtype=torch.int64, device=near.device)
        for k in range(K):
            take = (own < 0) & (near[k] >= 0)
            hit = torch.where(take, offsets[k] + near[k].to(torch.int64), hit)
            own = torch.where(take, torch.full_like(own, k), own)
        near_out[:n] = hit.to(near_out.dtype)
        owner[:n] = own.to(owner.dtype)

    def nn_stats(self, d1, d2, n, keys, tmp, part, out):
        """Table scores of rows [0, n): keys [2, >= n] receives DCR = sqrt(d1) and NNDR = sqrt(d1 / d2) (1 where
        d2 == 0, 0 where d2 = +inf), each row ascending; out[0], out[1] = their 5th percentiles with numpy's linear
        interpolation at position 0.05 (n - 1); out[2] = the smallest DCR; out[3] = the share of rows with d1 == 0."""
        a, b = d1[:n], d2[:n]
        safe = torch.where((b == 0) | torch.isinf(b), torch.ones_like(b), b)
        ratio = torch.sqrt(torch.where(torch.isinf(b), torch.zeros_like(a), a) / safe)
        ratio = torch.where(b == 0, torch.ones_like(ratio), ratio)
        keys[0, :n] = torch.sort(torch.sqrt(a)).values
        keys[1, :n] = torch.sort(ratio).values
        pos = (n - 1) * 0.05
        lo = min(max(int(math.floor(pos)), 0), n - 1)
        hi = min(lo + 1, n - 1)
        t = pos - lo
        for row in range(2):
            u, v = keys[row, lo], keys[row, hi]
            if t == 0.0 or bool(u == v):
                out[row] = u
            else:       # numpy's _lerp
                out[row] = v - (v - u) * (1.0 - t) if t >= 0.5 else u + (v - u) * t
        out[2] = keys[0, 0]
        out[3] = (a == 0).sum().to(torch.float64) / n

    # ------------------------------------------------------------------ fidelity evaluator
    FID_MAX_K = 8                                                # kernels/launch.h: the largest k

    @staticmethod
    def nn_topk_scratch(nq: int, nr: int, k: int) -> int:
        return 1

    @staticmethod
    def nn_ball_scratch(nq: int, nr: int) -> int:
        return 1

    def _nn_blocks(self, q_cont, q_cat, r_cont, r_cat):
        """(q0, q1, the [q1 - q0, nr] float64 block of d2) over blocks of queries, nn_top2's d2 and block size"""
        nq, nr = q_cont.shape[0], r_cont.shape[0]
        dev = q_cont.device
        step = max(1, self.NN_PAIRS // max(nr, 1))
        for q0 in range(0, nq, step):
            q1 = min(nq, q0 + step)
            dist = torch.zeros(q1 - q0, nr, dtype=torch.float64, device=dev)
            for c in range(q_cont.shape[1]):
                diff = q_cont[q0:q1, c, None] - r_cont[None, :, c]
                dist += diff * diff
            if q_cat.shape[1]:
                miss = torch.zeros(q1 - q0, nr, dtype=torch.int32, device=dev)
                for c in range(q_cat.shape[1]):
                    miss += (q_cat[q0:q1, c, None] != r_cat[None, :, c]).to(torch.int32)
                dist += miss.to(torch.float64)
            yield q0, q1, dist

    def nn_topk(self, q_cont, q_cat, r_cont, r_cat, exclude_self, k, out, scratch=None):
        """out[i] = the k-th smallest squared distance (nn_top2's d2) of query row i to the reference rows, counted
        with multiplicity; +inf where there are fewer than k candidates.  1 <= k <= FID_MAX_K.  exclude_self:
        reference row i is no candidate of query i.  A NaN distance is no candidate.  Works on blocks of queries."""
        k = int(k)
        if not 1 <= k <= self.FID_MAX_K:
            raise ValueError(f"nn_topk: k is 1..{self.FID_MAX_K}, got {k}")
        nr = r_cont.shape[0]
        inf = float("inf")
        for q0, q1, dist in self._nn_blocks(q_cont, q_cat, r_cont, r_cat):
            if exclude_self:
                rows = torch.arange(q1 - q0, device=dist.device)
                own = rows + q0
                ok = own < nr
                dist[rows[ok], own[ok]] = inf
            dist = torch.where(torch.isnan(dist), torch.full_like(dist, inf), dist)
            if nr < k:
                out[q0:q1] = inf
            else:
                out[q0:q1] = torch.topk(dist, k, dim=1, largest=False).values[:, k - 1]

    def nn_ball(self, q_cont, q_cat, r_cont, r_cat, r_rad2, cnt, dmin, scratch=None):
        """cnt[i] (int32) = the number of reference rows r with d2(q_i, r) <= r_rad2[r] (inclusive; a radius of +inf
        holds every distance that is no NaN), dmin[i] = the smallest d2(q_i, r) (+inf where every distance is NaN).
        d2 is nn_top2's.  Works on blocks of queries."""
        nr = r_cont.shape[0]
        rad = r_rad2[:nr]
        for q0, q1, dist in self._nn_blocks(q_cont, q_cat, r_cont, r_cat):
            cnt[q0:q1] = (dist <= rad[None, :]).sum(dim=1).to(cnt.dtype)
            dmin[q0:q1] = torch.where(torch.isnan(dist), torch.full_like(dist, float("inf")), dist).min(dim=1).values

    def prdc_reduce(self, cnt_a, cnt_b, dmin_b, rr, n, m, k, scores):
        """scores[0:4] = precision, recall, density, coverage (eval/fidelity.py) of n generated rows (cnt_a int32
        [>= n]) against m real rows (cnt_b int32, dmin_b / rr float64, [>= m]): integer sums in int64, one float64
        division each (by a tensor: torch may turn a division by a Python number into a product with its reciprocal,
        which rounds twice)."""
        n, m, k = int(n), int(m), int(k)
        a, b = cnt_a[:n].to(torch.int64), cnt_b[:m]
        f64 = torch.float64
        den = lambda v: torch.full((), float(v), dtype=f64, device=scores.device)      # noqa: E731
        scores[0] = (a > 0).sum().to(f64) / den(n)
        scores[1] = (b > 0).sum().to(f64) / den(m)
        scores[2] = a.sum().to(f64) / den(k * n)
        scores[3] = (dmin_b[:m] <= rr[:m]).sum().to(f64) / den(m)

    # ------------------------------------------------------------------ correlation evaluator
    CORR_CONT, CORR_CAT = 0, 1
    CORR_CHUNK, CORR_LDS_BINS = 1024, 16384     # the HIP kernels' row chunk and LDS table limit; shared attributes only
    CORR_CELLS = 1 << 24                         # table cells corr_counts holds at a time

    @staticmethod
    def corr_part(n_max: int, W: int, n_cont: int) -> int:
        return 1

    @staticmethod
    def corr_groups(n: int, W: int, n_cont: int) -> int:
        return 1

    def corr_pack(self, values, kind, slot, card, cont, cat_t, mean, part=None):
        """One pass over a decoded table values [n, n_cols] float64 (eval/correlation.py DeviceCorrelation).

        kind / slot int32 [n_cols]: a continuous column (CORR_CONT) becomes column slot of cont [>= n, n_cont]
        unchanged and mean[slot] = its sum / n; a categorical column (CORR_CAT) becomes row slot of cat_t
        [n_cat, >= n] int32: its code truncated to an integer when it lies in [0, card[slot]), else (NaN included)
        the overflow bin card[slot]."""
        n = values.shape[0]
        dev = values.device
        kl, sl = kind.tolist(), slot.tolist()
        cc = [c for c, k in enumerate(kl) if k == self.CORR_CONT]
        kc = [c for c, k in enumerate(kl) if k == self.CORR_CAT]
        if cc:
            cs = torch.tensor([sl[c] for c in cc], dtype=torch.long, device=dev)
            cont[:n, cs] = values[:, torch.tensor(cc, dtype=torch.long, device=dev)]
            mean.copy_(cont[:n].sum(dim=0) / n)
        if kc:
            ks = torch.tensor([sl[c] for c in kc], dtype=torch.long, device=dev)
            v = values[:, torch.tensor(kc, dtype=torch.long, device=dev)]
            cat_t[ks, :n] = _code_or_overflow(v, card[ks][None, :]).t().to(cat_t.dtype)

    def corr_moments(self, cont, cat_t, n, mean, card, offs, G, part=None):
        """G [W, n_cont] = F^T Xc in float64 with Xc = cont[:n] - mean and F = [Xc | one-hot(codes)]: rows
        [0, n_cont) hold the centred cross sums, row n_cont + offs[c] + k the sum of Xc over the rows whose code in
        categorical column c is k (k <= card[c]; codes are clamped into that range).  The one-hot is never built: the
        rows of Xc are added into the bins their codes select, one column at a time.  On a GPU index_add_ is a
        floating-point atomic scatter, so two runs may differ in the last bits there: the bit-identical guarantee of
        the contract holds for HipOps, and for these ops on the CPU only."""
        nc = cont.shape[1]
        if nc == 0:
            return
        xc = cont[:n] - mean[None, :]
        G[:nc] = xc.t() @ xc
        for c, (K, o) in enumerate(zip(card.tolist(), offs.tolist())):
            block = torch.zeros(K + 1, nc, dtype=G.dtype, device=G.device)
            block.index_add_(0, cat_t[c, :n].long().clamp(0, K), xc)
            G[nc + o:nc + o + K + 1] = block

    def corr_counts(self, cat_t, n, pairs, poff, counts, lds_bins=None):
        """counts (int32, flat) = the contingency tables the pair list asks for.  pairs int32 [P, 4] = (column a,
        column b or -1 for the margin of a, bins of a, bins of b); table p starts at poff[p] (int64 [P + 1]) and is
        row-major [bins of a][bins of b].  Codes are clamped into their bins.  Works on blocks of pairs that share
        column a, so only CORR_CELLS row-table cells exist at a time."""
        counts.zero_()
        pl, po = pairs.tolist(), poff.tolist()
        dev = cat_t.device
        block = max(1, self.CORR_CELLS // max(n, 1))
        i, P = 0, len(pl)
        while i < P:
            a, ka = pl[i][0], pl[i][2]
            j = i
            while j < P and j - i < block and pl[j][0] == a and pl[j][2] == ka:
                j += 1
            ca = cat_t[a, :n].long().clamp(0, ka - 1)
            b = torch.tensor([q[1] for q in pl[i:j]], dtype=torch.long, device=dev)
            kb = torch.tensor([q[3] for q in pl[i:j]], dtype=torch.long, device=dev)
            base = torch.tensor([o - po[i] for o in po[i:j]], dtype=torch.long, device=dev)
            cb = cat_t[b.clamp_min(0), :n].long().clamp_min(0)
            cb = torch.minimum(cb, (kb - 1)[:, None])
            cb = torch.where((b >= 0)[:, None], cb, torch.zeros_like(cb))
            flat = base[:, None] + ca[None, :] * kb[:, None] + cb
            counts[po[i]:po[j]] += torch.bincount(flat.flatten(), minlength=po[j] - po[i]).to(counts.dtype)
            i = j

    def corr_matrix(self, G, counts, poff, kind, slot, card, offs, n, A):
        """A [C, C] float64, the association matrix of the contract (eval/correlation.py): Pearson r from G's top
        block, the correlation ratio from the per-category sums and the margins, Theil's U(i|j) from the tables.
        The tables of poff: the n_cat margins first, then the pairs a < b in row-major order."""
        dev = A.device
        kl, sl = kind.tolist(), slot.tolist()
        cl, ol, po = card.tolist(), offs.tolist(), poff.tolist()
        n_cat = len(cl)
        nc = A.shape[0] - n_cat
        col_cont = [0] * nc
        col_cat = [0] * n_cat
        for c, (k, s) in enumerate(zip(kl, sl)):
            (col_cat if k == self.CORR_CAT else col_cont)[s] = c
        A.zero_()
        A.fill_diagonal_(1.0)
        nf = float(n)
        if nc:
            ci = torch.tensor(col_cont, dtype=torch.long, device=dev)
            d = torch.diagonal(G[:nc]).clone()
            den = torch.sqrt(d[:, None] * d[None, :])
            ok = (d[:, None] > 0) & (d[None, :] > 0)
            r = torch.where(ok, G[:nc] / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(den))
            r = r.clamp(-1.0, 1.0)
            r.fill_diagonal_(1.0)
            A[ci[:, None], ci[None, :]] = r
        margins, entropy = [], []
        for c in range(n_cat):
            m = counts[po[c]:po[c] + cl[c] + 1].to(torch.float64)
            p = m / nf
            h = -(torch.where(m > 0, p * torch.log(torch.where(m > 0, p, torch.ones_like(p))), torch.zeros_like(p))).sum()
            margins.append(m)
            entropy.append(h)
            if nc:
                S = G[nc + ol[c]:nc + ol[c] + cl[c] + 1]
                mm = torch.where(m > 0, m, torch.ones_like(m))[:, None]
                val = torch.where((m > 0)[:, None], S * S / mm, torch.zeros_like(S)).sum(dim=0)
                eta = torch.where(d > 0, torch.sqrt(val / torch.where(d > 0, d, torch.ones_like(d))),
                                  torch.zeros_like(d)).clamp(0.0, 1.0)
                A[col_cat[c], ci] = eta
                A[ci, col_cat[c]] = eta
        one = torch.ones((), dtype=torch.float64, device=dev)
        p = n_cat
        for a in range(n_cat):
            for b in range(a + 1, n_cat):
                ka, kb = cl[a] + 1, cl[b] + 1
                T = counts[po[p]:po[p] + ka * kb].view(ka, kb).to(torch.float64)
                p += 1
                pos = T > 0
                Ts = torch.where(pos, T, torch.ones_like(T))
                zero = torch.zeros_like(T)
                h_ab = torch.where(pos, (T / nf) * torch.log(margins[b][None, :] / Ts), zero).sum()   # H(a | b)
                h_ba = torch.where(pos, (T / nf) * torch.log(margins[a][:, None] / Ts), zero).sum()   # H(b | a)
                ha, hb = entropy[a], entropy[b]
                A[col_cat[a], col_cat[b]] = torch.where(ha > 0, ((ha - h_ab) / torch.where(ha > 0, ha, one))
                                                        .clamp(0.0, 1.0), one)
                A[col_cat[b], col_cat[a]] = torch.where(hb > 0, ((hb - h_ba) / torch.where(hb > 0, hb, one))
                                                        .clamp(0.0, 1.0), one)

    def corr_diff(self, A, B, out):
        """out[0] = ||A - B||_F; out[1] = the mean and out[2] = the maximum of |A - B| over the off-diagonal entries
        (both 0 for a 1 x 1 matrix)."""
        C = A.shape[0]
        d = (A - B).abs()
        out[0] = torch.sqrt((d * d).sum())
        off = d.clone()
        off.fill_diagonal_(0.0)
        out[1] = off.sum() / (C * (C - 1)) if C > 1 else 0.0
        out[2] = off.max() if C > 1 else 0.0

    # ------------------------------------------------------------------ ML-utility evaluator
    UTIL_CONT, UTIL_CAT, UTIL_TARGET = 0, 1, 2
    UTIL_MAX_FEATURES, UTIL_MAX_CLASSES, UTIL_CHUNK = 1024, 64, 128    # the HIP kernels' limits; shared attributes only

    @staticmethod
    def util_part(n_max: int, D: int, K: int) -> int:
        return 1

    @staticmethod
    def util_groups(n: int, cells: int) -> int:
        return 1

    def util_pack(self, values, kind, slot, mean, sd, tab):
        """One pass over a decoded table values [n, n_cols] float64 into the packed table ``tab``
        (eval/utility_device.py UtilityTable).  kind / slot int32 [n_cols]: a continuous column (UTIL_CONT) becomes
        column slot of tab.cont as (v - mean[slot]) / sd[slot]; a categorical feature (UTIL_CAT) row slot of tab.cat_t,
        its code when it lies in [0, card[slot]), else the overflow bin card[slot]; the target (UTIL_TARGET) tab.y, its
        code or K.  tab.counts [K] = rows per class, tab.s = n_valid / (present * count[y]) per row (0 where y == K),
        tab.info = [n_valid, classes present, S = sum_c count_c w_c (1 when that is 0), 0]."""
        n, K, dev = values.shape[0], tab.K, values.device
        kl, sl = kind.tolist(), slot.tolist()
        cc = [c for c, k in enumerate(kl) if k == self.UTIL_CONT]
        kc = [c for c, k in enumerate(kl) if k == self.UTIL_CAT]
        tc = [c for c, k in enumerate(kl) if k == self.UTIL_TARGET]
        if cc:
            cs = torch.tensor([sl[c] for c in cc], dtype=torch.long, device=dev)
            v = values[:, torch.tensor(cc, dtype=torch.long, device=dev)]
            tab.cont[:n, cs] = (v - mean[cs][None, :]) / sd[cs][None, :]
        if kc:
            ks = torch.tensor([sl[c] for c in kc], dtype=torch.long, device=dev)
            v = values[:, torch.tensor(kc, dtype=torch.long, device=dev)]
            tab.cat_t[ks, :n] = _code_or_overflow(v, tab.card[ks][None, :]).t().to(tab.cat_t.dtype)
        y = _code_or_overflow(values[:, tc[0]], K).long()
        tab.y[:n] = y.to(tab.y.dtype)
        counts = torch.bincount(y, minlength=K + 1)[:K]
        tab.counts.copy_(counts.to(tab.counts.dtype))
        cw, nv, present = _balanced_weights(counts)
        S = (counts.to(torch.float64) * cw).sum()
        tab.info[0], tab.info[1], tab.info[3] = nv, present, 0.0
        tab.info[2] = torch.where(S > 0, S, torch.ones_like(S))
        tab.s[:n] = torch.cat([cw, cw.new_zeros(1)])[y]

    @staticmethod
    def _util_codes(tab, n):
        return [tab.cat_t[c, :n].long().clamp(0, K) for c, K in enumerate(tab.card.tolist())]

    def util_gram(self, tab, n, M, part=None):
        """M [D, D] = (F^T diag(s) F / 2 + diag(reg)) / S with F = [cont | one-hot(codes) | 1], reg = 1 but for the
        last (intercept) row's 0.  The one-hot blocks are never built: a block of the product is the weighted
        contingency table of two columns, or the rows of s X added into the bins a column's codes select."""
        D, nc = tab.D, tab.cont.shape[1]
        X, s = tab.cont[:n], tab.s[:n]
        G = torch.zeros(D, D, dtype=torch.float64, device=M.device)
        sX = X * s[:, None]
        G[:nc, :nc] = X.t() @ sX
        G[D - 1, D - 1] = s.sum()
        G[:nc, D - 1] = G[D - 1, :nc] = sX.sum(dim=0)
        codes, cl, ol = self._util_codes(tab, n), tab.card.tolist(), tab.offs.tolist()
        for a, ca in enumerate(codes):
            ia, ka = nc + ol[a], cl[a] + 1
            blk = torch.zeros(ka, nc, dtype=torch.float64, device=M.device).index_add_(0, ca, sX)
            G[ia:ia + ka, :nc] = blk
            G[:nc, ia:ia + ka] = blk.t()
            G[ia:ia + ka, D - 1] = G[D - 1, ia:ia + ka] = torch.bincount(ca, weights=s, minlength=ka)
            for b in range(a, len(codes)):
                ib, kb = nc + ol[b], cl[b] + 1
                T = torch.bincount(ca * kb + codes[b], weights=s, minlength=ka * kb).view(ka, kb)
                G[ia:ia + ka, ib:ib + kb] = T
                G[ib:ib + kb, ia:ia + ka] = T.t()
        reg = torch.ones(D, dtype=torch.float64, device=M.device)
        reg[D - 1] = 0.0
        M.copy_((0.5 * G + torch.diag(reg)) / tab.info[2])

    def util_factor(self, M, Lt=None, X=None, Minv=None):
        """Minv = (M + 1e-10 trace(M) / D I)^-1 through the Cholesky factor (LAPACK on the host)."""
        D = M.shape[0]
        A = M.detach().cpu()
        A = A + torch.eye(D, dtype=torch.float64) * (1e-10 * torch.trace(A) / D)
        Minv.copy_(torch.cholesky_inverse(torch.linalg.cholesky(A)).to(M.device))

    def _util_logits(self, tab, n, P, codes):
        nc, ol = tab.cont.shape[1], tab.offs.tolist()
        Z = tab.cont[:n] @ P[:nc] + P[tab.D - 1][None, :]
        for c, code in enumerate(codes):
            Z = Z + P[nc + ol[c] + code]
        return Z

    def util_grad(self, tab, n, P, G, loss, part=None, lossp=None):
        """G [D, K] = grad f(P) and loss[0] = f(P) of f(P) = (sum_i s_i CE(softmax(F_i P), y_i) + |P without its
        last row|^2 / 2) / S; the softmax runs over the classes with counts > 0, the others get probability 0."""
        D, K, nc = tab.D, tab.K, tab.cont.shape[1]
        codes, cl, ol = self._util_codes(tab, n), tab.card.tolist(), tab.offs.tolist()
        Z = self._util_logits(tab, n, P, codes)
        s, y = tab.s[:n], tab.y[:n].long()
        pres = (tab.counts > 0)[None, :]
        neg = torch.full_like(Z, float("-inf"))
        mx = torch.where(pres, Z, neg).max(dim=1).values
        mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        E = torch.where(pres, torch.exp(Z - mx[:, None]), torch.zeros_like(Z))
        den = E.sum(dim=1)
        den = torch.where(den > 0, den, torch.ones_like(den))
        yv = y.clamp(0, K - 1)
        Y = torch.zeros_like(Z).scatter_(1, yv[:, None], 1.0)
        R = s[:, None] * (E / den[:, None] - Y)
        rows = s * (torch.log(den) + mx - Z.gather(1, yv[:, None])[:, 0])
        rows = torch.where(s > 0, rows, torch.zeros_like(rows))
        R = torch.where((s > 0)[:, None], R, torch.zeros_like(R))
        g = torch.zeros(D, K, dtype=torch.float64, device=P.device)
        g[:nc] = tab.cont[:n].t() @ R
        g[D - 1] = R.sum(dim=0)
        for c, code in enumerate(codes):
            g[nc + ol[c]:nc + ol[c] + cl[c] + 1] = torch.zeros(cl[c] + 1, K, dtype=torch.float64,
                                                               device=P.device).index_add_(0, code, R)
        g[:D - 1] += P[:D - 1]
        S = tab.info[2]
        loss[0] = (rows.sum() + 0.5 * (P[:D - 1] * P[:D - 1]).sum()) / S
        G.copy_(g / S)

    def util_step(self, tab, n, V, W, Minv, G, loss, part=None, lossp=None, beta=0.0):
        """One accelerated step: G = grad f(V); W' = V - Minv G; V' = W' + beta (W' - W)."""
        self.util_grad(tab, n, V, G, loss)
        wn = V - Minv @ G
        V.copy_(wn + float(beta) * (wn - W))
        W.copy_(wn)

    def util_predict(self, tab, n, train_counts, W, conf, G, loss, real, out):
        """conf [K, K] int32: rows of ``tab`` by (target code, predicted class), the prediction being the largest
        logit over the classes with train_counts > 0 (the lowest such class on a tie), rows whose target is no code
        skipped.  out[0..7] = weighted F1, accuracy, real[0], real[1], real[0] - F1, real[1] - accuracy, loss[0],
        max |G|."""
        Z = self._util_logits(tab, n, W, self._util_codes(tab, n))
        self._predict_conf(Z, train_counts, tab.y[:n].long(), tab.K, conf, real, out)
        out[6], out[7] = loss[0], G.abs().max()

    @staticmethod
    def _predict_conf(Z, train_counts, y, K, conf, real, out):
        """conf and out[0..5] of util_predict / mlp_predict from the logits Z [n, K] and the target codes y"""
        pres = (train_counts > 0)[None, :]
        Zm = torch.where(pres, Z, torch.full_like(Z, float("-inf")))
        mx = Zm.max(dim=1).values
        idx = torch.arange(K, device=Z.device)[None, :].expand_as(Z)
        pred = torch.where(Zm == mx[:, None], idx, torch.full_like(idx, K)).min(dim=1).values.clamp(max=K - 1)
        ok = (y >= 0) & (y < K)
        c = torch.bincount(y[ok] * K + pred[ok], minlength=K * K).view(K, K)
        conf.copy_(c.to(conf.dtype).view(conf.shape))
        cd = c.to(torch.float64)
        rs, cs, tp = cd.sum(dim=1), cd.sum(dim=0), torch.diagonal(cd)
        den = rs + cs
        f = torch.where(den > 0, 2.0 * tp / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
        total = rs.sum()
        safe = torch.where(total > 0, total, torch.ones_like(total))
        f1 = torch.where(total > 0, (rs * f).sum() / safe, torch.zeros_like(total))
        acc = torch.where(total > 0, tp.sum() / safe, torch.zeros_like(total))
        out[0], out[1], out[2], out[3] = f1, acc, real[0], real[1]
        out[4], out[5] = real[0] - f1, real[1] - acc

    # ------------------------------------------------------------------ MLP-utility evaluator (eval/mlp_device.py)
    MLP_MAX_HIDDEN, MLP_MAX_BATCH, MLP_MAX_STEPS, MLP_ROWS = 128, 1024, 10000, 64    # the HIP kernels' limits

    def _mlp_forward(self, tab, idx, theta, H):
        """(W1, W2, codes, h, z) of the rows idx of a packed table: h = relu(F W1), z = [h | 1] W2, the one-hot part
        of F W1 as the rows of W1 that the clamped codes select"""
        D, K, nc, ol = tab.D, tab.K, tab.cont.shape[1], tab.offs.tolist()
        W1, W2 = theta[:D * H].view(D, H), theta[D * H:D * H + (H + 1) * K].view(H + 1, K)
        codes = [tab.cat_t[c].long()[idx].clamp(0, Kc) for c, Kc in enumerate(tab.card.tolist())]
        pre = tab.cont[idx] @ W1[:nc]
        for c, code in enumerate(codes):
            pre = pre + W1[nc + ol[c] + code]
        h = torch.clamp(pre + W1[D - 1][None, :], min=0.0)
        return W1, W2, codes, h, h @ W2[:H] + W2[H][None, :]

    @staticmethod
    def _mlp_softmax(Z, y, counts, K):
        """(valid rows, P - Y with zero rows where y is no code, the rows' cross entropies): the softmax runs over the
        classes with counts > 0, the others get probability 0"""
        pres = (counts > 0)[None, :]
        mx = torch.where(pres, Z, torch.full_like(Z, float("-inf"))).max(dim=1).values
        mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        E = torch.where(pres, torch.exp(Z - mx[:, None]), torch.zeros_like(Z))
        den = E.sum(dim=1)
        den = torch.where(den > 0, den, torch.ones_like(den))
        valid = (y >= 0) & (y < K)
        yv = y.clamp(0, K - 1)
        Y = torch.zeros_like(Z).scatter_(1, yv[:, None], 1.0)
        dZ = torch.where(valid[:, None], E / den[:, None] - Y, torch.zeros_like(Z))
        ce = torch.log(den) + mx - Z.gather(1, yv[:, None])[:, 0]
        return valid, dZ, torch.where(valid, ce, torch.zeros_like(ce))

    def mlp_step(self, tab, n, b, nb, theta, m, v, h, dz, dh, cnt, H, alpha, lr_t):
        """One Adam step of the network theta = [W1 [D, H] | W2 [H + 1, K]] (the last rows the biases) on batch b of
        nb of the packed table ``tab``: its rows b, b + nb, ... < n.  g = grad of (sum over the batch's valid rows of
        CE(softmax([relu(F W1) | 1] W2), y) + alpha / 2 |W1, W2 without their bias rows|^2) / max(valid rows, 1); m
        = 0.9 m + 0.1 g, v = 0.999 v + 0.001 g^2, theta -= lr_t m / (sqrt(v) + 1e-8).  Scratch: h / dh float64
        [>= rows H], dz float64 [>= rows K] (the batch's h, dH and dZ) and cnt int32 [>= ceil(rows / MLP_ROWS)] (valid
        rows per block of MLP_ROWS batch rows)."""
        D, K, nc = tab.D, tab.K, tab.cont.shape[1]
        cl, ol = tab.card.tolist(), tab.offs.tolist()
        idx = torch.arange(int(b), int(n), int(nb), device=theta.device)
        rows = int(idx.numel())
        if not 0 <= int(b) < int(nb) <= int(n) or rows > self.MLP_MAX_BATCH:
            raise ValueError(f"mlp_step: batch {b} of {nb} over {n} rows has {rows} rows; MLP_MAX_BATCH = "
                             f"{self.MLP_MAX_BATCH}")
        W1, W2, codes, hh, Z = self._mlp_forward(tab, idx, theta, H)
        valid, dZ, _ = self._mlp_softmax(Z, tab.y.long()[idx], tab.counts, K)
        dH = (dZ @ W2[:H].t()) * (hh > 0).to(dZ.dtype)
        g1 = torch.zeros(D, H, dtype=torch.float64, device=theta.device)
        g1[:nc] = tab.cont[idx].t() @ dH
        g1[D - 1] = dH.sum(dim=0)
        for c, code in enumerate(codes):
            g1[nc + ol[c]:nc + ol[c] + cl[c] + 1] = torch.zeros(cl[c] + 1, H, dtype=torch.float64,
                                                               device=theta.device).index_add_(0, code, dH)
        g1[:D - 1] += alpha * W1[:D - 1]
        g2 = torch.cat([hh.t() @ dZ + alpha * W2[:H], dZ.sum(dim=0)[None, :]], dim=0)
        nv = valid.sum()
        g = torch.cat([g1.reshape(-1), g2.reshape(-1)]) / nv.clamp(min=1).to(torch.float64)
        blocks = (rows + self.MLP_ROWS - 1) // self.MLP_ROWS
        pad = torch.zeros(blocks * self.MLP_ROWS, dtype=torch.int64, device=theta.device)
        pad[:rows] = valid.long()
        cnt[:blocks] = pad.view(blocks, self.MLP_ROWS).sum(dim=1).to(cnt.dtype)
        h.view(-1)[:rows * H] = hh.reshape(-1)
        dh.view(-1)[:rows * H] = dH.reshape(-1)
        dz.view(-1)[:rows * K] = dZ.reshape(-1)
        m.mul_(0.9).add_(0.1 * g)
        v.mul_(0.999).add_(0.001 * g * g)
        theta.sub_(float(lr_t) * m / (torch.sqrt(v) + 1e-8))

    def mlp_loss(self, tab, n, theta, H, alpha, loss):
        """loss[0] = the objective of mlp_step over all n rows of ``tab`` (divided by its valid rows, 1 when there is
        none).  loss: float64 [>= 1 + ceil(n / MLP_ROWS)]; what follows loss[0] is scratch of the HIP kernels."""
        D, K = tab.D, tab.K
        idx = torch.arange(int(n), device=theta.device)
        W1, W2, _, _, Z = self._mlp_forward(tab, idx, theta, H)
        valid, _, ce = self._mlp_softmax(Z, tab.y.long()[idx], tab.counts, K)
        l2 = (W1[:D - 1] * W1[:D - 1]).sum() + (W2[:H] * W2[:H]).sum()
        loss[0] = (ce.sum() + 0.5 * alpha * l2) / valid.sum().clamp(min=1).to(torch.float64)

    def mlp_predict(self, tab, n, train_counts, theta, H, conf, loss, real, out):
        """conf [K, K] int32 as util_predict's, from the network's logits; out[0..6] = weighted F1, accuracy, real[0],
        real[1], real[0] - F1, real[1] - accuracy, loss[0]."""
        idx = torch.arange(int(n), device=theta.device)
        Z = self._mlp_forward(tab, idx, theta, H)[4]
        self._predict_conf(Z, train_counts, tab.y[:n].long(), tab.K, conf, real, out)
        out[6] = loss[0]

    # ------------------------------------------------------------------ tree-utility evaluator (eval/forest_device.py)
    TREE_CONT, TREE_CAT, TREE_TARGET = 0, 1, 2
    TREE_MAX_BINS, TREE_MAX_CLASSES, TREE_MAX_DEPTH, TREE_MAX_FEATURES = 256, 64, 20, 1024   # the HIP kernels' limits
    TREE_STREAM_DRAW, TREE_STREAM_FEAT = 0x74726231, 0x74726632      # Philox stream ids no other call site uses

    @staticmethod
    def _tree_mulhilo(a: int, c):
        """(hi, lo) 32-bit halves of a * c for a < 2^32 and int64 c < 2^32, without leaving 63 bits"""
        lo16, hi16 = a * (c & 0xFFFF), a * (c >> 16)
        t = hi16 + (lo16 >> 16)
        return t >> 16, ((t & 0xFFFF) << 16) | (lo16 & 0xFFFF)

    @classmethod
    def tree_word(cls, seed: int, stream: int, w, hi, lo):
        """first word of Philox4x32-10 (kernels/common.h) of the counter (lo, hi, stream, w) under the key seed, in
        int64 tensors"""
        c0, c1, c3 = (x if torch.is_tensor(x) else torch.tensor(int(x), dtype=torch.int64) for x in (lo, hi, w))
        c0, c1, c3 = torch.broadcast_tensors(c0.long(), c1.long().to(c0.device), c3.long().to(c0.device))
        c2 = torch.full_like(c0, int(stream))
        k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
        for _ in range(10):
            h0, l0 = cls._tree_mulhilo(0xD2511F53, c0)
            h1, l1 = cls._tree_mulhilo(0xCD9E8D57, c2)
            c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        return c0

    def tree_pack(self, values, kind, slot, tab):
        """Bins the row-major float64 table ``values`` [n, n_cols] into ``tab`` (eval.forest_device.TreeTable):
        tab.bins[f, r] (uint8) is, for a continuous feature, the number of its edges below the value (0 for a NaN)
        and, for a categorical one with K_c categories, the code or K_c where the value is no code; tab.y the target's
        code or K; tab.counts the valid rows per class and tab.cw the balanced class weights ``n_valid / (K_present
        count_c)``, 0 for an absent class."""
        n, K = int(values.shape[0]), tab.K
        eoff = tab.eoff.tolist()
        card = tab.card.tolist()
        for j, (k, f) in enumerate(zip(kind.tolist(), slot.tolist())):
            v = values[:, j]
            if k == self.TREE_CONT:
                e = tab.edges[eoff[f]:eoff[f + 1]]
                b = torch.searchsorted(e, torch.nan_to_num(v, nan=float("-inf")).contiguous(), right=False)
                tab.bins[f, :n] = b.clamp(max=self.TREE_MAX_BINS - 1).to(torch.uint8)
                continue
            Kc = K if k == self.TREE_TARGET else card[f]
            code = _code_or_overflow(v, Kc).long()
            if k == self.TREE_TARGET:
                tab.y[:n] = code.to(torch.int32)
                tab.counts.copy_(torch.bincount(code, minlength=K + 1)[:K].to(torch.int32))
            else:
                tab.bins[f, :n] = code.to(torch.uint8)
        tab.cw.copy_(_balanced_weights(tab.counts)[0])

    def tree_bootstrap(self, mult, n, bootstrap, seed):
        """mult [T, >= n] int32: 1 per row, or with ``bootstrap`` how often tree t drew the row among its n draws,
        draw j being row ``mulhi32(word(t, j), n)``."""
        T = int(mult.shape[0])
        if not bootstrap:
            mult[:, :n] = 1
            return
        dev = mult.device
        j = torch.arange(n, dtype=torch.int64, device=dev)[None, :]
        t = torch.arange(T, dtype=torch.int64, device=dev)[:, None]
        w = self.tree_word(seed, self.TREE_STREAM_DRAW, 0, t, j)
        hi, _ = self._tree_mulhilo(int(n), w)
        m = torch.zeros(T, n, dtype=torch.int64, device=dev)
        m.scatter_add_(1, hi, torch.ones_like(hi))
        mult[:, :n] = m.to(torch.int32)

    def tree_grow(self, tab, n, model, max_depth, min_leaf, m_feat, seed):
        """Grows the ``model.T`` trees of ``model`` (eval.forest_device.TreeModel) level by level on the first n rows
        of ``tab`` with the multiplicities model.mult (rows with multiplicity 0 or no valid class are left out); the
        criterion, the tie order, the competing features and the node layout are those of eval/forest_device.py."""
        dev = tab.bins.device
        K, F, NB = tab.K, tab.F, int(tab.max_bins)
        bins, y, w = tab.bins[:, :n].long(), tab.y[:n].long(), tab.cw
        nb = tab.nbins.long()
        m_feat = min(int(m_feat), F)
        model.feature.fill_(-1)
        for z in (model.bin, model.left, model.heap, model.counts):
            z.zero_()
        ar_b = torch.arange(NB, device=dev)
        ar_f = torch.arange(F, device=dev)
        chunk = max(1, (1 << 22) // (F * NB * K))
        for t in range(model.T):
            mult = model.mult[t, :n].long()
            rows = ((mult > 0) & (y >= 0) & (y < K)).nonzero().flatten()
            yr, mr, br = y[rows], mult[rows], bins[:, rows]
            item = torch.zeros_like(rows)
            model.heap[t, 0] = 1
            model.counts[t, 0] = torch.zeros(K, dtype=torch.int64, device=dev).index_add_(0, yr, mr).to(torch.int32)
            start, count = 0, 1
            for _ in range(int(max_depth)):
                tot = model.counts[t, start:start + count].long()
                heap = model.heap[t, start:start + count].long()
                cand = (tot > 0).sum(dim=1) > 1
                bf = torch.full((count,), -1, dtype=torch.int64, device=dev)
                bb = torch.zeros(count, dtype=torch.int64, device=dev)
                lc = torch.zeros(count, K, dtype=torch.int64, device=dev)
                for i0 in range(0, count, chunk):
                    i1 = min(count, i0 + chunk)
                    if not bool(cand[i0:i1].any()):
                        continue
                    I = i1 - i0
                    idx = ((item >= i0) & (item < i1)).nonzero().flatten()
                    flat = (((item[idx] - i0)[None, :] * F + ar_f[:, None]) * NB + br[:, idx]) * K + yr[idx][None, :]
                    hist = torch.zeros(I * F * NB * K, dtype=torch.int64, device=dev)
                    hist.index_add_(0, flat.flatten(), mr[idx][None, :].expand(F, -1).flatten())
                    pre = hist.view(I, F, NB, K).cumsum(dim=2)
                    totc = tot[i0:i1]
                    nl = pre.sum(dim=3)
                    nr = totc.sum(dim=1)[:, None, None] - nl
                    TL = torch.zeros(I, F, NB, dtype=torch.float64, device=dev)
                    QL, TR, QR = TL.clone(), TL.clone(), TL.clone()
                    for c in range(K):
                        ml = pre[..., c].to(torch.float64) * w[c]
                        mrr = (totc[:, c][:, None, None] - pre[..., c]).to(torch.float64) * w[c]
                        TL = TL + ml
                        QL = QL + ml * ml
                        TR = TR + mrr
                        QR = QR + mrr * mrr
                    valid = ((nl >= min_leaf) & (nr >= min_leaf) & (TL > 0) & (TR > 0) &
                             (ar_b[None, None, :] < (nb - 1)[None, :, None]) & cand[i0:i1][:, None, None])
                    one = torch.ones_like(TL)
                    score = torch.where(valid, QL / torch.where(valid, TL, one) + QR / torch.where(valid, TR, one), -one)
                    fs = score.max(dim=2).values
                    fb = torch.where((score == fs[..., None]) & valid, ar_b, NB).min(dim=2).values
                    comp = valid.any(dim=2)
                    if m_feat < F:
                        keys = self.tree_word(seed, self.TREE_STREAM_FEAT, heap[i0:i1][:, None], t, ar_f[None, :])
                        order = torch.where(comp, (keys << 10) | ar_f[None, :], torch.full_like(keys, 1 << 62))
                        rank = torch.empty_like(order)
                        rank.scatter_(1, order.argsort(dim=1), ar_f[None, :].expand(I, -1).contiguous())
                        comp = comp & (rank < m_feat)
                    fs = torch.where(comp, fs, -torch.ones_like(fs))
                    best = fs.max(dim=1).values
                    f_star = torch.where((fs == best[:, None]) & comp, ar_f, F).min(dim=1).values
                    has = f_star < F
                    f_c = f_star.clamp(max=F - 1)
                    b_star = fb.gather(1, f_c[:, None])[:, 0].clamp(max=NB - 1)
                    bf[i0:i1] = torch.where(has, f_star, -torch.ones_like(f_star))
                    bb[i0:i1] = torch.where(has, b_star, torch.zeros_like(b_star))
                    lc[i0:i1] = pre[torch.arange(I, device=dev), f_c, b_star]
                split = bf >= 0
                rank = split.long().cumsum(0) - 1
                nxt = start + count
                n_split = int(split.sum())
                model.feature[t, start:nxt] = bf.to(torch.int32)
                model.bin[t, start:nxt] = bb.to(torch.int32)
                if n_split == 0:
                    break
                l = (nxt + 2 * rank)[split]
                model.left[t, start:nxt] = torch.where(split, nxt + 2 * rank, torch.zeros_like(rank)).to(torch.int32)
                model.heap[t, l] = (2 * heap[split]).to(torch.int32)
                model.heap[t, l + 1] = (2 * heap[split] + 1).to(torch.int32)
                model.counts[t, l] = lc[split].to(torch.int32)
                model.counts[t, l + 1] = (tot[split] - lc[split]).to(torch.int32)
                go = split[item]
                right = br[bf[item].clamp(min=0), torch.arange(item.numel(), device=dev)] > bb[item]
                new_item = 2 * rank[item] + right.long()
                item, yr, mr, br = new_item[go], yr[go], mr[go], br[:, go]
                start, count = nxt, 2 * n_split

    def tree_predict(self, tab, n, cw, model, soft, conf):
        """conf [K, K] int32: the first n rows of ``tab`` by (target code, predicted class).  A row walks every tree
        by its bins to a leaf with masses ``m_c = n_c cw_c``; hard (one tree): the largest m_c; soft: the largest sum
        over the trees, in tree order, of ``m_c / T_leaf`` (T_leaf the sum of m_c in class order; a leaf with T_leaf =
        0 adds nothing).  The lowest class wins a tie; rows whose target is no code are skipped."""
        dev = tab.bins.device
        K = tab.K
        bins, y = tab.bins[:, :n].long(), tab.y[:n].long()
        ar = torch.arange(n, device=dev)
        P = torch.zeros(n, K, dtype=torch.float64, device=dev)
        for t in range(model.T):
            feature, bn, left = model.feature[t].long(), model.bin[t].long(), model.left[t].long()
            node = torch.zeros(n, dtype=torch.int64, device=dev)
            for _ in range(self.TREE_MAX_DEPTH + 1):
                f = feature[node]
                act = f >= 0
                if not bool(act.any()):
                    break
                b = bins[f.clamp(min=0), ar]
                node = torch.where(act, left[node] + (b > bn[node]).long(), node)
            m = model.counts[t].long()[node].to(torch.float64) * cw[None, :]
            if not soft:
                P = m
                break
            T = torch.zeros(n, dtype=torch.float64, device=dev)
            for c in range(K):
                T = T + m[:, c]
            ok = (T > 0)[:, None]
            P = P + torch.where(ok, m / torch.where(ok, T[:, None], torch.ones_like(m)), torch.zeros_like(m))
        idx = torch.arange(K, device=dev)[None, :].expand_as(P)
        pred = torch.where(P == P.max(dim=1).values[:, None], idx, torch.full_like(idx, K)).min(dim=1).values
        pred = pred.clamp(max=K - 1)
        ok = (y >= 0) & (y < K)
        conf.copy_(torch.bincount(y[ok] * K + pred[ok], minlength=K * K).view(K, K).to(conf.dtype))

    def tree_scores(self, conf, real, out):
        """out[0..5] = weighted F1, accuracy, real[0], real[1], real[0] - F1, real[1] - accuracy of the confusion
        matrix, the F1 terms added in class order"""
        cd = conf.to(torch.float64)
        rs, cs, tp = cd.sum(dim=1), cd.sum(dim=0), torch.diagonal(cd)
        den = rs + cs
        f = torch.where(den > 0, (2.0 * tp) / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
        total = rs.sum()
        safe = torch.where(total > 0, total, torch.ones_like(total))
        acc_f1 = torch.zeros((), dtype=torch.float64, device=conf.device)
        for c in range(int(conf.shape[0])):
            acc_f1 = acc_f1 + rs[c] * f[c]
        f1 = torch.where(total > 0, acc_f1 / safe, torch.zeros_like(total))
        acc = torch.where(total > 0, tp.sum() / safe, torch.zeros_like(total))
        out[0], out[1], out[2], out[3] = f1, acc, real[0], real[1]
        out[4], out[5] = real[0] - f1, real[1] - acc
