"""CTGANEngine's table generation (plain, conditional, pipelined; eager or as replayed hipGraphs): a mixin that reads
the engine's parameters, dimensions and ops and owns the attributes ``_init_generation`` sets.  A pass is sample ->
eval generator (fp32 storage, or bf16 with ``gen16``: bit-identical) -> decode, per chunk of ``gen_chunk`` rows."""
from __future__ import annotations

import dataclasses
from functools import partial
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ..utils.devsync import warm_and_capture
from .arena import _padded_rows
from .samplers import CondTables


@dataclasses.dataclass
class GenGraph:
    """A captured pass for one row count: the static buffers (one chunk's rows; ``out``: the table) and the graph(s)."""
    H: torch.Tensor
    logits: torch.Tensor
    col: torch.Tensor
    opt: torch.Tensor
    out: torch.Tensor
    graph: Optional["torch.cuda.CUDAGraph"] = None    # the pass; pipelined generation: its body
    prep: Optional["torch.cuda.CUDAGraph"] = None     # pipelined generation only: the snapshot of what the body reads

    def rows(self, k: int):
        return self.H[:k], self.logits[:k], self.col[:k], self.opt[:k]


class GenerationMixin:
    def _init_generation(self):
        self.gen_tables = self.gen_cond = self.gen_counts = None    # set_generation_tables
        # _gen_bufs: (H, logits, col, opt) of the eager passes, grown on demand; _gen_graphs / _gen_split: n -> the
        # captured generate_decoded(n) / prep + body of generate_decoded_split(n); _cond_ent: (m, bins, fixed
        # columns) -> buffers / hipGraph of a conditional pass, _guard_ent: the same of a guarded pass; _known_ent:
        # (m, tries) -> the same of a completion pass; _gen_prepped: event, the last pipelined prep is issued
        self._drop_generation()
        self._gen_done = None                     # event: the last pipelined generation body has finished
        self.last_conditional = None              # generate_decoded_where: passes, rows generated / kept, filled counts
        self.last_guard = None                    # generate_decoded_guarded: passes, rows generated / rejected / kept
        self.last_known = None                    # generate_decoded_known: sweeps, rows generated / open, distances
        self._known_transformer = None            # set_generation_tables: the transformer build_known reads
        self._gw16 = self._gwt = None             # bf16 / transposed generation copies of the generator weights
        self._gsnap = self._gsnap_pairs = self._gsnap_ctr = None      # pipelined generation: parameter / RNG snapshot

    def set_generation_tables(self, cond: CondTables, transformer):
        """Tables for sample_zero + fused decode (transformer: a fitted VGMTransformer)."""
        dev = self.device
        self.gen_cond = {
            "cdf_emp": torch.as_tensor(cond.cdf_emp, dtype=torch.float32, device=dev),
            "cond_offset": torch.as_tensor(self.layout.cond_offset, dtype=torch.int32, device=dev),
            "cond_width": torch.as_tensor(self.layout.cond_width, dtype=torch.int32, device=dev),
        }
        mu, sd = transformer.decode_tables()
        cols, pos, c = [], 0, 0
        for m in transformer.meta:
            if m["type"] == "continuous":
                nv = int(transformer.components[c].sum())
                cols.append((0, pos, nv, c, None))
                pos += 1 + nv
                c += 1
            else:
                w = int(m["size"])
                codes = torch.as_tensor(np.asarray(m["i2s"], dtype=np.float64), device=dev)
                cols.append((1, pos, w, -1, codes))
                pos += w
        self.gen_counts = np.asarray(cond.counts, dtype=np.float64)      # the span counts a driving range / set weighs
        self.gen_tables = {"cols": cols, "mu": torch.as_tensor(mu, dtype=torch.float64, device=dev),
                           "sd": torch.as_tensor(sd, dtype=torch.float64, device=dev)}
        self._known_transformer = transformer
        self._drop_generation()

    def _drop_generation(self) -> None:
        """Forget everything sized by or captured on the generation tables (the weight copies and the pipelined
        snapshot depend on the parameters alone and stay)."""
        self._gen_graphs: Dict[int, GenGraph] = {}
        self._gen_split: Dict[int, GenGraph] = {}
        self._cond_ent: Dict[tuple, dict] = {}
        self._guard_ent: Dict[tuple, dict] = {}
        self._known_ent: Dict[tuple, dict] = {}
        self._gen_bufs = self._gen_prepped = None

    def _prepare_generation_graphs(self, gen_rows: Sequence[int], gen_split: bool) -> None:
        """prepare_graphs' generation part: capture generate_decoded(n) / generate_decoded_split(n) ahead."""
        if self.gen_tables is None or not self._graphs_for_generation():
            return
        split = gen_split and self.can_split_generation()
        for n in (int(n) for n in gen_rows if n > 0):
            if n not in (self._gen_split if split else self._gen_graphs):
                (self._capture_gen_split if split else self._capture_gen)(n)

    def _graphs_for_generation(self) -> bool:
        """Generation passes replay hipGraphs unless asked otherwise: on a GPU with the HIP backend and gen_graph."""
        return self.device.type == "cuda" and self.cfg.gen_graph and self.ops.name == "hip"

    def _wait_gen_done(self) -> None:
        """The current stream queues behind a pipelined body that may still read the weight copies / the snapshot."""
        if self._gen_done is not None:
            torch.cuda.current_stream(self.device).wait_event(self._gen_done)

    def _decoded(self, n: int) -> torch.Tensor:
        return torch.empty(n, len(self.gen_tables["cols"]), dtype=torch.float64, device=self.device)

    # ------------------------------------------------------------------ buffers / weights / forward
    @property
    def gen16(self) -> bool:
        """Generation in bf16 storage (EngineConfig.gen_bf16): HIP bf16 backend, one-hot generator
        GEMMs, and 8-aligned column offsets (16-B bf16 operand rows)."""
        return (self.cfg.gen_bf16 and self.ops.name == "hip" and not getattr(self.ops, "f32", True) and
                self.use_onehot and all(o % 8 == 0 for o in self.off))

    def _gen_alloc(self, rows: int, bf16: bool):
        """Static buffers of a pass over ``rows`` rows: (H, logits, col, opt).  H: the fp32 activation buffer, or
        with ``bf16`` [rows, ceil8(c0)] bf16 activations [out_{L-1} | ... | out_0 | z] (no one-hot block)."""
        dev = self.device
        H = torch.zeros(rows, -(-self.c_cols[0] // 8) * 8, dtype=torch.bfloat16, device=dev) if bf16 else \
            _padded_rows(rows, self.Hw, dev)
        return (H, _padded_rows(rows, self.Dd, dev), torch.zeros(rows, dtype=torch.int32, device=dev),
                torch.zeros(rows, dtype=torch.int32, device=dev))

    def _gen_buffers(self, n: int, bf16: bool | None = None):
        """The eager passes' buffers, first n rows."""
        bf16 = self.gen16 if bf16 is None else bf16
        if self._gen_bufs is None or self._gen_bufs[0].shape[0] < n or \
                (self._gen_bufs[0].dtype == torch.bfloat16) != bf16:
            self._gen_bufs = self._gen_alloc(n, bf16)
        return tuple(t[:n] for t in self._gen_bufs)

    def _gen_weights16(self):
        """Generation views of the generator weights, refreshed from the current fp32 weights inside
        the generation graph (every replay sees the aggregated model), in ONE launch: per layer the
        bf16 copy of the dense columns and the one-hot block transposed to [C, N] fp32.
        Returns (bf16 copies, transposed blocks), one per layer (G-out last)."""
        c0 = self.c_cols[0]
        names = [f"G.{i}.W" for i in range(len(self.gdims))] + ["G.out.W"]
        starts = list(self.off[:len(self.gdims)]) + [0]
        if self._gw16 is None:
            self._gw16 = [torch.zeros(self.p[nm].shape[0], -(-(c0 - a) // 8) * 8, dtype=torch.bfloat16,
                                      device=self.device) for nm, a in zip(names, starts)]
            self._gwt = [torch.zeros(self.p[nm].shape[1] - (c0 - a), self.p[nm].shape[0], device=self.device)
                         for nm, a in zip(names, starts)]
        self.ops.L.gen_weight_prep([self.p[nm] for nm in names], [c0 - a for a in starts], self._gw16, self._gwt)
        return self._gw16, self._gwt

    def _g_forward16(self, H16, logits, w16, cond, params=None):
        """Eval-mode generator on the bf16 buffer: each layer's GEMM reads bf16 rows and weights,
        gathers the one-hot block from col / opt, and writes bf16 (BN-eval + ReLU epilogue); the output
        layer writes fp32 logits.  w16 = _gen_weights16(); params: biases / BN tensors by name (default the
        live ones; the pipelined generation passes its snapshot)."""
        o, p = self.ops, (self.p if params is None else params)
        c0 = self.c_cols[0]
        col, opt = cond
        wd, wt = w16
        for i, g in enumerate(self.gdims):
            a, b_ = self.off[i], self.off[i + 1]
            oh = (wt[i], col, opt, self._cond_off, True)
            o.linear_bn_relu(H16[:, a:c0], wd[i], p[f"G.{i}.b"], p[f"G.{i}.gamma"], p[f"G.{i}.beta"], H16[:, b_:a],
                             None, None, None, None, p[f"G.{i}.rm"], p[f"G.{i}.rv"], False, self.cfg.bn_momentum,
                             self.cfg.bn_eps, onehot=oh)
        oh = (wt[-1], col, opt, self._cond_off, True)
        o.gemm(H16[:, :c0], wd[-1], logits, tb=True, bias=p["G.out.b"], onehot=oh)

    def _gen_forward(self, H, logits, col, opt, w16=None, params=None):
        """The eval generator of a pass: on fp32 storage, or with ``w16`` (see _g_forward16) on the bf16 buffer."""
        if w16 is None:
            self._g_forward(H, logits, training=False, nhat=False, cond=(col, opt, True))
        else:
            self._g_forward16(H, logits, w16, (col, opt), params=params)

    def _gen_chunks(self, n: int, out: torch.Tensor, bufs, w16, params=None, ctr=None):
        """The chunk loop of a decoded pass: sample -> eval generator -> decode into ``out``.  ``bufs(k)``: a chunk's
        (H, logits, col, opt); ``ctr``: the RNG step counter the draws are keyed on (default the live one)."""
        kw = {} if ctr is None else {"ctr": ctr}
        for a in range(0, n, self.cfg.gen_chunk):
            b = min(n, a + self.cfg.gen_chunk)
            H, logits, col, opt = bufs(b - a)
            self.ops.sample_gen(self.gen_cond, H, self.c_cols, self.z_cols, col_out=col, opt_out=opt, stream_id=21, **kw)
            self._gen_forward(H, logits, col, opt, w16, params)
            self.ops.sample_decode(logits, out[a:b], self.gen_tables, stream_id=23, **kw)

    def _gen_pass(self, n: int, out: torch.Tensor, bufs):
        """generate_decoded's pass: the live model, its bf16 copies refreshed in the pass."""
        self._gen_chunks(n, out, bufs, self._gen_weights16() if self.gen16 else None)

    # ------------------------------------------------------------------ plain generation
    @torch.no_grad()
    def generate_encoded(self, n: int) -> torch.Tensor:
        """Activated generator output for n rows (eval BN): [n, data_dim]."""
        out = torch.empty(n, self.Dd, device=self.device)
        for a in range(0, n, self.cfg.gen_chunk):
            b = min(n, a + self.cfg.gen_chunk)
            H, logits, col, opt = self._gen_buffers(b - a, bf16=False)
            self.ops.sample_gen(self.gen_cond, H, self.c_cols, self.z_cols, col_out=col, opt_out=opt, stream_id=21)
            self._gen_forward(H, logits, col, opt)
            self.ops.activate(logits, out[a:b], self.spans, self.cfg.tau, stream_id=22)
        return out

    @torch.no_grad()
    def generate_decoded(self, n: int, use_graph: bool | None = None) -> torch.Tensor:
        """Fused sample -> G(eval) -> Gumbel-argmax/tanh decode: [n, n_cols] float64 on device.

        On a GPU the whole pass for a given n (every chunk's sampler, eval-BN GEMMs and decode
        launches) is captured once into a hipGraph and replayed each round; the result is a fresh
        tensor (a device copy of the graph's static output)."""
        if self.gen_tables is None:
            raise RuntimeError("set_generation_tables() first")
        if use_graph is None:
            use_graph = self._graphs_for_generation()
        self._wait_gen_done()
        if use_graph:
            ent = self._gen_graphs.get(n) or self._capture_gen(n)
            ent.graph.replay()
            out = ent.out.clone()
        else:
            out = self._decoded(n)
            self._gen_pass(n, out, self._gen_buffers)
        if hasattr(self.ops, "check"):
            self.ops.check()
        return out

    def _capture_gen(self, n: int) -> GenGraph:
        """Capture generate_decoded(n).  Nothing is restored: the warm-up (decode tables, lazy init) advances the RNG."""
        ent = GenGraph(*self._gen_alloc(min(n, self.cfg.gen_chunk), self.gen16), self._decoded(n))
        run = partial(self._gen_pass, n, ent.out, ent.rows)
        ent.graph, = warm_and_capture(self.device, run, [run], mode=self.capture_mode)
        self._gen_graphs[n] = ent
        return ent

    # ------------------------------------------------------------------ conditional generation
    @torch.no_grad()
    def generate_decoded_where(self, n: int, request: dict, max_passes: int = 64, chunk: int | None = None,
                               use_graph: bool | None = None) -> torch.Tensor:
        """Exactly n decoded rows carrying the requested category values: [n, n_cols] float64 on the device, grouped
        by the driving column's requested values in request order, in generation order (pass, then row) inside a
        group.  ``request``: models/conditional.py build_request (its quotas sum to n).

        One pass over m rows (``chunk``, default a size fitted to n, at most cfg.gen_chunk): sample_gen ->
        cond_request (every row's condition becomes the driving column's value of a bin drawn in proportion to the
        open quotas) -> eval generator -> sample_decode -> cond_partition (rows that carry every requested value move
        into their bin's quota segment).  The request lives in device buffers, so on the HIP backend with
        cfg.gen_graph the pass is captured once per (m, bins, fixed columns) and replayed; use_graph=False issues the
        same launches eagerly, and both give bit-identical tables from equal engine states.  Passes are issued in
        bursts that cannot overshoot (ceil(open quota / m) of them), with one readback of the filled counters per
        burst; max_passes passes without every quota full raise ConditionalSamplingError (no partial table).
        ``self.last_conditional`` records passes, rows generated, rows kept and the per-value counts.

        A request with range / set predicates (build_request) adds pred_mark after the decode: a row that fails a
        predicate loses its target before the partition.  When a predicate drives, pred_request takes cond_request's
        place (the driving span's options drawn by weight), the request has one bin, cond_partition compares no
        value, and the rows come back in generation order.  Entries and captured passes are then also keyed by the
        predicate shape (predicates, driver options, set-table bytes, whether a predicate drives);
        ``last_conditional["predicates"]`` lists per predicate its column, the rows it tested and the rows whose
        first failure it was, and a ConditionalSamplingError names the predicate with the most first failures."""
        from .conditional import ConditionalSamplingError
        if self.gen_tables is None:
            raise RuntimeError("set_generation_tables() first")
        n = int(n)
        quotas = [int(q) for q in request["quotas"]]
        if n != int(request["n"]) or sum(quotas) != n:
            raise ValueError(f"the request was built for {request['n']} rows, not {n}")
        nb, nf = len(quotas), int(request["fixed_j"].numel())
        if nb > getattr(self.ops, "COND_MAX_BINS", 64):
            raise ValueError(f"{nb} requested values; the kernels' bin limit is {self.ops.COND_MAX_BINS}")
        if n == 0:
            self.last_conditional = {"passes": 0, "generated": 0, "kept": 0, "filled": [0] * nb,
                                     "values": list(request["values"])}
            return self._decoded(0)
        if use_graph is None:
            use_graph = self._graphs_for_generation()
        if chunk is not None:
            m = int(chunk)
            if m < 1:
                raise ValueError("chunk must be positive")
        else:       # a power of two with a quarter of slack for rejected rows: few distinct sizes to capture
            m = min(int(self.cfg.gen_chunk), max(1024, 1 << int(np.ceil(np.log2(max(1.25 * n, 1.0))))))
        self._wait_gen_done()
        ent = self._cond_entry(m, nb, nf, n, self._pred_shape(request))
        for k in self._request_keys(ent):
            ent["req"][k].copy_(request[k])
        ent["req"]["filled"].zero_()
        ent["req"]["stats"].zero_()
        if ent["P"]:
            ent["req"]["pred_stats"].zero_()
        if use_graph and ent.get("graph") is None:
            self._capture_cond(ent, m)
        passes, filled = 0, [0] * nb
        while True:
            open_rows = sum(q - f for q, f in zip(quotas, filled))
            if open_rows <= 0:
                break
            if passes >= int(max_passes):
                self.last_conditional = self._cond_report(ent, request, passes, filled)
                if hasattr(self.ops, "check"):     # (a request pointing outside its tables fills nothing: say that)
                    self.ops.check()
                raise ConditionalSamplingError(
                    f"{passes} passes of {m} rows filled {sum(filled)} of {n} requested rows "
                    f"(per value: {dict(zip(map(str, request['values']), filled))})"
                    f"{self._worst_predicate(self.last_conditional)}", filled, quotas, request["values"])
            burst = max(1, min(-(-open_rows // m), int(max_passes) - passes))
            for _ in range(burst):
                if use_graph:
                    ent["graph"].replay()
                else:
                    self._cond_pass(ent, m)
            passes += burst
            filled = [int(x) for x in ent["req"]["filled"].tolist()]     # the one readback per burst
        out = ent["dst"][:n].clone()
        self.last_conditional = self._cond_report(ent, request, passes, filled)
        if hasattr(self.ops, "check"):
            self.ops.check()
        return out

    def _cond_report(self, ent, request, passes, filled):
        st = ent["req"]["stats"].tolist()
        rep = {"passes": int(passes), "generated": int(st[0]), "kept": int(st[1]), "filled": list(filled),
               "values": list(request["values"])}
        if ent.get("P"):
            # predicate k tests the rows its predecessors let through; "rejected": the rows whose first failure it is
            from .conditional import describe_predicate
            ps = ent["req"]["pred_stats"].tolist()
            desc = list(request.get("predicates") or [])
            tested, preds = int(ps[0]), []
            for k in range(ent["P"]):
                # (a hand-made request carries no description: its column index stands in)
                col, text = (desc[k][0], describe_predicate(desc[k])) if k < len(desc) else \
                    (int(request["pred_j"][k]), f"{k} on column {int(request['pred_j'][k])}")
                preds.append({"column": col, "predicate": text, "tested": tested, "rejected": int(ps[2 + k])})
                tested -= int(ps[2 + k])
            rep["predicates"] = preds
        return rep

    @staticmethod
    def _worst_predicate(report) -> str:
        """The clause of a ConditionalSamplingError that names the predicate with the most first failures."""
        preds = (report or {}).get("predicates")
        if not preds:
            return ""
        w = max(preds, key=lambda p: p["rejected"])
        return (f"; the predicate {w['predicate']} rejected {w['rejected']} of the {w['tested']} rows it tested "
                f"({100.0 * w['rejected'] / max(w['tested'], 1):.1f} %)")

    @staticmethod
    def _pred_shape(request) -> tuple:
        """(predicates, driver options, bytes of the sets' tables, a predicate drives) of a request: with (m, bins,
        fixed columns) the shape an entry's static buffers and its captured pass are made for."""
        if request is None or "pred_j" not in request:
            return (0, 0, 0, False)
        drives = "drv" in request
        return (int(request["pred_j"].numel()), int(request["drv_opt"].numel()) if drives else 0,
                int(request["pred_lut"].numel()), drives)

    @staticmethod
    def _request_keys(ent) -> tuple:
        """The request buffers copied into an entry's static ones."""
        keys = ("drive", "bin_opt", "bin_code", "quota", "seg_off", "fixed_j", "fixed_code")
        if ent["P"]:
            keys += ("pred_j", "pred_kind", "pred_lo", "pred_hi", "pred_lut_off", "pred_lut_len", "pred_lut")
        if ent["drives"]:
            keys += ("drv", "drv_opt", "drv_cum")
        return keys

    def _pred_buffers(self, req: dict, pshape: tuple) -> None:
        """The static predicate buffers of an entry (see _pred_shape), added to its request buffers."""
        P, M, L, drives = pshape
        dev = self.device
        z = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)      # noqa: E731
        if P:
            if P > getattr(self.ops, "PRED_MAX", 16):
                raise ValueError(f"{P} predicates; the kernels' limit is {self.ops.PRED_MAX}")
            req.update({"pred_j": z(P, torch.int32), "pred_kind": z(P, torch.int32), "pred_lo": z(P, torch.float64),
                        "pred_hi": z(P, torch.float64), "pred_lut_off": z(P, torch.int32),
                        "pred_lut_len": z(P, torch.int32), "pred_lut": z(L, torch.uint8),
                        "pred_stats": z(2 + 16, torch.int64)})
        if drives:
            req.update({"drv": z(2, torch.int32), "drv_opt": z(M, torch.int32), "drv_cum": z(M, torch.float64)})

    def _cond_entry(self, m: int, nb: int, nf: int, n: int, pshape: tuple = (0, 0, 0, False)) -> dict:
        """Static buffers of a conditional pass over m rows for requests of nb bins and nf fixed columns (and
        ``pshape``, _pred_shape: predicates, driver options, set-table bytes, whether a predicate drives): the pass's
        activations / logits / conditions / targets / decoded rows, the request buffers the launches read, and the
        quota segments (grown, and the graph dropped, when a request asks for more rows)."""
        pshape = tuple(pshape)
        key = (m, nb, nf) if pshape == (0, 0, 0, False) else (m, nb, nf) + pshape
        ent = self._cond_ent.get(key)
        dev = self.device
        if ent is None:
            H, lg, col, opt = self._gen_alloc(m, self.gen16)
            i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)      # noqa: E731
            i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)      # noqa: E731
            f64 = lambda k: torch.zeros(k, dtype=torch.float64, device=dev)    # noqa: E731
            ent = {"H": H, "lg": lg, "col": col, "opt": opt, "tgt": i32(m), "out": self._decoded(m),
                   "req": {"drive": i32(2), "bin_opt": i32(nb), "bin_code": f64(nb), "quota": i64(nb),
                           "filled": i64(nb), "seg_off": i64(nb), "fixed_j": i32(nf), "fixed_code": f64(nf),
                           "stats": i64(2)},
                   "P": pshape[0], "drives": bool(pshape[3]), "dst": None, "graph": None}
            self._pred_buffers(ent["req"], pshape)
            self._cond_ent[key] = ent
        if ent["dst"] is None or ent["dst"].shape[0] < n:
            if ent["graph"] is not None:
                torch.cuda.synchronize(dev)
            ent["graph"] = None
            ent["dst"] = self._decoded(n)
        return ent

    def _cond_pass(self, ent: dict, m: int):
        o, req = self.ops, ent["req"]
        H, lg, col, opt, tgt = ent["H"], ent["lg"], ent["col"], ent["opt"], ent["tgt"]
        w16 = self._gen_weights16() if self.gen16 else None
        o.sample_gen(self.gen_cond, H, self.c_cols, self.z_cols, col_out=col, opt_out=opt, stream_id=21)
        # (stream 24: the request's own Philox stream; 21-23 are the generation sampler's, activation's and decode's)
        if ent["drives"]:   # (stream 25: the weighted draw of a driving range / set)
            o.pred_request(req, col, opt, tgt, self.gen_cond, h=None if w16 is not None else H, c_col0=self.c_cols[0],
                           stream_id=25)
        else:
            o.cond_request(req, col, opt, tgt, self.gen_cond, h=None if w16 is not None else H,
                           c_col0=self.c_cols[0], stream_id=24)
        self._gen_forward(H, lg, col, opt, w16)
        o.sample_decode(lg, ent["out"], self.gen_tables, stream_id=23)
        if ent["P"]:
            o.pred_mark(req, ent["out"], tgt)
        if ent["drives"]:
            o.cond_partition(req, ent["out"], tgt, ent["dst"], any_value=True)
        else:
            o.cond_partition(req, ent["out"], tgt, ent["dst"])

    def _capture_cond(self, ent: dict, m: int):
        """Capture one conditional pass.  The warm-up sizes every lazily built table and scratch buffer; the RNG and the
        request's counters are put back after it, so a graph-replayed run starts from the state an eager run starts from."""
        req, ctr = ent["req"], self.ops.ctr

        def restore(ctr0):
            ctr.copy_(ctr0)
            req["filled"].zero_()
            req["stats"].zero_()
            if ent["P"]:
                req["pred_stats"].zero_()
        run = partial(self._cond_pass, ent, m)
        ent["graph"], = warm_and_capture(self.device, run, [run], snapshot=ctr.clone, restore=restore,
                                         mode=self.capture_mode)

    # ------------------------------------------------------------------ guarded generation
    @torch.no_grad()
    def generate_decoded_guarded(self, n: int, guard, request: dict | None = None, max_passes: int = 64,
                                 chunk: int | None = None, use_graph: bool | None = None) -> torch.Tensor:
        """Exactly n decoded rows none of which lies within the guard's radius of a real record: [n, n_cols] float64
        on the device.  ``guard``: eval/privacy.py PrivacyGuard on this engine's device; a generated row q is
        rejected iff some real row r has d2(q, r) <= guard.t2, with the privacy evaluator's d2.  Without ``request``
        the rows come in generation order (pass, then row); with one (models/conditional.py build_request) the table
        holds exactly the requested counts, grouped as generate_decoded_where groups them.

        One pass over m rows (``chunk``, default as generate_decoded_where): sample_gen -> cond_request (only with a
        request; else every row gets target 0) -> eval generator -> sample_decode -> nn_pack -> nn_within ->
        guard_mark (a row within the radius loses its target) -> cond_partition (without a request: one bin, no
        value compared).  Every row of every pass is tested.  Passes are issued in bursts with one readback per
        burst, captured once per (m, bins, fixed columns, guard) and replayed as in generate_decoded_where, the RNG
        counter and the counters restored after the warm-up, so eager and replayed runs from equal states give
        bit-identical tables.  max_passes passes without n rows raise ConditionalSamplingError (no table; the message
        carries the rejected share).  ``self.last_guard`` = {"passes", "generated", "rejected", "kept"}; with a
        request ``self.last_conditional`` is set as generate_decoded_where sets it.

        A request with range / set predicates runs pred_mark between the decode and the guard's steps (and
        pred_request in cond_request's place when a predicate drives).  The radius test still covers every row of the
        pass, so ``rejected`` counts every row within the radius, including rows a predicate had already rejected:
        it stays the guard's own rate over ``generated``, whatever the predicates let through."""
        from .conditional import ConditionalSamplingError
        if self.gen_tables is None:
            raise RuntimeError("set_generation_tables() first")
        n = int(n)
        n_cols = len(self.gen_tables["cols"])
        if guard.n_cols != n_cols or guard.t2.device != self.flat.device:
            raise ValueError(f"the guard holds {guard.n_cols}-column rows on {guard.t2.device}; the engine generates "
                             f"{n_cols}-column rows on {self.flat.device}")
        if request is not None:
            quotas = [int(q) for q in request["quotas"]]
            if n != int(request["n"]) or sum(quotas) != n:
                raise ValueError(f"the request was built for {request['n']} rows, not {n}")
            nb, nf, values = len(quotas), int(request["fixed_j"].numel()), list(request["values"])
            if nb > getattr(self.ops, "COND_MAX_BINS", 64):
                raise ValueError(f"{nb} requested values; the kernels' bin limit is {self.ops.COND_MAX_BINS}")
        else:
            if n < 0:
                raise ValueError("n must be non-negative")
            quotas, nb, nf, values = [n], 1, 0, []
        if n == 0:
            self.last_guard = {"passes": 0, "generated": 0, "rejected": 0, "kept": 0}
            if request is not None:
                self.last_conditional = {"passes": 0, "generated": 0, "kept": 0, "filled": [0] * nb, "values": values}
            return self._decoded(0)
        if use_graph is None:
            use_graph = self._graphs_for_generation()
        if chunk is not None:
            m = int(chunk)
            if m < 1:
                raise ValueError("chunk must be positive")
        else:
            m = min(int(self.cfg.gen_chunk), max(1024, 1 << int(np.ceil(np.log2(max(1.25 * n, 1.0))))))
        self._wait_gen_done()
        ent = self._guard_entry(m, nb, nf, n, guard, request is not None, self._pred_shape(request))
        req = ent["req"]
        if request is not None:
            for k in self._request_keys(ent):
                req[k].copy_(request[k])
        else:
            req["quota"].fill_(n)
        req["filled"].zero_()
        req["stats"].zero_()
        if ent["P"]:
            req["pred_stats"].zero_()
        ent["gstats"].zero_()
        if use_graph and ent.get("graph") is None:
            self._capture_guard(ent, m)

        def report(passes, filled):
            g = ent["gstats"].tolist()
            self.last_guard = {"passes": int(passes), "generated": int(g[0]), "rejected": int(g[1]),
                               "kept": int(sum(filled))}
            if request is not None:
                self.last_conditional = self._cond_report(ent, request, passes, filled)
        passes, filled = 0, [0] * nb
        while True:
            open_rows = sum(q - f for q, f in zip(quotas, filled))
            if open_rows <= 0:
                break
            if passes >= int(max_passes):
                report(passes, filled)
                if hasattr(self.ops, "check"):
                    self.ops.check()
                lg = self.last_guard
                share = lg["rejected"] / max(lg["generated"], 1)
                raise ConditionalSamplingError(
                    f"{passes} passes of {m} rows delivered {sum(filled)} of {n} rows; the guard (min_dcr "
                    f"{guard.min_dcr!r}) rejected {lg['rejected']} of {lg['generated']} generated rows "
                    f"({100.0 * share:.1f} %){self._worst_predicate(self.last_conditional if request else None)}",
                    filled, quotas, values)
            burst = max(1, min(-(-open_rows // m), int(max_passes) - passes))
            for _ in range(burst):
                if use_graph:
                    ent["graph"].replay()
                else:
                    self._guard_pass(ent, m)
            passes += burst
            filled = [int(x) for x in req["filled"].tolist()]     # the one readback per burst
        out = ent["dst"][:n].clone()
        report(passes, filled)
        if hasattr(self.ops, "check"):
            self.ops.check()
        return out

    def _guard_entry(self, m: int, nb: int, nf: int, n: int, guard, with_request: bool,
                     pshape: tuple = (0, 0, 0, False)) -> dict:
        """_cond_entry's buffers plus the guard's (packed pass, near, the search's scratch, its two counters), per
        (m, bins, fixed columns, request or not) of one guard: a captured pass reads the guard's tables, so another
        guard starts afresh."""
        dev = self.device
        if self._guard_ent and next(iter(self._guard_ent.values()))["guard"] is not guard:
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            self._guard_ent = {}
        pshape = tuple(pshape)
        key = (m, nb, nf, bool(with_request)) + (() if pshape == (0, 0, 0, False) else pshape)
        ent = self._guard_ent.get(key)
        if ent is None:
            H, lg, col, opt = self._gen_alloc(m, self.gen16)
            i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)      # noqa: E731
            i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)      # noqa: E731
            f64 = lambda k: torch.zeros(k, dtype=torch.float64, device=dev)    # noqa: E731
            ent = {"H": H, "lg": lg, "col": col, "opt": opt, "tgt": i32(m), "out": self._decoded(m),
                   "req": {"drive": i32(2), "bin_opt": i32(nb), "bin_code": f64(nb), "quota": i64(nb),
                           "filled": i64(nb), "seg_off": i64(nb), "fixed_j": i32(nf), "fixed_code": f64(nf),
                           "stats": i64(2)},
                   "guard": guard, "gbufs": guard.buffers(m), "gstats": i64(2), "request": bool(with_request),
                   "P": pshape[0], "drives": bool(pshape[3]), "dst": None, "graph": None}
            self._pred_buffers(ent["req"], pshape)
            self._guard_ent[key] = ent
        if ent["dst"] is None or ent["dst"].shape[0] < n:
            if ent["graph"] is not None:
                torch.cuda.synchronize(dev)
            ent["graph"] = None
            ent["dst"] = self._decoded(n)
        return ent

    def _guard_pass(self, ent: dict, m: int):
        o, req, guard = self.ops, ent["req"], ent["guard"]
        H, lg, col, opt, tgt = ent["H"], ent["lg"], ent["col"], ent["opt"], ent["tgt"]
        w16 = self._gen_weights16() if self.gen16 else None
        o.sample_gen(self.gen_cond, H, self.c_cols, self.z_cols, col_out=col, opt_out=opt, stream_id=21)
        if ent["drives"]:
            o.pred_request(req, col, opt, tgt, self.gen_cond, h=None if w16 is not None else H, c_col0=self.c_cols[0],
                           stream_id=25)
        elif ent["request"]:
            o.cond_request(req, col, opt, tgt, self.gen_cond, h=None if w16 is not None else H, c_col0=self.c_cols[0],
                           stream_id=24)
        else:
            tgt.zero_()         # every row aims at the one bin
        self._gen_forward(H, lg, col, opt, w16)
        o.sample_decode(lg, ent["out"], self.gen_tables, stream_id=23)
        if ent["P"]:
            o.pred_mark(req, ent["out"], tgt)
        guard.launch(ent["out"], *ent["gbufs"])
        o.guard_mark(ent["gbufs"][2], tgt, ent["gstats"])
        o.cond_partition(req, ent["out"], tgt, ent["dst"], any_value=ent["drives"] or not ent["request"])

    def _capture_guard(self, ent: dict, m: int):
        """Capture one guarded pass; the RNG counter, the request's and the guard's counters are put back after the
        warm-up (see _capture_cond)."""
        req, ctr = ent["req"], self.ops.ctr

        def restore(ctr0):
            ctr.copy_(ctr0)
            req["filled"].zero_()
            req["stats"].zero_()
            ent["gstats"].zero_()
            if ent["P"]:
                req["pred_stats"].zero_()
        run = partial(self._guard_pass, ent, m)
        ent["graph"], = warm_and_capture(self.device, run, [run], snapshot=ctr.clone, restore=restore,
                                         mode=self.capture_mode)

    # ------------------------------------------------------------------ completion of partial rows
    @torch.no_grad()
    def generate_decoded_known(self, known, mask, tries: int = 64, retries: int = 2, tol: float | None = None,
                               chunk: int | None = None, use_graph: bool | None = None) -> torch.Tensor:
        """The unknown cells of a known table: [N, n_cols] float64 on the device, row i carrying the known cells of
        input row i (their bits) and, in the others, the cells of the closest of the candidates generated for it.

        ``known`` [N, n_cols] float64 in the decoded space and ``mask`` [N, n_cols] (non-zero: the cell is known);
        models/known.py parse_known makes them from a frame or a CSV, build_known the per-row drivers.  One pass over
        m = q * tries rows (``chunk``: the rows of a pass, rounded down to a multiple of ``tries``) serves q rows of
        the table: sample_gen -> known_request (the rows of a slot take their query's condition) -> eval generator
        -> sample_decode -> known_match (each query keeps the lowest candidate with the smallest distance to its
        known cells, if strictly closer than its best so far).  Sweep 0 serves every row; up to ``retries`` further
        sweeps serve the rows that are still open -- a known category missed, or sqrt(dc) above ``tol`` (default:
        no bound, only categorical mismatches reopen) -- listed on the device in ascending order, with one readback
        (their count) per sweep.  Rows that stay open raise nothing: ``self.last_known`` says how many.

        On the HIP backend with cfg.gen_graph the pass is captured once per (m, tries) and replayed, the pass's
        queries copied into the static buffer before each replay; the RNG counter is restored after the warm-up, so
        eager and replayed runs from equal engine states give bit-identical tables and statistics.
        ``self.last_known``: rows, tries, sweeps, generated, open (after each sweep), exact_categorical (share of
        rows with no known category missed) and d_p50 / d_p95 / d_max of sqrt(dc)."""
        from .known import build_known
        if self.gen_tables is None:
            raise RuntimeError("set_generation_tables() first")
        R = int(tries)
        if not 1 <= R <= int(self.ops.KNOWN_MAX_TRIES):
            raise ValueError(f"tries must be 1..{self.ops.KNOWN_MAX_TRIES}, got {tries}")
        if int(retries) < 0:
            raise ValueError("retries must be non-negative")
        tol2 = float("inf") if tol is None else float(tol) * float(tol)
        if not tol2 >= 0:
            raise ValueError(f"tol must be a number >= 0, got {tol!r}")
        to_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)      # noqa: E731
        tab = build_known(self._known_transformer, self.gen_counts, to_np(known), to_np(mask))
        N = int(tab["known"].shape[0])
        if N == 0:
            self.last_known = {"rows": 0, "tries": R, "sweeps": 0, "generated": 0, "open": [],
                               "exact_categorical": 1.0, "d_p50": 0.0, "d_p95": 0.0, "d_max": 0.0}
            return self._decoded(0)
        if use_graph is None:
            use_graph = self._graphs_for_generation()
        if chunk is not None:
            if int(chunk) < 1:
                raise ValueError("chunk must be positive")
            q = max(1, int(chunk) // R)
        else:       # passes as large as the plain generation's, or one pass when the table needs fewer rows
            q = max(1, min(int(self.cfg.gen_chunk) // R, 1 << int(np.ceil(np.log2(N)))))
        m = q * R
        self._wait_gen_done()
        ent = self._known_entry(m, R, N)
        dev = self.device
        for k in ("known", "mask", "drv_span", "drv_opt"):
            ent[k][:N].copy_(torch.from_numpy(tab[k]).to(dev))
        ent["kind"].copy_(torch.from_numpy(tab["kind"]).to(dev))
        ent["scale"].copy_(torch.from_numpy(tab["scale"]).to(dev))
        st = ent["state"]
        st["best"].fill_(float("inf"))
        for k in ("dc", "miss", "seen", "pick"):
            st[k].zero_()
        ent["dst"].zero_()
        if use_graph and ent.get("graph") is None:
            self._capture_known(ent, m, R)
        todo = torch.arange(N, dtype=torch.int32, device=dev)
        opened, passes, sweeps = [], 0, 0
        while True:
            n_open = int(todo.numel())
            # the sweep's queries, padded with idle slots to whole passes: one copy per pass
            pad = torch.full((-(-n_open // q) * q,), -1, dtype=torch.int32, device=dev)
            pad[:n_open] = todo
            for a in range(0, int(pad.numel()), q):
                ent["qidx"].copy_(pad[a:a + q])
                if use_graph:
                    ent["graph"].replay()
                else:
                    self._known_pass(ent, m, R)
                passes += 1
            sweeps += 1
            todo = torch.nonzero((st["miss"][:N] > 0) | (st["dc"][:N] > tol2)).view(-1).to(torch.int32)
            opened.append(int(todo.numel()))          # the one readback per sweep
            if opened[-1] == 0 or sweeps > int(retries):
                break
        out = ent["dst"][:N].clone()
        d = torch.sqrt(st["dc"][:N]).cpu().numpy()
        self.last_known = {"rows": N, "tries": R, "sweeps": sweeps, "generated": passes * m, "open": opened,
                           "exact_categorical": float((st["miss"][:N] == 0).double().mean()),
                           "d_p50": float(np.percentile(d, 50)), "d_p95": float(np.percentile(d, 95)),
                           "d_max": float(d.max())}
        if hasattr(self.ops, "check"):
            self.ops.check()
        return out

    def _known_entry(self, m: int, R: int, N: int) -> dict:
        """Static buffers of a completion pass over m rows of ``R`` tries: the pass's activations / logits /
        conditions / decoded rows and its queries, and -- sized for the largest table seen (grown, and the graph
        dropped, when a table has more rows) -- the table, its drivers, the per-query state and the completed rows."""
        key = (m, R)
        ent = self._known_ent.get(key)
        dev = self.device
        n_cols = len(self.gen_tables["cols"])
        if ent is None:
            H, lg, col, opt = self._gen_alloc(m, self.gen16)
            ent = {"H": H, "lg": lg, "col": col, "opt": opt, "out": self._decoded(m),
                   "qidx": torch.full((m // R,), -1, dtype=torch.int32, device=dev),
                   "kind": torch.zeros(n_cols, dtype=torch.int32, device=dev),
                   "scale": torch.ones(n_cols, dtype=torch.float64, device=dev), "cap": 0, "graph": None}
            self._known_ent[key] = ent
        if ent["cap"] < N:
            if ent["graph"] is not None:
                torch.cuda.synchronize(dev)
            ent["graph"] = None
            z = lambda dt, *shape: torch.zeros(*shape, dtype=dt, device=dev)      # noqa: E731
            ent.update({"known": z(torch.float64, N, n_cols), "mask": z(torch.uint8, N, n_cols),
                        "drv_span": torch.full((N,), -1, dtype=torch.int32, device=dev),
                        "drv_opt": z(torch.int32, N), "dst": self._decoded(N),
                        "state": {"best": z(torch.float64, N), "dc": z(torch.float64, N), "miss": z(torch.int32, N),
                                  "seen": z(torch.int64, N), "pick": z(torch.int64, N)},
                        "cap": N})
        return ent

    def _known_pass(self, ent: dict, m: int, R: int):
        o = self.ops
        H, lg, col, opt = ent["H"], ent["lg"], ent["col"], ent["opt"]
        w16 = self._gen_weights16() if self.gen16 else None
        o.sample_gen(self.gen_cond, H, self.c_cols, self.z_cols, col_out=col, opt_out=opt, stream_id=21)
        o.known_request(ent["qidx"], ent["drv_span"], ent["drv_opt"], R, col, opt, self.gen_cond,
                        h=None if w16 is not None else H, c_col0=self.c_cols[0])
        self._gen_forward(H, lg, col, opt, w16)
        o.sample_decode(lg, ent["out"], self.gen_tables, stream_id=23)
        o.known_match(ent["known"], ent["mask"], ent["qidx"], R, ent["out"], ent["kind"], ent["scale"], ent["state"],
                      ent["dst"])

    def _capture_known(self, ent: dict, m: int, R: int):
        """Capture one completion pass.  The warm-up runs with every slot idle, so it writes no query's state; the RNG
        counter is put back after it (see _capture_cond)."""
        ctr = self.ops.ctr
        ent["qidx"].fill_(-1)
        run = partial(self._known_pass, ent, m, R)
        ent["graph"], = warm_and_capture(self.device, run, [run], snapshot=ctr.clone, restore=ctr.copy_,
                                         mode=self.capture_mode)

    # ------------------------------------------------------------------ pipelined generation
    def can_split_generation(self) -> bool:
        """generate_decoded_split applies: HIP bf16 generation with graphs."""
        return (self._graphs_for_generation() and self.gen16 and self.gen_tables is not None and
                getattr(self.ops, "batch_k", 1) == 1)

    def generate_decoded_split(self, n: int, gen_stream: "torch.cuda.Stream") -> torch.Tensor:
        """generate_decoded(n) in two parts, so the table of round r is generated while round r + 1 trains.

        The prep graph (on the current stream, ~10 us) copies everything the generation reads from the live model
        -- the bf16 / transposed weight copies of gen_weight_prep, each layer's bias, BatchNorm affine and running
        statistics, the output bias -- and snapshots the RNG step counter, advancing the live one by the body's
        bumps; the body graph (sampler, eval generator, decode) then runs on ``gen_stream`` reading only those
        copies.  The table is bit-identical to generate_decoded(n), and training's random numbers are unchanged
        (the live counter moves exactly as the unsplit pass would move it).  Returns a fresh tensor whose
        producer is ``gen_stream``."""
        self.generation_prep(n)
        return self.generation_body(n, gen_stream)

    def generation_prep(self, n: int) -> None:
        """The prep half of generate_decoded_split(n), on the current stream (see there)."""
        ent = self._gen_split.get(n) or self._capture_gen_split(n)
        self._wait_gen_done()
        ent.prep.replay()
        self._gen_prepped = torch.cuda.current_stream(self.device).record_event()

    def generation_body(self, n: int, gen_stream: "torch.cuda.Stream") -> torch.Tensor:
        """The body half, on ``gen_stream``: it waits for the prep (an event), not for whatever the current stream
        queued since -- the body of round r may be issued after round r + 1's training."""
        ent = self._gen_split[n]
        gen_stream.wait_event(self._gen_prepped)
        with torch.cuda.stream(gen_stream):
            ent.graph.replay()
            out = ent.out.clone()
            self._gen_done = gen_stream.record_event()
        if hasattr(self.ops, "check"):
            self.ops.check()
        return out

    def _gen_prep(self, n: int):
        """Copy what the body reads from the live model and snapshot the RNG counter, advancing the live one."""
        self._gen_weights16()
        if self._gsnap is None:
            names = [f"G.{i}.{k}" for i in range(len(self.gdims)) for k in ("b", "gamma", "beta", "rm", "rv")]
            names.append("G.out.b")
            self._gsnap = {nm: torch.empty_like(self.p[nm]) for nm in names}
            self._gsnap_pairs = ([self._gsnap[nm] for nm in names], [self.p[nm] for nm in names])
            self._gsnap_ctr = torch.zeros_like(self.ops.ctr)
        torch._foreach_copy_(*self._gsnap_pairs)
        self._gsnap_ctr.copy_(self.ops.ctr)
        for _ in range(-(-n // self.cfg.gen_chunk)):     # the body's decode bumps, once per chunk
            self.ops.L.rng_bump(self.ops.ctr)

    def _gen_body(self, n: int, out: torch.Tensor, bufs):
        """generate_decoded_split's body: the prepped weight copies, the parameter and RNG counter snapshots."""
        self._gen_chunks(n, out, bufs, (self._gw16, self._gwt), self._gsnap, self._gsnap_ctr)

    def _capture_gen_split(self, n: int) -> GenGraph:
        """Capture generate_decoded_split(n): the prep graph, then the body graph.  Nothing is restored: the warm-up
        (decode tables, lazy init) advances the RNG once."""
        ent = GenGraph(*self._gen_alloc(min(n, self.cfg.gen_chunk), True), self._decoded(n))
        prep, body = partial(self._gen_prep, n), partial(self._gen_body, n, ent.out, ent.rows)
        lane = self.ops.lane
        # the body runs beside training: its own split-K / scratch slots (ops lane 7), never the step's
        self.ops.lane = 7
        try:
            ent.prep, ent.graph = warm_and_capture(self.device, lambda: (prep(), body()), [prep, body],
                                                   mode=self.capture_mode)
        finally:
            self.ops.lane = lane
        self._gen_split[n] = ent
        return ent
