"""Federated privacy audit and guard of a running federation (FedConfig.privacy_every / min_dcr).

Every client keeps its records.  During initialisation it codes its own frame with the global meta and vocabularies,
the per-column extremes travel (``all_gather_object``), and it builds a :class:`ShardPrivacy` scaled with the combined
bounds.  From then on only per-generated-row scalars move:

* **audit** (rounds with ``(epoch + 1) % privacy_every == 0``): the federator broadcasts the round's table, every client
  searches its shard, the ``[n, 3]`` partials are gathered and merged on the federator (``nn_merge_shards`` ->
  ``nn_stats``).  Its own synchronous phase (``_sub("audit")``), outside the pipelined generation path;
* **guard** (after the last round, ``min_dcr``): the federator's ``generate_decoded_guarded`` runs with a guard whose
  ``launch`` is a collective -- the pass's decoded rows are broadcast, every client answers ``within``, the int32
  answers are gathered and folded (``nn_within_merge_shards``) into the pass's ``near``.

The results equal the pooled evaluator's / guard's on the concatenated shards bit for bit (eval/fed_privacy.py).  The
federator sees per-row distances and which client is nearest; nothing here is secure aggregation.
"""
from __future__ import annotations

import os
from typing import List, Optional

import numpy as np
import pandas as pd
import torch

from ..eval.fed_privacy import ShardPrivacy, merge_buffers, shard_offsets
from ..eval.privacy import code_real_table, combine_bounds, squared_radius, table_bounds


def privacy_on(cfg) -> bool:
    return int(getattr(cfg, "privacy_every", 0) or 0) > 0 or getattr(cfg, "min_dcr", None) is not None


def refuse_unsupported(cfg, comm=None) -> None:
    """Start-up refusals of the federated audit / guard, each naming the flag."""
    if not privacy_on(cfg):
        return
    which = "-privacy_every" if int(cfg.privacy_every or 0) > 0 else "-min_dcr"
    if int(cfg.privacy_every or 0) < 0:
        raise ValueError("-privacy_every must be >= 0")
    if cfg.min_dcr is not None:
        squared_radius(cfg.min_dcr)
    if cfg.mode == "mdgan":
        raise ValueError(f"{which}: the federated privacy audit / guard follows the FedAvg rounds; -mode mdgan has "
                         "no aggregated generator on the federator's rounds to audit")
    if cfg.batched_clients == "on":
        raise ValueError(f"{which}: not supported with -batched_clients on (the batched clients issue their work from "
                         "one thread); use -batched_clients off")
    if comm is not None and type(comm).__name__ == "HierComm":
        raise ValueError(f"{which}: not supported with -world_size N -local_clients K together; run one client per "
                         "process or every client in one process")


class _CollectiveGuard:
    """The guard ``generate_decoded_guarded`` drives on the federator: ``launch`` is one collective round trip."""

    def __init__(self, audit: "FedAudit", min_dcr: float):
        self.audit = audit
        rt = audit.rt
        self.device, self.ops = rt.device, rt.engine.ops
        self.n_cols = len(rt.global_meta["columns"])
        self.min_dcr = float(min_dcr)
        self.t2 = torch.tensor([squared_radius(min_dcr)], dtype=torch.float64, device=rt.engine.flat.device)
        self.k = rt.comm.n_clients

    def buffers(self, rows: int):
        dev = self.t2.device
        i32 = dict(dtype=torch.int32, device=dev)
        empty = torch.zeros(1, dtype=torch.float64, device=dev)
        return (empty, empty, torch.full((rows,), -1, **i32), empty, torch.full((rows,), -1, **i32))

    def launch(self, values: torch.Tensor, q_cont, q_cat, near, scratch, owner) -> None:
        a, c = self.audit, self.audit.rt.comm
        m = int(values.shape[0])
        c.broadcast_object(("pass", m), src=a.rt.federator)
        answers = a._within_round(values, m)
        self.ops.nn_within_merge_shards(answers, a.offsets, near[:m], owner[:m])


class FedAudit:
    def __init__(self, rt):
        """Collective over every rank, during initialisation (after the engine exists)."""
        self.rt = rt
        cfg, c = rt.cfg, rt.comm
        self.every = int(cfg.privacy_every or 0)
        self.min_dcr = cfg.min_dcr
        self.n_cols = len(rt.global_meta["columns"])
        self.guard_rows = int(cfg.guard_rows) if cfg.guard_rows else int(rt.n_sample)
        self.guard_chunk = min(int(cfg.engine.gen_chunk),
                               max(1024, 1 << int(np.ceil(np.log2(max(1.25 * self.guard_rows, 1.0))))))
        self.max_rows = max(int(rt.n_sample), self.guard_chunk if self.min_dcr is not None else 1)
        self.rows: List[dict] = []            # one record per audited epoch (federator)
        self.kept = None                      # FedConfig.keep_audit_table: (epoch, table, PrivacyScores)
        self.pending: List[int] = []          # due epochs whose table has not been audited yet (same on every rank)
        self._tables = {}                     # federator: epoch -> (table, event)
        dev = rt.device
        ops = rt.engine.ops
        coded = pair = None
        if rt.is_client:
            frame = getattr(rt, "_frame", None)
            coded = code_real_table(frame if frame is not None else rt._local_frame(), rt.global_meta, rt.vocabs)
            pair = (table_bounds(coded, rt.global_meta), int(coded.shape[0]))
        pairs = c.all_gather_object(pair)
        pairs = [pairs[r] for r in c.client_ranks]
        self.bounds = combine_bounds([p[0] for p in pairs])
        self.shard_rows = [p[1] for p in pairs]
        self.shard = None
        if rt.is_client:
            self.shard = ShardPrivacy(coded, rt.global_meta, rt.vocabs, dev, self.bounds, self.max_rows, ops=ops)
            self.t2 = torch.tensor([squared_radius(self.min_dcr or 0.0)], dtype=torch.float64, device=dev)
        self._recv = torch.zeros(self.max_rows, self.n_cols, dtype=torch.float64, device=dev)
        if rt.is_fed:
            self.offsets = shard_offsets(self.shard_rows, dev)
            self.buf = merge_buffers(ops, dev, self.max_rows, c.n_clients)
        # warm the kernels (code objects, first allocations) on a table of the real size, as _prepare_similarity does
        warm = self._recv[:int(rt.n_sample)]
        if self.shard is not None:
            self.shard.search(warm)
            self.shard.within(warm, self.t2)
        if rt.is_fed:
            k, n = c.n_clients, int(rt.n_sample)
            parts = torch.zeros(k, n, 3, dtype=torch.float64, device=dev)
            self.buf.merge(ops, parts, self.offsets, n)
            ops.nn_within_merge_shards(torch.full((k, n), -1, dtype=torch.int32, device=dev), self.offsets,
                                       self.buf.i1[:n], self.buf.owner[:n])
        if dev.type == "cuda":
            torch.cuda.current_stream(dev).synchronize()

    # ------------------------------------------------------------------ transport
    def _gather(self, mine: Optional[torch.Tensor], n: int, width: int, dtype) -> Optional[torch.Tensor]:
        """The clients' [n, width] answers stacked [K, n, width] on the federator's device, in client order."""
        rt = self.rt
        c = rt.comm
        k = c.n_clients
        dedicated = rt.federator not in c.client_ranks
        if mine is None:
            mine = torch.zeros(n, width, dtype=dtype, device=rt.device)
        if dedicated and c.dist_active and c.data_backend == "nccl":
            # the federator is outside the clients' RCCL group: the answers take the control plane
            got = c.all_gather_object(mine.cpu() if rt.is_client else None)
            if not rt.is_fed:
                return None
            return torch.stack([got[r] for r in c.client_ranks]).to(rt.device)
        out = c.gather_rows(mine, [n] * k, c.client_ranks, dst=rt.federator, to_host=False)
        if not rt.is_fed:
            return None
        return out.to(rt.device).view(k, n, width)

    def _table_round(self, table: Optional[torch.Tensor], n: int) -> torch.Tensor:
        """broadcast the federator's [n, n_cols] rows; returns them on this rank's device"""
        rt = self.rt
        buf = self._recv[:n]
        if rt.is_fed:
            buf.copy_(table)
        rt.comm.broadcast_tensor(buf, src=rt.federator)
        return buf

    def _within_round(self, values: Optional[torch.Tensor], m: int) -> Optional[torch.Tensor]:
        """one pass of the guard: rows out, every client's ``within`` back -> int32 [K, m] on the federator"""
        rows = self._table_round(values, m)
        mine = self.shard.within(rows, self.t2).view(m, 1) if self.shard is not None else None
        got = self._gather(mine, m, 1, torch.int32)
        return None if got is None else got.view(self.rt.comm.n_clients, m).contiguous()

    # ------------------------------------------------------------------ audit
    def due(self, epoch: int) -> bool:
        return self.every > 0 and (epoch + 1) % self.every == 0

    def keep(self, table, epoch: int) -> None:
        """Federator, where the round's table first exists (sample_round / _complete_handoff): hold a copy of a due
        table, ordered on the stream that produced it."""
        if not self.due(epoch) or table is None:
            return
        t = table if torch.is_tensor(table) else torch.from_numpy(table)
        t = t.to(self.rt.device, copy=True)
        ev = None
        if t.is_cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(t.device))
        self._tables[epoch] = (t, ev)

    def note_round(self, epoch: int, dumped: bool) -> None:
        """Every rank, after the round's sampling phase: audit what is due and exists."""
        if dumped and self.due(epoch):
            self.pending.append(epoch)
        self.drain()

    def drain(self) -> None:
        """Collective while an audit is pending: the federator names the epochs whose table exists (with a deferred
        hand-off the table of round r exists once round r + 1's training is queued)."""
        rt = self.rt
        if not self.pending:
            return
        ready = rt.comm.broadcast_object([e for e in self.pending if e in self._tables] if rt.is_fed else None,
                                         src=rt.federator)
        for epoch in ready:
            with rt._sub("audit"):
                self._audit(epoch)
            self.pending.remove(epoch)

    def _audit(self, epoch: int) -> None:
        rt = self.rt
        n = int(rt.n_sample)
        table = None
        if rt.is_fed:
            table, ev = self._tables.pop(epoch)
            if ev is not None:
                torch.cuda.current_stream(table.device).wait_event(ev)
            n = int(table.shape[0])
        n = int(rt.comm.broadcast_object(n, src=rt.federator))
        rows = self._table_round(table, n)
        mine = self.shard.search(rows) if self.shard is not None else None
        parts = self._gather(mine, n, 3, torch.float64)
        if not rt.is_fed:
            return
        ops = rt.engine.ops
        self.buf.merge(ops, parts.contiguous(), self.offsets, n)
        scores = self.buf.result(n)
        f = scores.floats()
        by = scores.by_client().cpu().tolist()
        rec = {"epoch": epoch, "dcr_p5": f["dcr_p5"], "nndr_p5": f["nndr_p5"], "dcr_min": f["dcr_min"],
               "copies": f["copies"], "nearest_by_client": by[0], "copies_by_client": by[1]}
        self.rows.append(rec)
        if rt.metrics is not None:
            rt.metrics.write(rec)
        if getattr(rt.cfg, "keep_audit_table", False):
            self.kept = (epoch, rows.clone(), scores)

    def write_online(self) -> Optional[str]:
        """{name}_result/privacy_online.csv (federator, after the last round)"""
        if self.every <= 0 or not self.rt.is_fed:
            return None
        path = os.path.join(self.rt.result_dir(), "privacy_online.csv")
        frame = pd.DataFrame([{"Epoch_No.": r["epoch"], "DCR_p5": r["dcr_p5"], "NNDR_p5": r["nndr_p5"],
                               "DCR_min": r["dcr_min"], "Copies": r["copies"],
                               "Nearest_by_client": " ".join(str(x) for x in r["nearest_by_client"]),
                               "Copies_by_client": " ".join(str(x) for x in r["copies_by_client"])}
                              for r in self.rows],
                             columns=["Epoch_No.", "DCR_p5", "NNDR_p5", "DCR_min", "Copies", "Nearest_by_client",
                                      "Copies_by_client"])
        frame.to_csv(path, index=False)
        return path

    # ------------------------------------------------------------------ guard
    def guarded_table(self) -> Optional[str]:
        """Collective after the last round: the federator generates ``guard_rows`` rows none of which lies within
        ``min_dcr`` of any client's record and writes {name}_result/{name}_guarded.csv; the clients answer its passes
        until it says "done" (also when it gives up: the message is sent in a ``finally``)."""
        if self.min_dcr is None:
            return None
        rt = self.rt
        c = rt.comm
        if not rt.is_fed:
            while True:
                msg = c.broadcast_object(None, src=rt.federator)
                if msg == "done":
                    return None
                self._within_round(None, int(msg[1]))
        from .runtime import _log
        guard = _CollectiveGuard(self, self.min_dcr)
        try:
            tab = rt.engine.generate_decoded_guarded(self.guard_rows, guard, max_passes=int(rt.cfg.guard_max_passes),
                                                     chunk=self.guard_chunk, use_graph=False)
        finally:
            c.broadcast_object("done", src=rt.federator)
        lg = rt.engine.last_guard
        self.last_guard = dict(lg)
        if getattr(rt.cfg, "keep_audit_table", False):
            self.kept_guarded = tab
        path = os.path.join(rt.result_dir(), f"{rt.name}_guarded.csv")
        rt._write_epoch_csv_body(tab.cpu().numpy(), -1, path=path)
        _log(rt.cfg, rt.rank, f"[guard] min_dcr {self.min_dcr!r}: {lg['passes']} passes, {lg['rejected']} of "
                              f"{lg['generated']} generated rows rejected -> {path}")
        return path
