"""Export the trained (aggregated) generator and sample from it later, without the federation.

The reference's federator has a ``save_model`` that pickles ``[generator, cond, transformer,
batch_size, embedding_dim]`` (`Server/dtds/distributed.py:560-563`), but nothing calls it and the
pickle needs the reference classes to load.  Here the federator writes ONE self-contained file after
the last round (``models/{name}_generator.pt``):

* the flat G / D / BN buffer and the engine configuration,
* the fitted VGM transformer (plain dict: meta, VGM posteriors, valid modes),
* the global span counts of the generation-time conditional sampler,
* the merged table meta and the label vocabularies (for the CSV decode).

Everything is tensors, lists, strings and numbers, so it loads with
``torch.load(..., weights_only=True)`` (no unpickling of code).  ``python -m dtds.sample`` then
regenerates any number of rows on the GPU (HIP engine, eval-mode BN, Gumbel-argmax decode) or the
CPU, and writes the same CSV as the per-epoch dumps.
"""
from __future__ import annotations

import dataclasses
import json
from typing import Optional

import numpy as np
import torch

from ..data.decode import csv_layout, decode_frame
from ..data.vocab import CategoryVocab
from ..features.transformer import VGMTransformer
from .engine import CTGANEngine, EngineConfig
from .samplers import CondTables

FORMAT = "fed_tgan_amd.generator/1"


def export_generator(path: str, engine: CTGANEngine, transformer: VGMTransformer, gen_cond: CondTables,
                     meta: dict, vocabs, name: str) -> str:
    cfg = dataclasses.asdict(engine.cfg)
    state = {
        "format": FORMAT,
        "name": name,
        "engine_cfg": json.dumps(cfg),
        "flat": engine.flat.detach().cpu().clone(),
        "bn_batches": int(engine.bn_batches),
        "transformer": json.dumps(transformer.to_dict()),
        "span_counts": torch.as_tensor(np.asarray(gen_cond.counts, dtype=np.float64)),
        "meta": json.dumps(meta, default=lambda o: o.item() if hasattr(o, "item") else str(o)),
        "vocabs": [[v.column_name, list(v.tolist())] for v in vocabs],
    }
    torch.save(state, path)
    return path


@dataclasses.dataclass
class LoadedGenerator:
    name: str
    engine: CTGANEngine
    transformer: VGMTransformer
    meta: dict
    vocabs: list
    _evaluators: dict = dataclasses.field(default_factory=dict, repr=False)   # kind -> (key, real frames, evaluator)

    def sample(self, n: int, where=None, max_passes: int = 64, min_dcr=None, guard_real=None) -> np.ndarray:
        """[n, n_columns] decoded values (label codes for categoricals), float64.  A GPU table comes
        back through pinned host memory (torch's caching host allocator): 1M rows in ~9 ms instead
        of ~54 ms for a pageable copy.

        where ({column name: value | {value: weight}}, models/conditional.py): exactly n rows carrying the
        requested category values, grouped by the weighted column's values in request order; raises
        ConditionalSamplingError when max_passes generation passes do not fill the request.  A categorical column
        also takes a list of values (any of them, in the model's own proportions) and a continuous one
        {"min": a, "max": b} in the units the CSV prints (either key may be absent; inclusive, enforced on the decoded
        value); when such an entry comes first and no column carries weights it drives, and the rows come back in
        generation order.

        min_dcr (a float >= 0) with guard_real (the real table: a DataFrame or a CSV path): the privacy guard
        (eval/privacy.py PrivacyGuard) -- no returned row lies within distance min_dcr of a real record, in the
        privacy evaluator's metric; 0 keeps out exact copies.  Still exactly n rows, in generation order (with where:
        the requested counts, grouped as above).  The real records have to be on this machine."""
        return self._to_host(self.device_table(n, where=where, max_passes=max_passes, min_dcr=min_dcr,
                                               guard_real=guard_real))

    @staticmethod
    def _to_host(vals: torch.Tensor) -> np.ndarray:
        if not vals.is_cuda:
            return vals.numpy()
        host = torch.empty(vals.shape, dtype=vals.dtype, pin_memory=True)
        host.copy_(vals, non_blocking=True)
        torch.cuda.current_stream(vals.device).synchronize()
        return host.numpy()

    def write_csv(self, path: str, n: Optional[int] = None, threads: int = 0, where=None, max_passes: int = 64,
                  min_dcr=None, guard_real=None, known=None, tries: int = 64, retries: int = 2, tol=None) -> str:
        """``n`` generated rows as a CSV; with ``known`` (a partial table, :meth:`complete`) its completed rows
        instead, in its row order (``n``, ``where`` and the guard do not combine with it)."""
        if known is not None:
            if where or min_dcr is not None or guard_real is not None:
                raise ValueError("known does not combine with where, min_dcr or guard_real")
            return self._write_values(path, self.complete(known, tries=tries, retries=retries, tol=tol), threads)
        if n is None:
            raise ValueError("write_csv needs the number of rows n (or a partial table: known=)")
        if min_dcr is not None:
            vals = self.sample(n, where=where or None, max_passes=max_passes, min_dcr=min_dcr, guard_real=guard_real)
        else:
            vals = self.sample(n, where=where, max_passes=max_passes) if where else self.sample(n)
        return self._write_values(path, vals, threads)

    def _known_arrays(self, known):
        """(known, mask) of a partial table: a DataFrame or a CSV path (models/known.py parse_known), or the pair
        of arrays itself."""
        if isinstance(known, tuple) and len(known) == 2:
            return known
        from .known import parse_known
        return parse_known(known, self.meta, self.vocabs, self.transformer)

    def complete(self, known, tries: int = 64, retries: int = 2, tol=None) -> np.ndarray:
        """The unknown cells of a partial table filled in: [N, n_columns] decoded values, float64, one row per input
        row in the input's order.  ``known``: a DataFrame or a CSV path whose blank cells are the holes (columns by
        name; models/known.py parse_known), or a pair (known float64 [N, n_columns] in the decoded space, mask).
        Every row's known cells come back as given; its other cells are those of the closest of ``tries`` rows
        generated under the row's own condition, so the row is an approximation of "a row of the model with these
        cells", and how close it got is in ``engine.last_known`` (``exact_categorical``, ``d_p50`` / ``d_p95`` /
        ``d_max``).  Rows that miss a known category (or, with ``tol``, lie farther than it) get up to ``retries``
        further rounds of candidates."""
        k, m = self._known_arrays(known)
        return self._to_host(self.engine.generate_decoded_known(k, m, tries=tries, retries=retries, tol=tol))

    def complete_frame(self, known, tries: int = 64, retries: int = 2, tol=None):
        """:meth:`complete` as a DataFrame in the CSV's value space (labels, expm1 of the non-negative columns), with
        the caller's own known cells spliced back verbatim."""
        import pandas as pd
        k, m = self._known_arrays(known)
        vals = self._to_host(self.engine.generate_decoded_known(k, m, tries=tries, retries=retries, tol=tol))
        out = decode_frame(vals, self.meta, self.vocabs)
        if isinstance(known, tuple):
            return out
        src = known if isinstance(known, pd.DataFrame) else pd.read_csv(known, dtype=str, keep_default_na=False)
        names = [c["column_name"] for c in self.meta["columns"]]
        for j, name in enumerate(names):
            if name in src.columns and name in out.columns and bool(np.asarray(m)[:, j].any()):
                on = np.asarray(m)[:, j] != 0
                col = out[name].astype(object)
                col[on] = src[name].to_numpy(dtype=object)[on]
                out[name] = col
        return out

    def _write_values(self, path: str, vals: np.ndarray, threads: int = 0) -> str:
        lay = csv_layout(self.meta, self.vocabs)
        if lay is not None:
            from ..utils import csvio
            if csvio.available():
                csvio.write_layout(path, vals, lay, threads=threads)
                return path
        decode_frame(vals, self.meta, self.vocabs).to_csv(path, index=False)
        return path

    def score(self, real, n: int = 40000, where=None, max_passes: int = 64):
        """(Avg_JSD, Avg_WD) of n generated rows against ``real`` (a DataFrame or a CSV path), as
        ``eval.similarity.stat_sim`` gives them for the written CSV: generated and scored on the engine's device
        (eval/device.py), only the two numbers come back.  The evaluator is kept per real table and n."""
        return self._evaluator(real, n).score(self.device_table(n, where=where, max_passes=max_passes)).floats()

    def write_csv_scored(self, path: str, n: int, real, threads: int = 0, where=None, max_passes: int = 64):
        """:meth:`write_csv` and :meth:`score` of the same n rows: the table is scored on the device while it is
        still there, then copied and written.  Returns (Avg_JSD, Avg_WD)."""
        return self.write_csv_evaluated(path, n, score_real=real, threads=threads, where=where,
                                        max_passes=max_passes)[0]

    def write_csv_evaluated(self, path: str, n: int, score_real=None, privacy_real=None, threads: int = 0, where=None,
                            max_passes: int = 64):
        """:meth:`write_csv` with :meth:`score` (score_real) and / or :meth:`privacy` (privacy_real) of the rows the
        CSV holds, both taken on the device before the copy.  Returns ((Avg_JSD, Avg_WD) | None, privacy dict | None)."""
        return self.write_csv_all(path, n, score_real=score_real, privacy_real=privacy_real, threads=threads,
                                  where=where, max_passes=max_passes)[:2]

    def write_csv_all(self, path: str, n: int, score_real=None, privacy_real=None, corr_real=None, threads: int = 0,
                      where=None, max_passes: int = 64, utility_real=None, utility_test=None, utility_iters: int = 200,
                      utility_models=("lr",), utility_trees: int = 100, utility_depth: int = 12,
                      utility_hidden: int = 100, utility_steps: int = 1000, utility_batch: int = 512, min_dcr=None,
                      guard_real=None, fidelity_real=None, fidelity_k: int = 5):
        """:meth:`write_csv` with whichever of :meth:`score` (score_real), :meth:`privacy` (privacy_real),
        :meth:`correlation` (corr_real) and :meth:`utility` (utility_real, utility_test) are asked for, all of the
        rows the CSV holds and all taken on the device before the copy.  utility_models: ``"lr"`` (:meth:`utility`)
        and / or ``"dt"`` / ``"rf"`` (:meth:`tree_utility`, with utility_trees and utility_depth) and / or ``"mlp"``
        (:meth:`mlp_utility`, with utility_hidden, utility_steps and utility_batch), whose keys share the utility dict
        in that order.  min_dcr: the privacy guard of :meth:`sample`, against guard_real or, by default, privacy_real
        (whose ``copies`` is then 0).  Returns ((Avg_JSD, Avg_WD) | None, privacy dict | None, correlation dict | None, utility
        dict | None).  With fidelity_real (and fidelity_k) the dict of :meth:`fidelity` for the same rows is appended
        as a fifth element; without it the return value is the 4-tuple."""
        utility_models = tuple(utility_models)
        if not utility_models or set(utility_models) - {"lr", "dt", "rf", "mlp"}:
            raise ValueError("utility_models must be a non-empty subset of ('lr', 'dt', 'rf', 'mlp'), got "
                             f"{utility_models}")
        if min_dcr is not None and guard_real is None:
            guard_real = privacy_real
        vals = self.device_table(n, where=where, max_passes=max_passes, min_dcr=min_dcr, guard_real=guard_real)
        sim = self._evaluator(score_real, n).score(vals) if score_real is not None else None
        priv = self._privacy_evaluator(privacy_real, n).score(vals) if privacy_real is not None else None
        corr = self._correlation_evaluator(corr_real, n).score(vals) if corr_real is not None else None
        fid = self._fidelity_evaluator(fidelity_real, n, fidelity_k).score(vals) if fidelity_real is not None else None
        util = forest = mlp = None
        if utility_real is not None and "lr" in utility_models:
            util = self._utility_evaluator(utility_real, utility_test, n, utility_iters).score(vals)
        tree_models = tuple(m for m in ("dt", "rf") if m in utility_models)
        if utility_real is not None and tree_models:
            forest = self._forest_evaluator(utility_real, utility_test, n, utility_trees, utility_depth, 0,
                                            tree_models).score(vals)
        if utility_real is not None and "mlp" in utility_models:
            mlp = self._mlp_evaluator(utility_real, utility_test, n, utility_hidden, utility_steps,
                                      utility_batch).score(vals)
        self._write_values(path, self._to_host(vals), threads)
        out = [s.floats() if s is not None else None for s in (sim, priv, corr, util)]
        for more in (forest, mlp):
            if more is not None:
                out[3] = dict(out[3] or {}, **more.floats())
        if fid is not None:
            out.append(fid.floats())
        return tuple(out)

    def utility(self, train_real, test_real=None, n: int = 40000, where=None, max_passes: int = 64,
                iters: int = 200) -> dict:
        """ML utility of n generated rows (eval/utility_device.py): a class-balanced logistic regression is fitted
        on them on the engine's device and tested on real rows; ``f1_fake`` / ``acc_fake`` against ``f1_real`` /
        ``acc_real`` of the same fit on ``train_real``, their gaps, and ``loss_fake`` / ``grad_fake`` of the fit.
        The tables are DataFrames or CSV paths; without ``test_real`` the rows of ``train_real`` with ``index % 5
        == 4`` are held out and the rest are the training rows.  The evaluator is kept per tables, n and iters."""
        return self._utility_evaluator(train_real, test_real, n, iters).score(
            self.device_table(n, where=where, max_passes=max_passes)).floats()

    def _utility_evaluator(self, train_real, test_real, n: int, iters: int = 200):
        from ..eval.utility_device import DeviceUtility
        return self._cached("utility", (train_real, test_real), (int(n), int(iters)), lambda train, test: DeviceUtility(
            *self._held_out(train, test), self.meta, self.vocabs, self.engine.device, ops=self.engine.ops,
            iters=int(iters), max_rows=int(n)))

    def tree_utility(self, train_real, test_real=None, n: int = 40000, where=None, trees: int = 100,
                     max_depth: int = 12, seed: int = 0, max_passes: int = 64) -> dict:
        """Tree utility of n generated rows (eval/forest_device.py): a histogram decision tree and a random forest of
        ``trees`` trees, both of depth ``max_depth`` at most and with balanced class weights, are fitted on them on
        the engine's device and tested on real rows; ``dt_*`` / ``rf_*`` ``f1_fake`` / ``acc_fake`` against ``f1_real``
        / ``acc_real`` of the same fits on ``train_real``, and their gaps.  Tables and the held-out default as for
        :meth:`utility`.  The evaluator is kept per tables, n, trees, max_depth and seed."""
        return self._forest_evaluator(train_real, test_real, n, trees, max_depth, seed).score(
            self.device_table(n, where=where, max_passes=max_passes)).floats()

    def _forest_evaluator(self, train_real, test_real, n: int, trees: int = 100, max_depth: int = 12, seed: int = 0,
                          models=("dt", "rf")):
        from ..eval.forest_device import DeviceForest
        params = (int(n), int(trees), int(max_depth), int(seed), tuple(models))
        return self._cached("forest", (train_real, test_real), params, lambda train, test: DeviceForest(
            *self._held_out(train, test), self.meta, self.vocabs, self.engine.device, ops=self.engine.ops,
            trees=int(trees), max_depth=int(max_depth), seed=int(seed), max_rows=int(n), models=tuple(models)))

    def mlp_utility(self, train_real, test_real=None, n: int = 40000, where=None, hidden: int = 100,
                    steps: int = 1000, batch: int = 512, seed: int = 0, max_passes: int = 64) -> dict:
        """MLP utility of n generated rows (eval/mlp_device.py): a network of one hidden layer of ``hidden`` units is
        trained on them on the engine's device by ``steps`` Adam steps over strided batches of ``batch`` rows and
        tested on real rows; ``mlp_f1_fake`` / ``mlp_acc_fake`` against ``mlp_f1_real`` / ``mlp_acc_real`` of the
        same fit on ``train_real``, their gaps, and ``mlp_loss_fake`` of the fit.  Tables and the held-out default as
        for :meth:`utility`.  The evaluator is kept per tables, n, hidden, steps, batch and seed."""
        return self._mlp_evaluator(train_real, test_real, n, hidden, steps, batch, seed).score(
            self.device_table(n, where=where, max_passes=max_passes)).floats()

    def _mlp_evaluator(self, train_real, test_real, n: int, hidden: int = 100, steps: int = 1000, batch: int = 512,
                       seed: int = 0):
        from ..eval.mlp_device import DeviceMLP
        params = (int(n), int(hidden), int(steps), int(batch), int(seed))
        return self._cached("mlp", (train_real, test_real), params, lambda train, test: DeviceMLP(
            *self._held_out(train, test), self.meta, self.vocabs, self.engine.device, ops=self.engine.ops,
            hidden=int(hidden), steps=int(steps), batch=int(batch), seed=int(seed), max_rows=int(n)))

    def correlation(self, real, n: int = 40000, where=None, max_passes: int = 64) -> dict:
        """Diff. Corr. of n generated rows against ``real`` (a DataFrame or a CSV path): generated and scored on the
        engine's device (eval/correlation.py), only the four numbers come back: ``corr_diff`` (the Frobenius
        distance between the two tables' association matrices), ``corr_mean_abs`` / ``corr_max_abs`` over the column
        pairs, and the real table's own even / odd row ``corr_diff_rr`` as the baseline.  The evaluator is kept per
        real table and n."""
        return self._correlation_evaluator(real, n).score(
            self.device_table(n, where=where, max_passes=max_passes)).floats()

    def _correlation_evaluator(self, real, n: int):
        from ..eval.correlation import DeviceCorrelation
        return self._table_evaluator("correlation", DeviceCorrelation, real, n)

    def fidelity(self, real, n: int = 40000, where=None, max_passes: int = 64, k: int = 5) -> dict:
        """Precision / recall / density / coverage of n generated rows against ``real`` (a DataFrame or a CSV path):
        generated and scored on the engine's device (eval/fidelity.py), only the eight numbers come back:
        ``precision`` / ``density`` (are the generated rows inside the real rows' k-nearest-neighbour balls),
        ``recall`` / ``coverage`` (is every real row reached), and the real table's own even / odd row
        ``precision_rr`` / ``recall_rr`` / ``density_rr`` / ``coverage_rr`` as the baseline, at half the table's
        size.  The evaluator is kept per real table, n and k."""
        return self._fidelity_evaluator(real, n, k).score(
            self.device_table(n, where=where, max_passes=max_passes)).floats()

    def _fidelity_evaluator(self, real, n: int, k: int = 5):
        from ..eval.fidelity import DeviceFidelity
        return self._cached("fidelity", (real,), (int(n), int(k)), lambda frame: DeviceFidelity(
            frame, self.meta, self.vocabs, self.engine.device, ops=self.engine.ops, k=int(k), max_rows=int(n)))

    def privacy(self, real, n: int = 40000, where=None, max_passes: int = 64) -> dict:
        """DCR / NNDR of n generated rows against ``real`` (a DataFrame or a CSV path): generated and scored on the
        engine's device (eval/privacy.py), only the six numbers come back: the 5th percentiles ``dcr_p5`` /
        ``nndr_p5``, ``dcr_min``, the share of exact ``copies``, and the real table's own ``dcr_rr_p5`` /
        ``nndr_rr_p5`` as the baseline.  The evaluator is kept per real table and n."""
        return self._privacy_evaluator(real, n).score(self.device_table(n, where=where, max_passes=max_passes)).floats()

    def _privacy_evaluator(self, real, n: int):
        from ..eval.privacy import DevicePrivacy
        return self._table_evaluator("privacy", DevicePrivacy, real, n)

    def _evaluator(self, real, n: int):
        from ..eval.device import DeviceSimilarity
        return self._table_evaluator("similarity", DeviceSimilarity, real, n)

    def _table_evaluator(self, kind: str, cls, real, n: int):
        return self._cached(kind, (real,), (int(n),), lambda frame: cls(
            frame, self.meta, self.vocabs, self.engine.device, ops=self.engine.ops, max_rows=int(n)))

    def _cached(self, kind: str, tables, params: tuple, build):
        """The evaluator of ``kind`` for these real tables (DataFrames, CSV paths or None) and parameters: the one
        kept from the last call if they are the same, else ``build(*frames)``, which replaces it."""
        key = tuple(t if isinstance(t, str) or t is None else id(t) for t in tables) + params
        entry = self._evaluators.get(kind)
        if entry is None or entry[0] != key:
            import pandas as pd
            frames = tuple(pd.read_csv(t) if isinstance(t, str) else t for t in tables)
            self._evaluators.pop(kind, None)         # (its buffers go before the new one's are allocated)
            # (the frames are kept with their evaluator, so their ids stay their own while the entry lives)
            self._evaluators[kind] = entry = (key, frames, build(*frames))
        return entry[2]

    @staticmethod
    def _held_out(train, test):
        """without test rows, the rows of ``train`` with ``index % 5 == 4`` are held out and the rest train"""
        if test is not None:
            return train, test
        held = np.arange(len(train)) % 5 == 4
        return train[~held].reset_index(drop=True), train[held].reset_index(drop=True)

    def _guard(self, real, min_dcr):
        """The PrivacyGuard of radius min_dcr around ``real`` (kept per real table; a new radius shares its packed
        table)."""
        from ..eval.privacy import PrivacyGuard, squared_radius
        squared_radius(min_dcr)
        if real is None:
            raise ValueError("min_dcr needs the real table to guard against (guard_real)")
        dev = self.engine.device
        base = self._cached("guard", (real,), (), lambda frame: PrivacyGuard(
            frame, self.meta, self.vocabs, dev, min_dcr=min_dcr, ops=self.engine.ops))
        if base.min_dcr != float(min_dcr):
            base.min_dcr = float(min_dcr)
            base.t2.fill_(squared_radius(min_dcr))       # (a captured pass reads t2 from the device)
        return base

    def device_table(self, n: int, where=None, max_passes: int = 64, min_dcr=None, guard_real=None) -> torch.Tensor:
        """:meth:`sample`'s table where the engine left it: [n, n_columns] float64 on the engine's device"""
        if min_dcr is not None:
            guard = self._guard(guard_real, min_dcr)
            req = None
            if where:
                from .conditional import build_request
                req = build_request(self.transformer, self.meta, self.vocabs, where, int(n), self.engine.device,
                                    counts=self.engine.gen_counts)
            return self.engine.generate_decoded_guarded(int(n), guard, request=req, max_passes=max_passes)
        if guard_real is not None:
            raise ValueError("guard_real without min_dcr: give the radius (0 keeps out exact copies)")
        if where:
            from .conditional import build_request
            req = build_request(self.transformer, self.meta, self.vocabs, where, int(n), self.engine.device,
                                    counts=self.engine.gen_counts)
            return self.engine.generate_decoded_where(int(n), req, max_passes=max_passes)
        return self.engine.generate_decoded(int(n))


def load_generator(path: str, device: Optional[torch.device] = None, backend: str = "auto",
                   seed: int = 0) -> LoadedGenerator:
    st = torch.load(path, map_location="cpu", weights_only=True)
    if st.get("format") != FORMAT:
        raise ValueError(f"{path}: not a {FORMAT} file")
    device = device or (torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu"))
    cfg = json.loads(st["engine_cfg"])
    cfg = {k: tuple(v) if isinstance(v, list) else v for k, v in cfg.items()}
    cfg.setdefault("g_wt", False)     # files written before input-major generator storage existed
    ecfg = EngineConfig(**cfg)
    tr = VGMTransformer.from_dict(json.loads(st["transformer"]))
    eng = CTGANEngine(tr.layout, ecfg, device, backend=backend, seed=seed)
    eng.flat.copy_(st["flat"].to(device))
    eng.bn_batches = int(st["bn_batches"])
    eng.set_generation_tables(CondTables(tr.layout, st["span_counts"].numpy()), tr)
    vocabs = [CategoryVocab(lst, name) for name, lst in st["vocabs"]]
    return LoadedGenerator(st["name"], eng, tr, json.loads(st["meta"]), vocabs)
