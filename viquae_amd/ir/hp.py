"""Mirror of ``meerqat.ir.hp``: the grid search of BM25's ``b`` and ``k1`` that maximises a rank metric (MRR) on a validation set,
then the search of a test set with the parameters found (EXPERIMENTS.rst, "BM25 (ViQuAE)"; meerqat/ir/hp.py:125-251).

    python -m viquae_amd.ir.hp bm25 <config> [--train=<dataset> --k=<k> --disable_caching --cleanup_cache_files
                                              --metrics=<path> --test=<dataset>]

The config is the reference's (experiments/ir/viquae/hp/bm25/config.json) after the BM25 migration: the text index says
``"kind": "BM25"`` where the shipped file says ``"es": true``; an unmigrated file stops with the Searcher's documented
error.  Exactly one BM25 index must exist among the KBs, and a searcher that fuses several indexes is refused, as in the reference.

What is the same: ``Objective`` / ``BM25Objective`` / ``get_objective`` / ``hyperparameter_search`` and their arguments, the search
space ``np.arange(*bounds, step)`` per parameter (default ``b``: bounds (0, 1), step 0.1; ``k1``: bounds (0, 3), step 0.1 -- 10 x 30
trials), the objective ``mrr@{k}`` maximised, relevance judged on the fly against the reference KB, the test-set files.
What differs:
  * the reference does not run as shipped (it imports names that no longer exist, reads an undefined ``eval_dataset`` and drives a
    live Elasticsearch through ``put_settings``): this module follows its documented intent;
  * there is no optuna.  The grid is enumerated ``b``-major, then ``k1`` (``grid_points``), every trial is run, and the study's
    ``best_params`` is the FIRST maximum in that order (optuna's GridSampler visits the grid in a shuffled order and
    ``study.best_trial`` is the first maximum it met: parity with it is UNPINNED, like the parity of BM25 itself with a live
    server).  Other samplers, optuna storage (``storage`` / ``study_name`` are accepted and ignored: no sqlite file, no resume) and
    fusion during the search stay out.  With ``metric_save_path`` the trial table is written to ``<path>/trials.json``;
  * all trials run at once: per ``map`` batch of questions the clauses are packed once and ``search_grid_device`` scores the whole
    grid, a tile of settings per sweep of the postings (csrc/bm25.hip); per question the union of the passages retrieved by any
    trial is judged once (the Searcher's ``qrels`` / ``qnonrels`` are the record); a trial's value is
    ``metrics.evaluate(qrels, its id table, metric)`` on the device.  The index's own parameters are not touched by the search;
  * ``hyperparameter_search`` returns the study (``best_params``, ``best_value``, ``trials``, ``report``, ``eval_dataset``), the
    reference returns the test dataset alone.
"""
import json
import warnings
from pathlib import Path

import numpy as np

from .runs import ArrayRun
from .search import IndexKind
from .searcher import Searcher, dataset_search

DEFAULT_HYP_HYP = {"b": {"bounds": (0, 1), "step": 0.1}, "k1": {"bounds": (0, 3), "step": 0.1}}


def parameter_values(hyp):
    """The values of one parameter: ``np.arange(*bounds, step)`` as the reference builds them, or an explicit ``values`` list."""
    if "values" in hyp:
        return [float(v) for v in hyp["values"]]
    return np.arange(*hyp["bounds"], hyp["step"]).tolist()


def search_space(hyp_hyp=None):
    hyp_hyp = DEFAULT_HYP_HYP if hyp_hyp is None else hyp_hyp
    return dict(b=parameter_values(hyp_hyp["b"]), k1=parameter_values(hyp_hyp["k1"]))


def grid_points(space):
    """The trials in grid order: ``b``-major, then ``k1`` -> [{"b": ..., "k1": ...}]."""
    return [{"b": b, "k1": k1} for b in space["b"] for k1 in space["k1"]]


def first_maximum(values, direction="maximize"):
    """Index of the best trial: the first one, in grid order, that no other trial beats."""
    if not len(values):
        raise ValueError("no trial was run")
    best = 0
    for i, v in enumerate(values):
        if (v > values[best]) if direction == "maximize" else (v < values[best]):
            best = i
    return best


class GridSampler:
    """Stands where ``optuna.samplers.GridSampler(search_space)`` does: the only sampler provided."""

    def __init__(self, search_space):
        self.search_space = {name: list(values) for name, values in search_space.items()}


class Study:
    """What the job reads of an ``optuna.Study``: ``trials`` ([{"b", "k1", "value"}] in grid order), ``best_params`` -- the
    FIRST maximum in grid order -- and ``best_value``."""

    def __init__(self, direction="maximize", sampler=None, study_name=None, storage=None):
        self.direction, self.sampler, self.study_name, self.storage = direction, sampler, study_name, storage
        self.trials = []
        self.report = self.eval_dataset = self.objective = None

    @property
    def best_trial(self):
        return self.trials[first_maximum([t["value"] for t in self.trials], self.direction)]

    @property
    def best_params(self):
        return {name: value for name, value in self.best_trial.items() if name != "value"}

    @property
    def best_value(self):
        return self.best_trial["value"]


class Objective:
    """
    Parameters
    ----------
    dataset: Dataset
        Used to optimize hyperparameters (None: no optimisation)
    metric_for_best_model: str, optional
        Defaults to "mrr@{self.searcher.k}" (e.g. "mrr@100")
    eval_dataset: Dataset, optional
        Searched after optimisation with the best parameters
    map_kwargs, fn_kwargs: dict, optional
        Passed to ``dataset.map``
    **searcher_kwargs:
        passed to Searcher
    """

    def __init__(self, dataset, metric_for_best_model=None, eval_dataset=None, map_kwargs={}, fn_kwargs={}, **searcher_kwargs):
        self.dataset = dataset
        self.searcher_kwargs = searcher_kwargs
        self.searcher = Searcher(**searcher_kwargs)
        self.metric_for_best_model = f"mrr@{self.searcher.k}" if metric_for_best_model is None else metric_for_best_model
        self.eval_dataset = eval_dataset
        self.map_kwargs = dict(map_kwargs)
        self.fn_kwargs = dict(fn_kwargs)

    def optimize(self, points):
        raise NotImplementedError

    def evaluate(self, best_params, metric_save_path=None):
        raise NotImplementedError


class BM25Objective(Objective):
    """
    Parameters
    ----------
    hyp_hyp: dict, optional
        Hyper-hyperparameters: per parameter the ``bounds`` and ``step`` of the grid (``np.arange(*bounds, step)``), or its
        ``values``.  Defaults to ``DEFAULT_HYP_HYP``.
    grid_method: str, optional
        Passed to ``MI355XBM25Index.search_grid`` as ``method`` (extra key).
    settings: dict, optional
        The reference fills it with the tried values for ``put_settings``; kept, and filled with the best parameters.
        Defaults to ``{'similarity': {'karpukhin': {'b': 0.75, 'k1': 1.2}}}``
    """

    def __init__(self, dataset, hyp_hyp=None, settings=None, grid_method=None, **kwargs):
        super().__init__(dataset, **kwargs)
        self.grid_method = grid_method  # "grid" | "loop" | None: MI355XBM25Index.search_grid's default
        self.hyp_hyp = DEFAULT_HYP_HYP if hyp_hyp is None else hyp_hyp
        self.settings = {"similarity": {"karpukhin": {"b": 0.75, "k1": 1.2}}} if settings is None else settings
        if self.searcher.do_fusion:
            raise NotImplementedError("fusion during the hyperparameter search is not provided (neither is it by the reference)")
        found = [(kb, name) for kb in self.searcher.kbs.values() for name, index in kb.indexes.items() if index.kind == IndexKind.BM25]
        if len(found) != 1:
            names = [name for _, name in found]
            raise ValueError(f"expected exactly one index of kind 'BM25' among the KBs, got {len(found)} {names}: the search "
                             "re-weights one text index (a shipped config's '\"es\": true' becomes '\"kind\": \"BM25\"')")
        self.kb, self.index_name = found[0]
        if self.kb.index_mapping is not None:
            raise NotImplementedError("the parameter grid searches a passage index directly: no index_mapping")
        self.index = self.kb.dataset._indexes[self.index_name]

    def optimize(self, points):
        """Every trial of ``points`` ([{"b", "k1"}]) over ``self.dataset`` -> their values, in order."""
        from .metrics import evaluate
        searcher, index, key, k = self.searcher, self.index, self.kb.indexes[self.index_name].key, self.searcher.k
        params = [(float(p["k1"]), float(p["b"])) for p in points]
        q_ids, id_blocks, score_blocks = [], [], []

        def run_batch(batch, **_):
            ids = list(batch["id"])
            queries = ["" if q is None else q for q in batch[key]]  # a missing question retrieves nothing
            # the clauses packed once, then search_grid_device over the whole grid, a tile of settings per sweep
            D, I = index.search_grid(queries, params, k, method=self.grid_method)
            q_ids.extend(ids)
            id_blocks.append(I)
            score_blocks.append(D)
            if searcher.reference_kb is None:
                return
            question_types = batch.get("question_type", ["String"] * len(ids))
            for row, (q_id, gt, question_type) in enumerate(zip(ids, batch["output"], question_types)):
                union = np.unique(I[:, row, :])
                searcher.judge(q_id, {str(i) for i in union[union >= 0].tolist()}, gt, question_type)

        needed = {"id", key} | ({"output", "question_type"} if searcher.reference_kb is not None else set())
        dataset = self.dataset.remove_columns([c for c in self.dataset.column_names if c not in needed])
        map_kwargs = dict(self.map_kwargs)
        if "new_fingerprint" not in map_kwargs:
            from datasets.fingerprint import generate_random_fingerprint
            map_kwargs["new_fingerprint"] = generate_random_fingerprint()
        dataset.map(run_batch, batched=True, fn_kwargs=self.fn_kwargs, **map_kwargs)
        if not q_ids:
            raise ValueError("the train dataset is empty")
        I, D = np.concatenate(id_blocks, axis=1), np.concatenate(score_blocks, axis=1)
        values = []
        for g in range(len(params)):
            run = ArrayRun()                         # the trial's [nq, k] id table, kept as an array
            run.add_block(q_ids, I[g], D[g])
            values.append(evaluate(searcher.qrels, run, self.metric_for_best_model, device=searcher.metric_device))
        return values

    def evaluate(self, best_params, metric_save_path=None):
        """Re-weight the resident index with ``best_params`` and run ``self.eval_dataset`` through the ordinary search job with fresh
        runs and qrels (``dataset_search`` over this objective's KBs: it writes qrels.json, metrics.json, metrics.tex and
        <index_name>.json under ``metric_save_path``) -> the report."""
        for parameters in self.settings["similarity"].values():
            parameters.update(best_params)
        self.index.set_bm25(k1=best_params["k1"], b=best_params["b"])
        kwargs = {name: value for name, value in self.searcher_kwargs.items() if name not in ("kbs", "reference_kb", "k", "qrels", "qnonrels")}
        if self.searcher.reference_kb is None:  # judged in advance: the files the searcher was given
            kwargs.update({name: self.searcher_kwargs[name] for name in ("qrels", "qnonrels") if name in self.searcher_kwargs})
        self.searcher = dataset_search(self.eval_dataset, k=self.searcher.k, metric_save_path=metric_save_path, map_kwargs=self.map_kwargs,
                                       kbs=self.searcher.kbs, reference_kb=self.searcher.reference_kb, **kwargs)
        return self.searcher.report


def get_objective(objective_type, train_dataset, **objective_kwargs):
    """-> (objective, default_study_kwargs): 'bm25' gives a ``BM25Objective`` and ``dict(direction='maximize',
    sampler=GridSampler(search_space))``, the grid of ``objective.hyp_hyp``."""
    if objective_type == "bm25":
        objective = BM25Objective(train_dataset, **objective_kwargs)
        default_study_kwargs = dict(direction="maximize", sampler=GridSampler(search_space(objective.hyp_hyp)))
    else:
        raise ValueError(f"Invalid objective type: {objective_type}")
    return objective, default_study_kwargs


def hyperparameter_search(study_name=None, storage=None, metric_save_path=None, optimize_kwargs={}, study_kwargs={},
                          cleanup_cache_files=False, **objective_kwargs):
    """Runs the grid over the train dataset (when there is one), prints and keeps the best trial -- the FIRST maximum in grid order,
    ``b``-major then ``k1`` -- and searches the test dataset (when there is one) with the best parameters; with no train dataset
    the test dataset is searched with the config's own parameters.  Returns the ``Study``.

    ``study_name`` / ``storage`` are accepted and ignored (no optuna storage); ``study_kwargs["sampler"]`` must be a
    ``GridSampler`` (or the name "GridSampler" with ``sampler_kwargs``): anything else is ``NotImplementedError``.
    ``metric_save_path``: where ``trials.json`` and the test set's qrels, runs and metrics go."""
    # the study's own arguments first: a sampler that is not provided must not cost an index build
    sampler = study_kwargs.get("sampler")
    if isinstance(sampler, str):
        if sampler != "GridSampler":
            raise NotImplementedError(f"sampler '{sampler}': only the grid is provided")
        sampler = GridSampler(**study_kwargs.get("sampler_kwargs", {}))
    if sampler is not None and not isinstance(sampler, GridSampler):
        raise NotImplementedError(f"sampler {type(sampler).__name__}: only the grid (viquae_amd.ir.hp.GridSampler) is provided")
    direction = study_kwargs.get("direction", "maximize")
    if direction not in ("maximize", "minimize"):
        raise ValueError(f"direction must be 'maximize' or 'minimize', got {direction!r}")
    objective, default_study_kwargs = get_objective(**objective_kwargs)
    if sampler is None:
        sampler = default_study_kwargs["sampler"]
    if optimize_kwargs:
        warnings.warn(f"hyperparameter_search: every trial of the grid is run, ignoring optimize_kwargs {sorted(optimize_kwargs)}")
    study = Study(direction=direction, sampler=sampler, study_name=study_name, storage=storage)
    print(f"Using a sampler of type {type(study.sampler)}")
    if metric_save_path is not None:
        metric_save_path = Path(metric_save_path)
        metric_save_path.mkdir(exist_ok=True)
    if objective.dataset is not None:
        points = grid_points(sampler.search_space)
        values = objective.optimize(points)
        study.trials = [dict(point, value=float(value)) for point, value in zip(points, values)]
        if cleanup_cache_files:
            objective.dataset.cleanup_cache_files()
        best_params = study.best_params
        print(f"Best value: {study.best_value} ({objective.metric_for_best_model})")
        print(f"Best hyperparameters: {best_params}")
        if metric_save_path is not None:
            with open(metric_save_path / "trials.json", "wt") as file:
                json.dump(study.trials, file)
    else:
        best_params = {"b": objective.index.b, "k1": objective.index.k1}
    # apply hyperparameters on test set
    if objective.eval_dataset is not None:
        study.report = objective.evaluate(best_params, metric_save_path)
        study.eval_dataset = objective.eval_dataset
    study.objective = objective
    return study


def main(objective_type, config_path, train=None, k=100, disable_caching=False, cleanup_cache_files=False, metrics=None, test=None):
    import datasets
    from datasets import load_from_disk
    if disable_caching:
        datasets.disable_caching()
    with open(config_path, "rt") as file:
        config = json.load(file)
    format_kwargs = config.pop("format", {})
    dataset = eval_dataset = None
    if train is not None:
        dataset = load_from_disk(train)
        dataset.set_format(**format_kwargs)
    if test is not None:
        eval_dataset = load_from_disk(test)
        eval_dataset.set_format(**format_kwargs)
    study = hyperparameter_search(objective_type=objective_type, train_dataset=dataset, k=int(k), metric_save_path=metrics,
                                  eval_dataset=eval_dataset, cleanup_cache_files=cleanup_cache_files, **config)
    if study.eval_dataset is not None:
        # the reference saves the test dataset back where it came from; `datasets` refuses to write a dataset over the files it is
        # read from, so it is written beside them and moved into place
        import shutil
        saving = str(test).rstrip("/") + ".saving"
        study.eval_dataset.save_to_disk(saving)
        shutil.rmtree(test)
        shutil.move(saving, test)
    return study


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="optimize hyperparameters of the ir.search pipeline (meerqat.ir.hp)")
    ap.add_argument("type", help="'bm25' to optimize BM25 hyperparameters")
    ap.add_argument("config", help="path to the JSON configuration file (passed as kwargs)")
    ap.add_argument("--train", help="train dataset (the grid runs over it)")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--disable_caching", action="store_true")
    ap.add_argument("--cleanup_cache_files", action="store_true")
    ap.add_argument("--metrics", help="where trials.json and the test set's metrics go")
    ap.add_argument("--test", help="test dataset (searched with the best parameters)")
    a = ap.parse_args()
    main(a.type, a.config, a.train, a.k, a.disable_caching, a.cleanup_cache_files, a.metrics, a.test)
