"""GPU, end to end: the BM25 parameter search (viquae_amd/ir/hp.py) with the shipped hp config (tests/golden/config_surface.json,
experiments/ir/viquae/hp/bm25/config.json) after the documented migration -- in memory only, ``"es": true`` replaced by ``"kind":
"BM25"`` -- over the planted world of tests/bm25_hp_world.py, in which the length normalisation decides the rank of the only relevant
passage: 12 trials, 7 distinct values of mrr@10, the maximum reached twice (tests/test_bm25_grid_cpu.py checks all this on the
restatement).  The trial table must equal, value for value, the per-trial loop ``set_bm25`` + ``dataset_search`` +
``metrics.evaluate``; the test-split files must be those ``dataset_search`` writes at the best parameters."""
import copy
import json

import pytest

from tests import bm25_hp_world as world
from tests import config_surface as cs

pytestmark = pytest.mark.gpu

HP_CONFIG = "experiments/ir/viquae/hp/bm25/config.json"


def _migrated():
    config = copy.deepcopy(cs.configs()[HP_CONFIG])
    changed = 0
    for kb in config["kb_kwargs"].values():
        for ix in kb.get("index_kwargs", {}).values():
            if ix.get("es"):
                del ix["es"]
                ix["kind"] = "BM25"
                ix["load"] = False
                changed += 1
    assert changed == 1
    return config


@pytest.fixture()
def job(tmp_path, monkeypatch):
    import datasets
    datasets.disable_progress_bars()
    monkeypatch.chdir(tmp_path)
    train, test = world.build(str(tmp_path))
    config = _migrated()
    config["hyp_hyp"] = world.HYP_HYP
    return config, train, test


def test_unmigrated_config_stops_with_the_documented_error(job):
    import datasets
    from viquae_amd.ir import hp
    _, train, _ = job
    config = copy.deepcopy(cs.configs()[HP_CONFIG])
    with pytest.raises(NotImplementedError, match="Elasticsearch"):
        hp.hyperparameter_search(objective_type="bm25", train_dataset=datasets.load_from_disk(train), k=world.K, **config)


def test_grid_search_then_test_split(job, tmp_path):
    import datasets
    from viquae_amd.ir import hp
    from viquae_amd.ir.bm25 import MI355XBM25Index
    from viquae_amd.ir.metrics import evaluate
    from viquae_amd.ir.searcher import dataset_search
    config, train, test = job
    with open(tmp_path / "config.json", "wt") as file:
        json.dump(config, file)
    out = tmp_path / "metrics"
    study = hp.main("bm25", str(tmp_path / "config.json"), train=train, k=world.K, metrics=str(out), test=test)

    # the trial table: grid order, the restatement's values, the first maximum
    trials = study.trials
    assert [(t["b"], t["k1"]) for t in trials] == world.GRID
    values = [t["value"] for t in trials]
    # (a mean of 48 reciprocal ranks in float64: within 48 * 2^-53 of the restatement's, whatever the order of the sum)
    assert values == pytest.approx(world.restated_mrr(), rel=0, abs=1e-12)
    assert len({round(v, 9) for v in values}) == 7 and values[0] == 0.5 and max(values) == 1.0
    assert [g for g, v in enumerate(values) if v == 1.0] == [5, 9]
    assert study.best_value == 1.0 and study.best_params == {"b": 0.5, "k1": 0.4}
    assert json.load(open(out / "trials.json")) == trials
    objective = study.objective
    assert objective.metric_for_best_model == f"mrr@{world.K}" and isinstance(study.sampler, hp.GridSampler)
    assert study.sampler.search_space == dict(b=[0.0, 0.5, 1.0], k1=[0.0, 0.4, 1.2, 2.9])

    # value for value what the per-trial loop gives: set_bm25 + the existing dataset_search + metrics.evaluate
    index = objective.index
    assert isinstance(index, MI355XBM25Index) and index.ntotal == 3 * world.NQ
    assert (index.k1, index.b) == (0.4, 0.5)  # the test split was searched with the best parameters
    questions = datasets.load_from_disk(train)
    loop = []
    for b, k1 in world.GRID:
        index.set_bm25(k1, b)
        searcher = dataset_search(questions, k=world.K, report=False, kbs=objective.searcher.kbs, reference_kb=objective.searcher.reference_kb,
                                  kb_kwargs=config["kb_kwargs"], map_kwargs=config["map_kwargs"])
        loop.append(evaluate(searcher.qrels, searcher.runs["BM25"], f"mrr@{world.K}"))
    assert values == loop

    # the test split's files: those of dataset_search at the best parameters
    index.set_bm25(0.4, 0.5)
    want = tmp_path / "want"
    dataset_search(datasets.load_from_disk(test), k=world.K, metric_save_path=want, kbs=objective.searcher.kbs,
                   reference_kb=objective.searcher.reference_kb, kb_kwargs=config["kb_kwargs"], map_kwargs=config["map_kwargs"])
    for name in ("qrels.json", "metrics.json", "BM25.json"):
        assert json.load(open(out / name)) == json.load(open(want / name)), name
    assert open(out / "metrics.tex").read() == open(want / "metrics.tex").read()
    report = json.load(open(out / "metrics.json"))
    assert report["model_names"] == ["BM25"] and report["BM25"]["scores"]["mrr@100"] == 1.0
    assert len(json.load(open(out / "BM25.json"))) == 20 and len(datasets.load_from_disk(test)) == 20


def test_test_split_alone_uses_the_configs_parameters(job, tmp_path):
    from viquae_amd.ir import hp
    config, _, test = job
    with open(tmp_path / "config.json", "wt") as file:
        json.dump(config, file)
    study = hp.main("bm25", str(tmp_path / "config.json"), k=world.K, metrics=str(tmp_path / "metrics"), test=test)
    assert study.trials == [] and (study.objective.index.k1, study.objective.index.b) == (0.5, 0.3)
    assert not (tmp_path / "metrics" / "trials.json").exists() and (tmp_path / "metrics" / "metrics.json").exists()


def test_two_bm25_indexes_fusion_and_other_samplers_are_refused(job):
    import datasets
    from viquae_amd.ir import hp
    config, train, _ = job
    questions = datasets.load_from_disk(train)
    with pytest.raises(NotImplementedError, match="sampler"):
        hp.hyperparameter_search(objective_type="bm25", train_dataset=questions, k=world.K, study_kwargs={"sampler": "TPESampler"}, **config)
    two = copy.deepcopy(config)
    (kb,) = two["kb_kwargs"].values()
    kb["index_kwargs"]["BM25_again"] = copy.deepcopy(kb["index_kwargs"]["BM25"])
    with pytest.raises(NotImplementedError, match="fusion"):   # two indexes: the Searcher fuses them by default
        hp.get_objective("bm25", questions, k=world.K, **{n: v for n, v in two.items() if n not in ("study_name", "storage")})
    with pytest.raises(ValueError, match="exactly one"):
        hp.get_objective("bm25", questions, k=world.K, do_fusion=False, **{n: v for n, v in two.items() if n not in ("study_name", "storage")})
