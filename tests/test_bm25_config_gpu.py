"""GPU, end to end: the two shipped BM25 search configs (tests/golden/config_surface.json) after the documented migration -- in
memory only, ``"es": true`` replaced by ``"kind": "BM25"`` and ``"load": false`` -- run through ``dataset_search`` over the
synthetic world of tests/config_surface.py: the KB column ``passage`` holds the texts, the question key ``input`` holds the
strings "who mentions answer{i}".  (The unmodified files still stop with the documented error: tests/test_config_surface_*.)"""
import copy
import json

import pytest

from tests import config_surface as cs

pytestmark = pytest.mark.gpu

BM25_ONLY = "experiments/ir/viquae/bm25/config.json"
FUSED = "experiments/ir/viquae/bm25+arcface+clip+imagenet/config_test.json"


def _migrated(rel):
    config = copy.deepcopy(cs.configs()[rel])
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


def _world(config, root, nq=48):
    """tests/config_surface.build_search_world lays every dataset out (the reference KB's ``passage`` column -- the BM25 column -- holds
    the texts); the question column of the BM25 index then becomes the question strings."""
    questions, world = cs.build_search_world(config, root, nq=nq)
    questions = questions.remove_columns("input").add_column("input", [f"who mentions answer{i}" for i in range(nq)])
    return questions, world


@pytest.mark.parametrize("rel", [BM25_ONLY, FUSED])
def test_migrated_bm25_config_runs_to_the_end(rel, tmp_path, monkeypatch):
    import datasets
    from viquae_amd.ir.bm25 import MI355XBM25Index
    from viquae_amd.ir.searcher import dataset_search
    datasets.disable_progress_bars()
    config = _migrated(rel)
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "metrics"
    nq = 48
    questions, world = _world(config, str(tmp_path), nq)
    questions.set_format(**config.pop("format", {}))
    searcher = dataset_search(questions, k=10, metric_save_path=out, **config)
    (kb_path,) = [p for p, kb in config["kb_kwargs"].items() if "BM25" in kb["index_kwargs"]]
    index = searcher.kbs[kb_path].dataset._indexes["BM25"]
    assert isinstance(index, MI355XBM25Index) and (index.k1, index.b) == (0.5, 0.3) and index.ntotal == 360
    runs = {name: (run.to_dict() if hasattr(run, "to_dict") else dict(run)) for name, run in searcher.runs.items()}
    assert set(runs) == set(world["index_names"])
    bm25 = runs["BM25"]
    for i in range(nq):
        ranked = list(bm25[f"q{i}"])
        assert ranked[:2] == [str(3 * i), str(3 * i + 1)], (i, ranked[:3])
        assert len(ranked) == 10
    assert json.load(open(out / "BM25.json")) == bm25
    report = json.load(open(out / "metrics.json"))
    assert report["model_names"] == list(runs)
    assert report["BM25"]["scores"]["precision@1"] == 1.0 and report["BM25"]["scores"]["mrr@100"] == 1.0
    if rel == BM25_ONLY:
        assert not searcher.do_fusion
        return
    fused = json.load(open(out / "test_run.json"))
    assert set(fused) == {f"q{i}" for i in range(nq)}
    assert all(len(run) >= 10 for run in fused.values())
