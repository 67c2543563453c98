"""GPU: a BM25 search job whose questions have FEWER than k hits.  The index fills the slots behind a question's last hit with
``(-inf, -1)``; the Searcher keeps only the hits in its runs (a server returns only its hits) -- no ``"-1"`` document in a run, in
the run file or among the judged passages -- on the judged path (a reference KB: relevance decided on the fly) and on the unjudged
one (qrels given, result blocks kept as arrays until the end of the job)."""
import json

import pytest

pytestmark = pytest.mark.gpu

PASSAGES = ["red fox jumps", "red dog sleeps gold", "blue bird sings", "green fish swims", "red red fox"]
QUESTIONS = ["red fox", "blue", "purple"]          # 3 hits, 1 hit, none: all fewer than k = 4
WANT = [["4", "0", "1"], ["2"], []]


def _world():
    import datasets
    from viquae_amd.ir.search import KnowledgeBase
    kb = KnowledgeBase(dataset=datasets.Dataset.from_dict({"passage": PASSAGES}))
    kb.add_or_load_index(column="passage", index_name="BM25", kind="BM25", key="input")
    questions = datasets.Dataset.from_dict({"id": ["a", "b", "c"], "input": QUESTIONS,
                                            "output": [{"original_answer": "gold", "answer": ["gold"]}] * 3})
    return kb, questions


@pytest.mark.parametrize("judged", [True, False])
def test_runs_hold_only_the_hits(judged, tmp_path):
    import datasets
    from viquae_amd.ir.searcher import dataset_search
    datasets.disable_progress_bars()
    kb, questions = _world()
    kwargs = dict(reference_kb=kb.dataset) if judged else dict(qrels=str(tmp_path / "given.json"))
    if not judged:
        with open(tmp_path / "given.json", "wt") as file:
            json.dump({"a": {"1": 1}, "b": {}, "c": {}}, file)
    out = tmp_path / "out"
    searcher = dataset_search(questions, k=4, metric_save_path=out, kb_kwargs={"kb": {}}, kbs={"kb": kb}, **kwargs)
    run = searcher.runs["BM25"]
    assert [list(run[q]) for q in ("a", "b", "c")] == WANT
    assert all(score > 0 for q in run for score in run[q].values())
    assert json.load(open(out / "BM25.json")) == {q: dict(run[q]) for q in ("a", "b", "c")}
    assert searcher.qrels["a"] == {"1": 1}
    if judged:
        assert searcher.qrels == {"a": {"1": 1}, "b": {}, "c": {}}
        assert searcher.qnonrels == {"a": {"4": 0, "0": 0}, "b": {"2": 0}, "c": {}}
    report = json.load(open(out / "metrics.json"))
    assert report["BM25"]["scores"]["mrr@100"] == pytest.approx(1 / 9, abs=1e-12)   # rank 3 for "a", nothing for "b" and "c"
