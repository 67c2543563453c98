"""CPU suite of the reader stage (viquae_amd/rc/reader.py): the host side of the evaluation against the reference-minted
golden (tools/make_golden_reader.py), the SQuAD metrics, the numpy restatement of the span search, the output files and
the binding of the shipped config.  The device steps are in tests/test_reader_gpu.py."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests import reader_restatement as rr

GOLDEN = rr.load_golden()
NPZ = {size: np.load(os.path.join(rr.GOLDEN, f"reader_{size}.npz")) for size in GOLDEN["sizes"]}


def _data_kwargs(paths, run=False):
    kw = dict(GOLDEN["settings"]["data"]["init_args"])
    kw.update(kb=paths["kb"], dataset_path=paths["dataset"], tokenizer_name_or_path=paths["tokenizer"],
              run_path=paths["run"] if run else None)
    return kw


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return rr.write_world(str(tmp_path_factory.mktemp("reader_world")), GOLDEN["world"])


@pytest.mark.parametrize("source", ["search_key", "run_path"])
def test_batches_match_the_reference_collate(world, source):
    from viquae_amd.rc.reader import ReaderData
    data = ReaderData(**_data_kwargs(world, run=source == "run_path"))
    assert data.M == GOLDEN["M"] == 24 and data.batch_size == GOLDEN["batch_size"] == 8
    d = NPZ["tiny"]
    batches = list(data.batches(data.split("test")))
    assert [len(b) for b in batches] == [8, 8]
    for bi, items in enumerate(batches):
        batch, scores, answers = data.collate(items)
        for k in ("input_ids", "token_type_ids", "attention_mask"):
            assert np.array_equal(batch[k].numpy(), d[f"b{bi}_{k}"]), (bi, k)
        assert scores.dtype == np.float32 and np.array_equal(scores.reshape(-1), d[f"b{bi}_passage_scores"])
        assert answers == [q["output"]["answer"] for q in GOLDEN["world"]["questions"][8 * bi: 8 * bi + 8]]
    # the ragged questions: fewer than M results (padded with '' and 0) and none at all
    assert d["b1_passage_scores"].reshape(8, 24)[1].tolist() == [0.0] * 24
    assert d["b1_input_ids"].shape[1] == 256  # the long passage is truncated at max_length


def test_weight_shift_per_batch():
    from viquae_amd.rc.reader import shift_weights
    d = NPZ["tiny"]
    shifts = []
    for bi in range(2):
        scores = d[f"b{bi}_passage_scores"].reshape(8, 24)
        with pytest.warns(UserWarning, match="adding 1-minimum"):
            w = shift_weights(scores)
        assert w.dtype == np.float32 and np.array_equal(w, d[f"b{bi}_shifted_weights"])
        assert np.array_equal(w, rr.shift_weights(scores))
        shifts.append(float(w[0, 0] - scores[0, 0]))
    assert shifts[0] != shifts[1]  # two batches, two minima, two shifts
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.array_equal(shift_weights(np.full((2, 3), 2.5, np.float32)), np.full((2, 3), 2.5, np.float32))


@pytest.mark.parametrize("size", ["tiny", "base2"])
def test_decoding_of_given_triples(world, size):
    from transformers import BertTokenizerFast
    from viquae_amd.rc.reader import decode_answers
    tok = BertTokenizerFast.from_pretrained(world["tokenizer"])
    d, g = NPZ[size], GOLDEN["sizes"][size]
    for bi, gb in enumerate(g["batches"]):
        ids = d[f"b{bi}_input_ids"].reshape(gb["N"], GOLDEN["M"], gb["L"])
        assert decode_answers(tok, ids, *d[f"b{bi}_spans"]) == gb["predictions"]
        assert decode_answers(tok, ids, *d[f"b{bi}_weighted_spans"]) == gb["weighted_predictions"]


def test_em_f1_against_squad_per_question():
    from viquae_amd.rc.reader import normalize_answer, per_question_metrics
    for case in GOLDEN["metric_cases"]:
        got = per_question_metrics([case["prediction"]], [case["answers"]])
        assert got == case["reference"], case
    assert normalize_answer("  The  U.S.A.,  an  Apple! ") == "usa apple"
    assert normalize_answer("") == ""


@pytest.mark.parametrize("size", ["tiny", "base2"])
def test_per_question_metrics_and_averages(size):
    from viquae_amd.rc.reader import average_metrics, per_question_metrics
    g = GOLDEN["sizes"][size]
    per_question = {"exact_match": [], "f1": [], "weighted_exact_match": [], "weighted_f1": []}
    for gb in g["batches"]:
        answers = [q["output"]["answer"] for q in GOLDEN["world"]["questions"]][len(per_question["f1"]):][: gb["N"]]
        for prefix, preds, ref in (("", gb["predictions"], gb["metrics"]), ("weighted_", gb["weighted_predictions"],
                                                                            gb["weighted_metrics"])):
            m = per_question_metrics(preds, answers)
            assert m == {k: [float(x) for x in v] for k, v in ref.items()}
            for k, v in m.items():
                per_question[prefix + k].extend(v)
    assert average_metrics(per_question) == g["metrics"]
    assert average_metrics({"exact_match": [], "f1": [1.0]}) == {"exact_match": None, "f1": 1.0}


def test_restatement_matches_the_reference_spans():
    for case in GOLDEN["planted"]:
        w = None if case["weights"] is None else np.array(case["weights"], np.float32)
        got = rr.best_spans(np.array(case["start"], np.float32), np.array(case["end"], np.float32), w,
                            case["cannot_be_first_token"])
        assert got.tolist() == case["reference"], case
    for size, g in GOLDEN["sizes"].items():
        d = NPZ[size]
        for bi, gb in enumerate(g["batches"]):
            N, M, L = gb["N"], GOLDEN["M"], gb["L"]
            p = [torch.log_softmax(torch.from_numpy(d[f"b{bi}_{k}_logits"]).reshape(N, M * L), 1).exp().reshape(N, M, L).numpy()
                 for k in ("start", "end")]
            assert np.array_equal(rr.best_spans(*p), d[f"b{bi}_spans"]), (size, bi)
            assert np.array_equal(rr.best_spans(*p, d[f"b{bi}_shifted_weights"]), d[f"b{bi}_weighted_spans"]), (size, bi)


def test_output_files(tmp_path):
    from viquae_amd.rc.reader import write_outputs
    g = GOLDEN["sizes"]["tiny"]
    result = {"metrics": g["metrics"], "predictions": g["predictions"], "weighted_predictions": g["weighted_predictions"]}
    write_outputs(result, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["metrics.json", "predictions.json", "weighted_predictions.json"]
    metrics = json.load(open(tmp_path / "metrics.json"))
    assert list(metrics) == ["exact_match", "f1", "weighted_exact_match", "weighted_f1"] and metrics == g["metrics"]
    assert json.load(open(tmp_path / "predictions.json")) == g["predictions"]
    assert json.load(open(tmp_path / "weighted_predictions.json")) == g["weighted_predictions"]
    empty = tmp_path / "no_weighted"
    write_outputs(dict(result, weighted_predictions=[]), str(empty))
    assert sorted(os.listdir(empty)) == ["metrics.json", "predictions.json"]


def test_shipped_config_binds():
    from viquae_amd.rc.reader import bind_config
    model_kwargs, data_kwargs = bind_config(GOLDEN["settings"])
    assert model_kwargs == {"class_name": "MultiPassageBERT", "fuse_ir_score": False,
                            "pretrained_model_name_or_path": "experiments/rc/triviaqa/lightning_logs/version_0/checkpoints/step=46000"}
    assert data_kwargs["M"] == 24 and data_kwargs["eval_batch_size"] == 8 and data_kwargs["search_key"] == "search"
    assert data_kwargs["tokenization_kwargs"] == {"max_length": 256, "padding": "longest"}


def _settings(model=None, data=None, model_init=None):
    s = json.loads(json.dumps(GOLDEN["settings"]))
    s["model"]["init_args"]["model_kwargs"].update(model or {})
    s["model"]["init_args"].update(model_init or {})
    s["data"]["init_args"].update(data or {})
    return s


@pytest.mark.parametrize("change, feature", [
    (dict(model={"fuse_ir_score": True}), "fuse_ir_score"),
    (dict(model={"class_name": "MultiPassageECA"}), "MultiPassageECA"),
    (dict(model={"class_name": "MultiPassageVilt"}), "MultiPassageVilt"),
    (dict(model_init={"tune_M": True}), "tune_M"),
    (dict(data={"oracle": True}), "oracle"),
    (dict(data={"extract_name": True}), "extract_name"),
    (dict(data={"image_kb": "data/viquae_wikipedia"}), "image_kb"),
])
def test_config_refusals(change, feature):
    from viquae_amd.rc.reader import bind_config
    with pytest.raises(NotImplementedError, match=feature):
        bind_config(_settings(**change))


def test_other_refusals(world, tmp_path):
    from viquae_amd.rc.reader import ReaderData, main
    from viquae_amd.encoders import MultiPassageBERT
    with pytest.raises(NotImplementedError, match="fit"):
        main(["fit", "--config", "unused.yaml"])
    with pytest.raises(NotImplementedError, match="fuse_ir_score"):
        MultiPassageBERT({}, {"score_proj_w": torch.ones(1, 1)})
    with pytest.raises(NotImplementedError, match="fuse_ir_score"):
        MultiPassageBERT({}, {}, fuse_ir_score=True)
    for key in ("oracle", "extract_name"):
        with pytest.raises(NotImplementedError, match=key):
            ReaderData(**dict(_data_kwargs(world), **{key: True}))
    data = ReaderData(**_data_kwargs(world))
    item = dict(data.split("test")[0], question_type="Numerical")
    with pytest.raises(NotImplementedError, match="question type"):
        data.collate([item])
    bad_run = tmp_path / "run.trec"
    bad_run.write_text("q00 Q0 1 1 1.0 x\n")
    with pytest.raises(NotImplementedError, match="JSON"):
        ReaderData(**dict(_data_kwargs(world), run_path=str(bad_run)))


def test_class_name_resolves_to_the_hip_reader():
    from viquae_amd import encoders
    from viquae_amd.data.loading import get_class_from_name
    assert get_class_from_name("MultiPassageBERT") is encoders.MultiPassageBERT


def test_map_run():
    from viquae_amd.rc.reader import map_run

    class Run:
        run = {"q": {"a": 3.0, "b": 2.0, "c": 1.0}, "e": {}}
    mapped = map_run(Run(), {"a": [4, 5], "b": [6], "c": [7]}, k=3)
    assert mapped.run == {"q": {"4": 3.0, "5": 3.0, "6": 2.0}, "e": {}}
    # a document is taken whole once started; an id met again keeps its place and takes the later score
    mapped = map_run(Run(), {"a": [4, 5], "b": [5, 6, 7], "c": [8]}, k=3)
    assert list(mapped.run["q"].items()) == [("4", 3.0), ("5", 2.0), ("6", 2.0), ("7", 2.0)]
    assert list(map_run(Run(), {"a": [4], "b": [4], "c": [9]}, k=5).run["q"].items()) == [("4", 2.0), ("9", 1.0)]


def test_mapping_run_feeds_the_passages(world, tmp_path):
    """run_path + mapping_run: the run's documents are re-keyed to knowledge-base rows before the top M are taken."""
    from viquae_amd.rc.reader import ReaderData
    run = json.load(open(world["run"]))
    mapping = {doc: [(int(doc) + 1) % len(GOLDEN["world"]["passages"])] for docs in run.values() for doc in docs}
    mapping_path = tmp_path / "mapping.json"
    mapping_path.write_text(json.dumps(mapping))
    data = ReaderData(**dict(_data_kwargs(world, run=True), mapping_run=str(mapping_path)))
    item = data.split("test")[0]
    texts, scores = data.eval_passages(item)
    rows = [(i + 1) % len(GOLDEN["world"]["passages"]) for i in item["search_indices"][:24]]
    assert texts == [GOLDEN["world"]["passages"][r] for r in rows]
    assert scores == list(item["search_scores"][:24])


def test_token_f1_edges():
    from viquae_amd.rc.reader import token_f1
    assert token_f1([], ["a"]) == 0.0 and token_f1(["a"], []) == 0.0 and token_f1([], []) == 0.0
    assert token_f1(["x", "x", "y"], ["x", "y", "y"]) == 2 * (2 / 3) * (2 / 3) / (2 / 3 + 2 / 3)
    assert token_f1(["a", "b"], ["b", "a"]) == 1.0


def test_unknown_model_kwargs_are_refused():
    from viquae_amd.encoders import MultiPassageBERT
    from viquae_amd.data.loading import get_pretrained
    with pytest.raises(NotImplementedError, match="config"):
        MultiPassageBERT.from_pretrained("unused/checkpoint", config={"num_labels": 3})
    with pytest.raises(NotImplementedError, match="torch_dtype"):
        get_pretrained("MultiPassageBERT", "unused/checkpoint", fuse_ir_score=False, torch_dtype="float16")
