"""The reader stage: extractive answers from the top-M passages of a retrieval run, scored with SQuAD exact match and F1.

Mirrors the EVALUATION path of the reference's ``Reader`` (meerqat/train/trainee.py:742-824) fed by ``ReaderDataModule``
(meerqat/train/data.py:925-1076), as ``experiments/rc/viquae/config.yaml`` runs it:

  1. per question, the passage ids / scores of ``item[search_key + "_indices" / "_scores"][:M]`` or of the run at ``run_path``
     (optionally through ``mapping_run``); missing passages are '' and missing scores 0
  2. ``tokenizer(questions, passages, return_tensors='pt', padding='longest', truncation=True, ...)`` -> [N * M, L], one
     tokenizer call per batch of ``eval_batch_size`` questions (the batch fixes L and the weight shift)
  3. MultiPassageBERT (viquae_amd.encoders, dense BERT forward + QA head on the device) -> start / end logits of every position
  4. one log-softmax per question over its M * L positions, on the device (csrc/reader.hip)
  5. the best span of get_best_spans, on the device, once plain and once weighted by the passage scores (shifted to >= 1)
  6. ``tokenizer.batch_decode(..., skip_special_tokens=True)`` and per-question EM / F1 (max over the answer aliases)
  7. averages as in ``eval_epoch_end``; ``metrics.json``, ``predictions.json``, ``weighted_predictions.json``

CLI (the reference's LightningCLI call; the trainer keys of the YAML are ignored, Lightning is not needed):
    python -m viquae_amd.rc.reader test --config experiments/rc/viquae/config.yaml [--output DIR]

Training (``fit``), the eval loss, oracle passages, name extraction, M tuning, image knowledge bases and the multimodal
readers are not provided and refuse with NotImplementedError.
"""
import argparse
import itertools
import json
import os
import re
import string
import sys
import warnings
from collections import Counter

import numpy as np
import torch

from .. import _lib

# --------------------------------------------------------------------------------------------------
# SQuAD answer normalisation and metrics
# --------------------------------------------------------------------------------------------------
_DROP_PUNCTUATION = {ord(c): None for c in string.punctuation}
_ARTICLE = re.compile(r"\b(?:a|an|the)\b")


def normalize_answer(text):
    """SQuAD normalisation: lower case, ASCII punctuation deleted, the words 'a', 'an', 'the' replaced by a space, runs of
    whitespace collapsed to one space, no leading or trailing space."""
    text = text.lower().translate(_DROP_PUNCTUATION)
    return " ".join(_ARTICLE.sub(" ", text).split())


def _shared_token_count(tokens, other):
    """Size of the multiset intersection of two token lists: each token of ``other`` claims one unclaimed equal token."""
    unclaimed = Counter(tokens)
    shared = 0
    for t in other:
        if unclaimed[t]:
            unclaimed[t] -= 1
            shared += 1
    return shared


def token_f1(prediction_tokens, truth_tokens):
    """SQuAD's F1 of two token lists: the harmonic mean 2 p r / (p + r) of the token precision p = shared / |prediction| and
    recall r = shared / |truth|, evaluated left to right in double precision; 0 when no token is shared (an empty side
    included)."""
    shared = _shared_token_count(prediction_tokens, truth_tokens)
    if not shared:
        return 0.0
    p, r = shared / len(prediction_tokens), shared / len(truth_tokens)
    return 2 * p * r / (p + r)


def question_scores(prediction, answers):
    """(exact match, F1) of one predicted string against the answer aliases of its question: the best alias counts."""
    pred = normalize_answer(prediction)
    aliases = [normalize_answer(a) for a in answers]
    em = 1.0 if pred in aliases else 0.0
    f1 = max(token_f1(pred.split(), a.split()) for a in aliases)
    return em, f1


def per_question_metrics(predictions, references):
    """{'exact_match': [...], 'f1': [...]} over the questions (squad_per_question, meerqat/train/metrics.py:156-178)."""
    if len(predictions) != len(references):
        raise ValueError(f"{len(predictions)} predictions for {len(references)} questions")
    scores = [question_scores(p, r) for p, r in zip(predictions, references)]
    return {"exact_match": [s[0] for s in scores], "f1": [s[1] for s in scores]}


def average_metrics(per_question):
    """The mean of every list in ``per_question`` (summed in question order), None for an empty list (eval_epoch_end)."""
    return {k: (sum(v) / len(v) if v else None) for k, v in per_question.items()}


# --------------------------------------------------------------------------------------------------
# device steps
# --------------------------------------------------------------------------------------------------
def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def log_softmax_per_question(start_logits, end_logits, N, M, L):
    """One log-softmax per question over its M * L start (and end) logits, and the probabilities exp(logp).
    -> (start_logp, end_logp, start_p, end_p), each fp32 [N, M, L] on the logits' device."""
    if not (start_logits.is_cuda and end_logits.is_cuda):
        raise _lib.MeerqatHipError("the reader runs on MI355X only: logits must be on a GPU (no CPU fallback)")
    lib = _lib.load()
    s = start_logits.to(torch.float32).contiguous()
    e = end_logits.to(torch.float32).contiguous()
    if s.numel() != N * M * L or e.numel() != N * M * L:
        raise ValueError(f"logits of {s.numel()} / {e.numel()} elements for N={N}, M={M}, L={L}")
    out = torch.empty((4, N, M, L), dtype=torch.float32, device=s.device)
    with torch.cuda.device(s.device):
        _lib.check(lib.mq_reader_log_softmax_f32(s.data_ptr(), e.data_ptr(), N, M, L, out[0].data_ptr(), out[1].data_ptr(),
                                                 out[2].data_ptr(), out[3].data_ptr(), _stream(s)), "mq_reader_log_softmax_f32")
    return out[0], out[1], out[2], out[3]


def best_spans(start_probs, end_probs, weights=None, cannot_be_first_token=True):
    """get_best_spans (meerqat/models/qa.py:18-77) on the device: probabilities [N, M, L], optional passage weights [N, M]
    (ALREADY shifted: see :func:`shift_weights`) -> (passage, start, end exclusive) as int64 device tensors [N]."""
    if not (start_probs.is_cuda and end_probs.is_cuda):
        raise _lib.MeerqatHipError("the reader runs on MI355X only: probabilities must be on a GPU (no CPU fallback)")
    lib = _lib.load()
    N, M, L = start_probs.shape
    if tuple(end_probs.shape) != (N, M, L):
        raise ValueError(f"start {tuple(start_probs.shape)} and end {tuple(end_probs.shape)} probabilities differ in shape")
    s = start_probs.to(torch.float32).contiguous()
    e = end_probs.to(torch.float32).contiguous()
    w = None
    if weights is not None:
        w = torch.as_tensor(weights, dtype=torch.float32).to(s.device).contiguous()
        if w.numel() != N * M:
            raise ValueError(f"{w.numel()} weights for N={N}, M={M}")
    out = torch.empty((3, N), dtype=torch.int64, device=s.device)
    with torch.cuda.device(s.device):
        _lib.check(lib.mq_reader_best_spans_f32(s.data_ptr(), e.data_ptr(), w.data_ptr() if w is not None else None, N, M, L,
                                                int(bool(cannot_be_first_token)), out[0].data_ptr(), out[1].data_ptr(),
                                                out[2].data_ptr(), _stream(s)), "mq_reader_best_spans_f32")
    return out[0], out[1], out[2]


def shift_weights(passage_scores):
    """The reference's in-place shift of the weights (get_best_spans): if the batch-wide minimum is below 1, ``1 - min`` is
    added to every weight, in fp32, with its warning.  ``passage_scores`` fp32 [N, M] (or [N * M]) -> a shifted copy."""
    w = np.array(passage_scores, dtype=np.float32, copy=True)
    offset = np.float32(1) - w.min()  # > 0 exactly when the minimum is below 1 (Sterbenz: exact near 1)
    if offset > 0:
        warnings.warn("weights should be > 1, adding 1-minimum")
        w += offset
    return w


def decode_answers(tokenizer, input_ids, passages, starts, ends):
    """``tokenizer.batch_decode(input_ids[q, p, start:end], skip_special_tokens=True)`` for every question q.
    input_ids: host int array [N, M, L]; the triples: host ints [N]."""
    ids = np.asarray(input_ids)
    spans = [ids[q, int(p), int(s):int(e)].tolist() for q, (p, s, e) in enumerate(zip(passages, starts, ends))]
    return tokenizer.batch_decode(spans, skip_special_tokens=True)


# --------------------------------------------------------------------------------------------------
# passages and batches (ReaderDataModule in evaluation)
# --------------------------------------------------------------------------------------------------
class _MappedRun:
    def __init__(self, run):
        self.run = run


def _expand_ranking(ranking, mapping, k):
    """One query's ranking with every document replaced by the ids ``mapping`` lists for it (as strings, each taking the
    document's score; an id met again keeps its first place and takes the later score).  Documents are taken whole, best
    first, until at least ``k`` distinct ids are held."""
    expanded = {}
    for doc, score in ranking.items():
        if len(expanded) >= k:
            break
        expanded.update(dict.fromkeys(map(str, mapping[doc]), score))
    return expanded


def map_run(run, mapping, k=100):
    """A run re-keyed through ``mapping`` (document id -> list of new ids), as the reader's ``mapping_run`` option does
    (meerqat/train/data.py:864-874) -> an object whose ``.run`` is {query id: {new id: score}}."""
    if k < 1:
        raise ValueError(f"map_run keeps at least one id per query (k = {k})")
    return _MappedRun({q: _expand_ranking(ranking, mapping, k) for q, ranking in run.run.items()})


def _read_run(run_path, mapping_path, k):
    """The run at ``run_path`` (viquae_amd.ir.embedding.load_run: ranx, or a JSON run without it), re-keyed through the JSON
    mapping at ``mapping_path`` when one is given; None without a run."""
    if run_path is None:
        return None
    from ..ir.embedding import load_run
    run = load_run(run_path)
    if mapping_path is None:
        return run
    with open(mapping_path, "rt") as file:
        return map_run(run, json.load(file), k=k)


def _refuse(feature):
    raise NotImplementedError(f"reader: {feature} is not provided by viquae_amd (evaluation of MultiPassageBERT over text "
                              "passages only)")


class ReaderData:
    """The evaluation side of ReaderDataModule: questions of one split, their top-M passages and the tokenized batches."""

    def __init__(self, tokenizer_class, tokenizer_name_or_path, kb, dataset_path=None, train_path=None, validation_path=None,
                 test_path=None, batch_size=8, train_batch_size=None, eval_batch_size=None, M=24, n_relevant_passages=1,
                 keep_dataset_columns=None, tokenization_kwargs=None, image_kwargs=None, loader_kwargs=None,
                 dataset_format=None, input_key="input", image_kb=None, search_key="search", filter_train_rels=False,
                 keep_kb_columns=None, kb_format=None, image_kb_format=None, kb_input_key="passage", max_n_answers=10,
                 run_path=None, train_original_answer_only=True, oracle=False, extract_name=False, mapping_run=None,
                 tokenizer=None):
        if oracle:
            _refuse("oracle: true (relevant passages only)")
        if extract_name:
            _refuse("extract_name (answering with the entity name)")
        if image_kb is not None:
            _refuse("image_kb (multimodal passages)")
        if image_kwargs:
            _refuse("image_kwargs (image features of the multimodal readers)")
        if dataset_path is None and test_path is None:
            raise ValueError("reader: dataset_path or test_path is needed to evaluate the test split")
        from datasets import load_from_disk
        from ..data.loading import get_pretrained
        self.tokenizer = tokenizer if tokenizer is not None else get_pretrained(
            tokenizer_class, pretrained_model_name_or_path=tokenizer_name_or_path)
        self.dataset_path, self.test_path = dataset_path, test_path
        self.batch_size = eval_batch_size if eval_batch_size is not None else batch_size
        self.M = int(M)
        if self.M < 1 or self.batch_size < 1:
            raise ValueError(f"reader: M = {M} and eval_batch_size = {self.batch_size} must be positive")
        self.input_key, self.kb_input_key, self.search_key = input_key, kb_input_key, search_key
        self.kb = load_from_disk(kb)
        if kb_format is not None:
            self.kb.set_format(**kb_format)
        self.tokenization_kwargs = dict(return_tensors="pt", padding="longest", truncation=True, return_overflowing_tokens=False)
        self.tokenization_kwargs.update(tokenization_kwargs or {})
        self.run = _read_run(run_path, mapping_run, self.M)

    def split(self, name="test"):
        from datasets import load_from_disk
        if self.dataset_path is None:
            return load_from_disk(self.test_path)
        return load_from_disk(self.dataset_path)[name]

    def ranking(self, item):
        """(knowledge-base rows, scores) of one question's retrieval results, best first, at most M of each: from the
        dataset's ``<search_key>_indices`` / ``_scores`` columns, or from the run (its document ids are strings of rows)."""
        if self.run is not None:
            results = self.run.run[item["id"]]
            top = list(itertools.islice(results.items(), self.M))
            return [int(doc) for doc, _ in top], [score for _, score in top]
        rows, scores = item[f"{self.search_key}_indices"], item[f"{self.search_key}_scores"]
        return list(rows[: self.M]), list(scores[: self.M])

    def eval_passages(self, item):
        """(passage texts, scores) of the top-M results of one question; a question without results has none."""
        rows, scores = self.ranking(item)
        texts = self.kb.select(rows)[self.kb_input_key] if rows else []
        return list(texts), scores

    def collate(self, items):
        """-> (tokenizer output [N * M, L], passage scores fp32 [N, M], answer aliases per question)"""
        questions, passages, scores, answers = [], [], [], []
        for item in items:
            if item.get("question_type", "String") not in ("String", None):
                _refuse(f"question type {item['question_type']!r} (numerical / time answers)")
            passage, score = self.eval_passages(item)
            score = score + [0] * (self.M - len(score))
            passage = passage + [""] * (self.M - len(passage))
            questions.extend([item[self.input_key]] * self.M)
            passages.extend(passage)
            scores.append(score)
            answers.append(item["output"]["answer"])
        batch = self.tokenizer(questions, passages, **self.tokenization_kwargs)
        return batch, np.asarray(scores, dtype=np.float32).reshape(len(items), self.M), answers

    def batches(self, dataset):
        for lo in range(0, len(dataset), self.batch_size):
            yield [dataset[i] for i in range(lo, min(lo + self.batch_size, len(dataset)))]


# --------------------------------------------------------------------------------------------------
# the job
# --------------------------------------------------------------------------------------------------
def answer_batch(model, data, batch, scores, device):
    """Device forward, normalisation and both span searches of one batch -> (predictions, weighted predictions)."""
    N, M = scores.shape
    ids = batch["input_ids"]
    L = ids.shape[1]
    inputs = {k: batch[k].to(device, non_blocking=True) for k in ("input_ids", "attention_mask", "token_type_ids") if k in batch}
    out = model(**inputs)
    _, _, sp, ep = log_softmax_per_question(out["start_logits"], out["end_logits"], N, M, L)
    plain = torch.stack(best_spans(sp, ep)).cpu().numpy()
    weighted = torch.stack(best_spans(sp, ep, weights=shift_weights(scores))).cpu().numpy()
    ids = ids.reshape(N, M, L).numpy()
    return decode_answers(data.tokenizer, ids, *plain), decode_answers(data.tokenizer, ids, *weighted)


def evaluate(model, data, split="test", device=None):
    """Runs the reader over a split -> {'metrics': ..., 'predictions': [...], 'weighted_predictions': [...]}."""
    device = torch.device(device or "cuda")
    per_question = {"exact_match": [], "f1": [], "weighted_exact_match": [], "weighted_f1": []}
    predictions, weighted_predictions = [], []
    for items in data.batches(data.split(split)):
        batch, scores, answers = data.collate(items)
        pred, wpred = answer_batch(model, data, batch, scores, device)
        for prefix, p in (("", pred), ("weighted_", wpred)):
            for k, v in per_question_metrics(p, answers).items():
                per_question[prefix + k].extend(v)
        predictions.extend(pred)
        weighted_predictions.extend(wpred)
    return {"metrics": average_metrics(per_question), "predictions": predictions, "weighted_predictions": weighted_predictions}


def write_outputs(result, output_dir):
    """metrics.json, predictions.json and (when there are any) weighted_predictions.json, as test_epoch_end writes them."""
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, "metrics.json"), "wt") as file:
        json.dump(result["metrics"], file)
    with open(os.path.join(output_dir, "predictions.json"), "wt") as file:
        json.dump(result["predictions"], file)
    if result["weighted_predictions"]:
        with open(os.path.join(output_dir, "weighted_predictions.json"), "wt") as file:
            json.dump(result["weighted_predictions"], file)


_MULTIMODAL_READERS = ("MultiPassageECA", "MultiPassageVilt")


def bind_config(config):
    """The reader's parts of a LightningCLI config (dict): -> (model_kwargs, data init_args).  The trainer keys are ignored;
    what the evaluation cannot honour refuses here, before anything is loaded."""
    model = config.get("model") or {}
    if model.get("class_path", "meerqat.train.trainee.Reader").rsplit(".", 1)[-1] != "Reader":
        _refuse(f"model class {model.get('class_path')!r} (only meerqat.train.trainee.Reader)")
    init = dict(model.get("init_args") or {})
    if init.get("tune_M"):
        _refuse("tune_M (tuning the number of passages)")
    model_kwargs = dict(init.get("model_kwargs") or {})
    name = model_kwargs.get("class_name")
    if name in _MULTIMODAL_READERS:
        _refuse(f"the multimodal reader {name}")
    if name != "MultiPassageBERT":
        _refuse(f"reader class {name!r} (only MultiPassageBERT)")
    if model_kwargs.get("fuse_ir_score"):
        _refuse("fuse_ir_score: true")
    data = config.get("data") or {}
    if data.get("class_path", "meerqat.train.data.ReaderDataModule").rsplit(".", 1)[-1] != "ReaderDataModule":
        _refuse(f"data module {data.get('class_path')!r} (only meerqat.train.data.ReaderDataModule)")
    data_kwargs = dict(data.get("init_args") or {})
    for key, feature in (("oracle", "oracle: true (relevant passages only)"), ("extract_name", "extract_name"),
                         ("image_kb", "image_kb (multimodal passages)"), ("image_kwargs", "image_kwargs (multimodal readers)")):
        if data_kwargs.get(key):
            _refuse(feature)
    return model_kwargs, data_kwargs


def load_config(path):
    import yaml
    with open(path, "rt") as file:
        return yaml.safe_load(file)


def test(config, output=None, device=None):
    """The reference's ``test`` subcommand: load the reader and the data of ``config`` (a path or a dict), evaluate split
    'test' and write the three files under ``output``.  -> the result of :func:`evaluate`."""
    cfg = load_config(config) if isinstance(config, (str, os.PathLike)) else config
    model_kwargs, data_kwargs = bind_config(cfg)
    _lib.require_gpu()
    from ..data.loading import get_pretrained
    data = ReaderData(**data_kwargs)
    model = get_pretrained(**model_kwargs).to(device or "cuda").eval()
    result = evaluate(model, data, "test", device)
    if output is None:
        output = os.path.dirname(os.path.abspath(config)) if isinstance(config, (str, os.PathLike)) else "."
    write_outputs(result, output)
    return result


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m viquae_amd.rc.reader", description=__doc__.split("\n")[0])
    parser.add_argument("subcommand", choices=["fit", "validate", "test", "predict"])
    parser.add_argument("--config", required=True)
    parser.add_argument("--output", default=None, help="where metrics.json and the predictions go (default: the config's folder)")
    args = parser.parse_args(argv)
    if args.subcommand != "test":
        _refuse(f"the '{args.subcommand}' subcommand (training and the other stages; only 'test')")
    result = test(args.config, args.output)
    print(json.dumps(result["metrics"]))


if __name__ == "__main__":
    sys.exit(main())
