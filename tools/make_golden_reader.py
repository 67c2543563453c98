#!/usr/bin/env python3
"""Reader golden (tests/golden/reader.json, reader_tiny.npz, reader_base2.npz) from the REFERENCE's own evaluation path:
ReaderDataModule.get_eval_passages / collate_fn (meerqat/train/data.py:925-1076) driven through a stand-in datamodule and
trainer -- once with the `search_key` columns, once with a run -- then the reference's MultiPassageBERT (a Hugging Face
BertForQuestionAnswering whose forward calls multi_passage_rc_loss) and Reader.eval_step / log_probs_to_answers /
eval_epoch_end (meerqat/train/trainee.py:742-824, get_best_spans and squad_per_question inside).  Runs in the build
container only (the reference and its imports live there); the weights are regenerated from their seed on both sides
(tests/reader_restatement.py) and the golden records their checksum."""
import copy
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import reader_restatement as rr  # noqa: E402
from tools import ref_import  # noqa: E402

SIZES = {"tiny": (rr.TINY, 11), "base2": (rr.BASE2, 12)}
CONFIG = os.path.join(ref_import.REFERENCE, "experiments", "rc", "viquae", "config.yaml")

# EM / F1 cases for squad_per_question: punctuation, articles, whitespace, case, empty prediction, several aliases
METRIC_CASES = [
    ("Paris", ["paris"]), ("the Eiffel Tower!", ["Eiffel tower"]), ("  New   York ", ["new york city", "New York"]),
    ("", ["anything"]), ("", [""]), ("an apple a day", ["apple day"]), ("U.S.A.", ["usa"]), ("Hello, world", ["world hello"]),
    ("1,000 km", ["1000 km", "one thousand"]), ("theatre", ["the atre"]), ("a", ["an"]), ("cats and dogs", ["dogs", "cats"]),
    ("Mount Everest in Nepal", ["Everest"]), ("Jean-Paul Sartre", ["jeanpaul sartre"]), ("don't", ["dont", "do not"]),
]


def _datamodule(world, tokenizer, tokenization_kwargs, M, run=None):
    from meerqat.train.data import ImageFormatter, ReaderDataModule
    import datasets
    dm = object.__new__(ReaderDataModule)
    dm.M, dm.search_key, dm.run = M, "search", run
    dm.kb = datasets.Dataset.from_dict({"passage": world["passages"], "index": list(range(len(world["passages"])))})
    dm.kb_input_key, dm.input_key, dm.image_kb, dm.padding_passage = "passage", "input", None, [""]
    dm.oracle, dm.extract_name, dm.train_original_answer_only, dm.max_n_answers = False, False, True, 10
    dm.tokenizer, dm.image_formatter = tokenizer, ImageFormatter()
    dm.tokenization_kwargs = dict(return_tensors="pt", padding="longest", truncation=True, return_overflowing_tokens=False)
    dm.tokenization_kwargs.update(tokenization_kwargs)
    model = types.SimpleNamespace(fuse_ir_score=False)
    dm.trainer = types.SimpleNamespace(state=types.SimpleNamespace(stage="test"), lightning_module=types.SimpleNamespace(model=model))
    return dm


def _reader(model, dm):
    from meerqat.train.trainee import Reader

    class ReaderStandIn:
        tune_M = False
        step, eval_step = Reader.step, Reader.eval_step
        log_probs_to_answers, eval_epoch_end = Reader.log_probs_to_answers, Reader.eval_epoch_end

        def __init__(self):
            self.model = model
            self.trainer = types.SimpleNamespace(datamodule=dm)

        def __call__(self, **inputs):
            return self.model(**inputs)

    return ReaderStandIn()


def main():
    ref_import.install_reader_stubs()
    import datasets
    import yaml
    from meerqat.models.qa import MultiPassageBERT, get_best_spans
    from meerqat.train.metrics import squad_per_question
    from transformers import BertConfig, BertTokenizerFast
    datasets.disable_progress_bars()
    with open(CONFIG) as f:
        cfg = yaml.safe_load(f)
    settings = {"model": {"class_path": cfg["model"]["class_path"], "init_args": cfg["model"]["init_args"]},
                "data": {"class_path": cfg["data"]["class_path"], "init_args": cfg["data"]["init_args"]}}
    data_args = cfg["data"]["init_args"]
    M, batch_size = data_args["M"], data_args["eval_batch_size"]
    world = rr.make_world(M=M)
    tmp = tempfile.mkdtemp(prefix="mq_reader_golden_")
    with open(os.path.join(tmp, "vocab.txt"), "w") as f:
        f.write("\n".join(world["vocab"]) + "\n")
    tokenizer = BertTokenizerFast.from_pretrained(tmp)
    items = [dict(q) for q in datasets.Dataset.from_list(world["questions"])]
    # ranx orders a query's documents by decreasing score: the run below is already in that order
    run = ref_import._RunStandIn({q: dict(sorted(d.items(), key=lambda kv: -kv[1])) for q, d in world["run"].items()})
    golden = {"settings": settings, "world": world, "M": M, "batch_size": batch_size, "sizes": {}}

    # the batches, through both passage sources
    batches = []
    for lo in range(0, len(items), batch_size):
        chunk = items[lo: lo + batch_size]
        a = _datamodule(world, tokenizer, data_args["tokenization_kwargs"], M).collate_fn(copy.deepcopy(chunk))
        b = _datamodule(world, tokenizer, data_args["tokenization_kwargs"], M, run).collate_fn(copy.deepcopy(chunk))
        for k in ("input_ids", "token_type_ids", "attention_mask", "passage_scores"):
            assert torch.equal(a[k], b[k]), k
        assert a["answer_strings"] == b["answer_strings"]
        batches.append(a)

    arrays_common = {}
    for bi, batch in enumerate(batches):
        for k in ("input_ids", "token_type_ids", "attention_mask"):
            arrays_common[f"b{bi}_{k}"] = batch[k].numpy().astype(np.int32)
        arrays_common[f"b{bi}_passage_scores"] = batch["passage_scores"].numpy()

    for size, (arch, seed) in SIZES.items():
        state = rr.reader_state(arch, len(world["vocab"]), seed)
        hf = BertConfig(**rr.hf_config(arch, len(world["vocab"])))
        model = MultiPassageBERT(hf, fuse_ir_score=False).eval()
        missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
        assert not unexpected and all("position_ids" in m for m in missing), (missing, unexpected)
        arrays = dict(arrays_common)
        outputs, entry = [], {"config": arch, "seed": seed, "checksum": rr.state_checksum(state), "batches": []}
        dm = _datamodule(world, tokenizer, data_args["tokenization_kwargs"], M)
        reader = _reader(model, dm)
        for bi, batch in enumerate(batches):
            inputs = {k: (v.clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in batch.items()}
            scores_before = inputs["passage_scores"].clone()
            with torch.no_grad(), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out = reader.eval_step(inputs, bi)
            N = len(out["predictions"])
            L = batch["input_ids"].shape[1]
            # the log-probabilities of the reference's forward (multi_passage_rc_loss), again, and the triples behind the answers
            with torch.no_grad():
                o = model(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], token_type_ids=batch["token_type_ids"],
                          start_positions=batch["start_positions"], end_positions=batch["end_positions"],
                          answer_mask=batch["answer_mask"])
            slp, elp = o.start_log_probs.reshape(N, M, L), o.end_log_probs.reshape(N, M, L)
            assert torch.equal(torch.log_softmax(o.start_logits.reshape(N, M * L), 1).reshape(N, M, L), slp)
            plain = torch.stack(get_best_spans(slp.exp(), elp.exp())).numpy()
            w = scores_before.clone().reshape(N, M)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                weighted = torch.stack(get_best_spans(slp.exp(), elp.exp(), weights=w)).numpy()
            ids = batch["input_ids"].reshape(N, M, L)
            dec = lambda t: tokenizer.batch_decode([ids[q, t[0, q], t[1, q]: t[2, q]] for q in range(N)], skip_special_tokens=True)  # noqa: E731
            assert dec(plain) == out["predictions"] and dec(weighted) == out["weighted_predictions"]
            assert np.array_equal(rr.best_spans(slp.exp().numpy(), elp.exp().numpy()), plain)
            assert np.array_equal(rr.best_spans(slp.exp().numpy(), elp.exp().numpy(), w.numpy()), weighted)
            assert np.array_equal(rr.shift_weights(scores_before.numpy()).reshape(N, M), w.numpy())
            arrays[f"b{bi}_start_logits"] = o.start_logits.numpy().astype(np.float32)
            arrays[f"b{bi}_end_logits"] = o.end_logits.numpy().astype(np.float32)
            arrays[f"b{bi}_shifted_weights"] = w.numpy()
            arrays[f"b{bi}_spans"] = plain
            arrays[f"b{bi}_weighted_spans"] = weighted
            arrays[f"b{bi}_margin"] = rr.best_and_runner_up(slp.exp().numpy(), elp.exp().numpy())
            arrays[f"b{bi}_weighted_margin"] = rr.best_and_runner_up(slp.exp().numpy(), elp.exp().numpy(), w.numpy())
            outputs.append(out)
            entry["batches"].append({"N": N, "L": L, "predictions": out["predictions"],
                                     "weighted_predictions": out["weighted_predictions"], "metrics": out["metrics"],
                                     "weighted_metrics": out["weighted_metrics"]})
        epoch = reader.eval_epoch_end(outputs)
        entry["metrics"] = epoch["metrics"]
        entry["predictions"], entry["weighted_predictions"] = epoch["predictions"], epoch["weighted_predictions"]
        golden["sizes"][size] = entry
        path = os.path.join(rr.GOLDEN, f"reader_{size}.npz")
        np.savez_compressed(path, **arrays)
        print(size, path, os.path.getsize(path), entry["metrics"])

    # get_best_spans on planted cases: exact ties across passages and inside one, all-zero passages, denormal products
    planted = rr.planted_cases()
    golden["planted"] = []
    for case in planted:
        s, e = torch.tensor(case["start"]), torch.tensor(case["end"])
        w = None if case["weights"] is None else torch.tensor(case["weights"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = torch.stack(get_best_spans(s, e, weights=w, cannot_be_first_token=case["cannot_be_first_token"])).tolist()
        golden["planted"].append(dict(case, reference=res))
    golden["metric_cases"] = [{"prediction": p, "answers": a, "reference": squad_per_question([p], [a])} for p, a in METRIC_CASES]
    golden["metric_cases"] = [dict(c, reference={k: [float(x) for x in v] for k, v in c["reference"].items()})
                              for c in golden["metric_cases"]]
    with open(os.path.join(rr.GOLDEN, "reader.json"), "w") as f:
        json.dump(golden, f)
    print("reader.json", os.path.getsize(os.path.join(rr.GOLDEN, "reader.json")))


if __name__ == "__main__":
    main()
