#!/usr/bin/env python3
"""Throughput of the reader stage (viquae_amd/rc/reader.py) on the shape of experiments/rc/viquae/config.yaml:
1,257 test questions, M = 24 passages each, batches of 8 questions (192 pairs), max_length 256; MultiPassageBERT at
bert-base widths (12 layers) with random weights; a synthetic 30,522-entry WordPiece vocabulary (no network), ~130-token
passages and ~20-token questions.

Reports questions/s of the whole job (tokenization, forward, head, normalisation, both span searches, decoding, metrics)
and of the device alone, split into forward (embeddings + 12 layers), QA head, log-softmax and the two span searches.
The head reads hidden states the last layer has just written (139 MB per batch, inside the 256-MB Infinity Cache): it is
timed as it runs in the job AND once more per batch after a 1-GiB write has evicted them ("head_cold": the HBM stream).
    python tools/reader_timing.py [--questions 1257] [--out FILE]
The kernel profile profiles/reader_kernel_stats.csv is the stats file of
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/reader_timing.py --questions 160 --device-batches 10
(10 device batches x 2 passes + 20 job batches = 40 forwards, 40 + 10 head launches; the cold pass runs on the second pass only).
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch


def build_world(root, n_questions, n_passages, M, rng):
    import datasets
    from bench_encode_surface import make_passages, make_vocab
    words, suffixes = make_vocab(os.path.join(root, "tok"), rng)
    passages = make_passages(n_passages, words, suffixes, rng)                     # ~130 word pieces
    questions = make_passages(n_questions, words, suffixes, rng, mean_words=15, sd_words=4)  # ~20 word pieces
    datasets.Dataset.from_dict({"passage": passages, "index": list(range(n_passages))}).save_to_disk(os.path.join(root, "kb"))
    qs = {"id": [f"q{i}" for i in range(n_questions)], "input": questions,
          "output": [{"original_answer": str(w), "answer": [str(w)]} for w in rng.choice(words, n_questions)],
          "search_indices": [rng.choice(n_passages, M, replace=False).tolist() for _ in range(n_questions)],
          "search_scores": [np.sort(rng.uniform(0, 30, M))[::-1].tolist() for _ in range(n_questions)]}
    datasets.DatasetDict({"test": datasets.Dataset.from_dict(qs)}).save_to_disk(os.path.join(root, "dataset"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=1257)
    ap.add_argument("--passages", type=int, default=20000)
    ap.add_argument("--device-batches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import datasets
    from bench_encoders import BERT_BASE, random_bert_state
    from viquae_amd.encoders import MultiPassageBERT, qa_head
    from viquae_amd.rc import reader as R
    datasets.disable_progress_bars()
    M, batch = 24, 8
    rng = np.random.default_rng(0)
    root = tempfile.mkdtemp(prefix="mq_reader_timing_")
    build_world(root, a.questions, a.passages, M, rng)
    state = random_bert_state(BERT_BASE, 0, prefix="bert.")
    g = torch.Generator().manual_seed(1)
    state["qa_outputs.weight"] = torch.randn(2, 768, generator=g) * 0.02
    state["qa_outputs.bias"] = torch.zeros(2)
    dev = torch.device("cuda")
    model = MultiPassageBERT.from_state_dict(dict(BERT_BASE), state).to(dev).eval()
    from transformers import BertTokenizerFast
    tok = BertTokenizerFast.from_pretrained(os.path.join(root, "tok"))
    data = R.ReaderData("BertTokenizerFast", None, kb=os.path.join(root, "kb"), dataset_path=os.path.join(root, "dataset"),
                        M=M, eval_batch_size=batch, tokenization_kwargs={"max_length": 256, "padding": "longest"}, tokenizer=tok)
    split = data.split("test")
    out = {"workload": f"{a.questions} questions x M={M}, batches of {batch}, bert-base (12 layers, random weights), "
                       f"synthetic WordPiece vocabulary, max_length 256", "gemm_mode": os.environ.get("MQ_ENC_GEMM", "split_bf16")}

    # -- device alone, per stage, on real batches already on the device ----------------------------------------------
    batches = []
    for items in list(data.batches(split))[: a.device_batches]:
        b, scores, _ = data.collate(items)
        batches.append(({k: b[k].to(dev) for k in ("input_ids", "attention_mask", "token_type_ids")}, R.shift_weights(scores)))
    Ls = [b["input_ids"].shape[1] for b, _ in batches]
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    stage = {"forward": 0.0, "head": 0.0, "log_softmax": 0.0, "spans": 0.0}
    evict = torch.empty(1 << 28, dtype=torch.float32, device=dev)  # 1 GiB: four times the Infinity Cache
    head_cold, head_bytes = 0.0, 0
    for rep in range(2):  # the first pass warms up
        acc = {k: 0.0 for k in stage}
        for inputs, w in batches:
            N, L = inputs["input_ids"].shape[0] // M, inputs["input_ids"].shape[1]
            e = [ev() for _ in range(5)]
            e[0].record()
            last, _ = model.bert(inputs["input_ids"], inputs["token_type_ids"], inputs["attention_mask"])
            e[1].record()
            logits = qa_head(last.view(N * M * L, -1), model.qa_w, model.qa_b).view(2, N * M, L)
            e[2].record()
            _, _, sp, ep = R.log_softmax_per_question(logits[0], logits[1], N, M, L)
            e[3].record()
            R.best_spans(sp, ep)
            R.best_spans(sp, ep, weights=w)
            e[4].record()
            torch.cuda.synchronize()
            for k, (i, j) in zip(acc, ((0, 1), (1, 2), (2, 3), (3, 4))):
                acc[k] += e[i].elapsed_time(e[j]) / 1e3
            if rep == 1:  # the head once more, its input evicted from the cache first
                evict.fill_(float(rep))
                c = [ev() for _ in range(2)]
                c[0].record()
                qa_head(last.view(N * M * L, -1), model.qa_w, model.qa_b)
                c[1].record()
                torch.cuda.synchronize()
                head_cold += c[0].elapsed_time(c[1]) / 1e3
                head_bytes += last.numel() * 4
        stage = acc
    total = sum(stage.values())
    nq = len(batches) * batch
    out["device"] = {"batches": len(batches), "mean_L": round(float(np.mean(Ls)), 1), "questions_per_s": round(nq / total, 1),
                     "ms_per_batch": {k: round(v / len(batches) * 1e3, 3) for k, v in stage.items()},
                     "share": {k: round(v / total, 4) for k, v in stage.items()},
                     "head_TB_per_s": round(head_bytes / stage["head"] / 1e12, 2),
                     "head_cold": {"ms_per_batch": round(head_cold / len(batches) * 1e3, 3),
                                   "TB_per_s": round(head_bytes / head_cold / 1e12, 2)}}

    # -- the whole job ------------------------------------------------------------------------------------------------
    list(data.batches(split.select(range(16))))  # warm the dataset cache
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = R.evaluate(model, data, "test")
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    out["job"] = {"questions": len(result["predictions"]), "seconds": round(t, 2), "questions_per_s": round(len(result["predictions"]) / t, 1)}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
