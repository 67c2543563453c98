"""Step 5 of the reader (meerqat/models/qa.py:18-77, get_best_spans) restated in numpy, and the seeded pieces the reader
tests rebuild from tests/golden/reader.json: the MultiPassageBERT weights and the on-disk world (vocabulary, knowledge
base, questions, run) of the end-to-end test.  Not a test module."""
import hashlib
import json
import os

import numpy as np

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TINY = dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, max_position_embeddings=512,
            type_vocab_size=2, layer_norm_eps=1e-12)
BASE2 = dict(hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=512,
             type_vocab_size=2, layer_norm_eps=1e-12)


def candidates(start_probs, end_probs, weights=None, cannot_be_first_token=True):
    """P[n, m, i, j] = fl(fl(s_i e_j) w_m) for i <= j, 0 below the diagonal and (cannot_be_first_token) in row i = 0."""
    s = np.asarray(start_probs, dtype=F32)
    e = np.asarray(end_probs, dtype=F32)
    N, M, L = s.shape
    row, col = np.arange(L)[:, None], np.arange(L)[None, :]
    allowed = (row <= col) & (row >= (1 if cannot_be_first_token else 0))
    P = np.where(allowed, s[..., :, None] * e[..., None, :], F32(0))
    if weights is not None:
        P = P * np.asarray(weights, dtype=F32).reshape(N, M)[..., None, None]
    return P


def best_spans(start_probs, end_probs, weights=None, cannot_be_first_token=True):
    """(passage, start, end exclusive) int64 [N]: among the candidates equal to the question's largest one, the lowest
    (passage, start, end) in lexicographic order -- i.e. the first passage reaching the maximum, then the first flat index
    i * L + j inside it."""
    s = np.asarray(start_probs, dtype=F32)
    N, M, L = s.shape
    out = np.zeros((3, N), dtype=np.int64)
    for q in range(N):
        w = None if weights is None else np.asarray(weights, dtype=F32).reshape(N, M)[q: q + 1]
        P = candidates(s[q: q + 1], np.asarray(end_probs, dtype=F32)[q: q + 1], w, cannot_be_first_token)[0]
        m, i, j = np.argwhere(P == P.max())[0]  # argwhere lists hits in (m, i, j) order
        out[:, q] = m, i, j + 1
    return out


def best_and_runner_up(start_probs, end_probs, weights=None, cannot_be_first_token=True):
    """fp32 [2, N]: the winning candidate's score and the largest score of any OTHER (passage, start, end) triple."""
    s = np.asarray(start_probs, dtype=F32)
    N, M, L = s.shape
    spans = best_spans(start_probs, end_probs, weights, cannot_be_first_token)
    out = np.zeros((2, N), dtype=F32)
    for q in range(N):
        w = None if weights is None else np.asarray(weights, dtype=F32).reshape(N, M)[q: q + 1]
        flat = candidates(s[q: q + 1], np.asarray(end_probs, dtype=F32)[q: q + 1], w, cannot_be_first_token)[0].reshape(-1)
        g = spans[0, q] * L * L + spans[1, q] * L + spans[2, q] - 1
        out[0, q] = flat[g]
        flat[g] = -1
        out[1, q] = flat.max()
    return out


def shift_weights(scores):
    """get_best_spans' in-place shift: + (1 - min) in fp32 when the batch-wide minimum is below 1."""
    w = np.array(scores, dtype=F32, copy=True)
    m = w.min()
    if m < 1:
        w += F32(1) - m
    return w


def planted_cases():
    """Small span-search cases with exact ties (across passages, inside one), all-zero passages, denormal products, weights
    below and above 1, M = 1 and both cannot_be_first_token values: lists, for a JSON golden."""
    cases = []
    # ties across passages: passages 0 and 2 equal, passage 1 smaller; and inside one passage (several (i, j) of equal value)
    s = np.array([[[0, .5, .5, 0, 0, 0], [0, .25, 0, .25, 0, 0], [0, .5, .5, 0, 0, 0]]], F32)
    e = np.array([[[0, 0, .5, .5, 0, 0], [0, 0, .5, .5, 0, 0], [0, 0, .5, .5, 0, 0]]], F32)
    for cbf in (True, False):
        cases.append(dict(start=s.tolist(), end=e.tolist(), weights=None, cannot_be_first_token=cbf))
    # the best candidate sits in row 0 (only taken when cannot_be_first_token is False)
    s0 = np.array([[[.9, .01, .02, .03], [.1, .1, .1, .1]]], F32)
    e0 = np.array([[[.9, .01, .02, .04], [.1, .1, .1, .1]]], F32)
    for cbf in (True, False):
        cases.append(dict(start=s0.tolist(), end=e0.tolist(), weights=None, cannot_be_first_token=cbf))
    # all-zero passages; a question whose every candidate is 0 -> (0, 0, 1)
    z = np.zeros((2, 3, 5), F32)
    z[1, 2, 3] = .5
    z2 = z.copy()
    z2[1, 2, 4] = .5
    cases.append(dict(start=z.tolist(), end=z2.tolist(), weights=None, cannot_be_first_token=True))
    # denormal products (1e-20 * 1e-21 ~ 1e-41), distinct and tied
    d = np.array([[[0, 1e-20, 3e-20, 3e-20], [0, 2e-20, 1e-20, 1e-22]]], F32)
    d2 = np.array([[[0, 1e-21, 1e-21, 2e-21], [0, 1e-21, 3e-21, 1e-21]]], F32)
    cases.append(dict(start=d.tolist(), end=d2.tolist(), weights=None, cannot_be_first_token=True))
    cases.append(dict(start=d.tolist(), end=d2.tolist(), weights=[[1.5, 1.0]], cannot_be_first_token=True))
    # weights below and above 1 (already shifted by the caller: the reference shifts them in place first)
    rng = np.random.default_rng(5)
    p = rng.random((2, 4, 7)).astype(F32)
    q = rng.random((2, 4, 7)).astype(F32)
    for w in ([[0.25, 3.0, 1.0, 0.5], [2.0, 2.0, 0.1, 7.0]], [[1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]]):
        cases.append(dict(start=p.tolist(), end=q.tolist(), weights=w, cannot_be_first_token=True))
    # M = 1
    cases.append(dict(start=p[:, :1].tolist(), end=q[:, :1].tolist(), weights=None, cannot_be_first_token=True))
    cases.append(dict(start=p[:, :1].tolist(), end=q[:, :1].tolist(), weights=[[4.0], [0.5]], cannot_be_first_token=False))
    return cases


# --------------------------------------------------------------------------------------------------
# seeded weights
# --------------------------------------------------------------------------------------------------
def reader_shapes(cfg, vocab_size):
    from oracle import encoders as oe
    c = dict(cfg, vocab_size=vocab_size)
    shapes = oe.bert_param_shapes(c, prefix="bert.")
    shapes["qa_outputs.weight"] = (2, cfg["hidden_size"])
    shapes["qa_outputs.bias"] = (2,)
    return shapes


def reader_state(cfg, vocab_size, seed):
    """name -> fp32 array of a BertForQuestionAnswering, drawn from numpy default_rng(seed) (oracle.encoders.seeded_state)."""
    from oracle import encoders as oe
    return oe.seeded_state(reader_shapes(cfg, vocab_size), seed)


def state_checksum(state):
    h = hashlib.sha256()
    for name in sorted(state):
        h.update(name.encode())
        h.update(np.ascontiguousarray(state[name], dtype=F32).tobytes())
    return h.hexdigest()


def hf_config(cfg, vocab_size):
    return dict(cfg, vocab_size=vocab_size, model_type="bert", architectures=["BertForQuestionAnswering"], hidden_act="gelu",
                hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, position_embedding_type="absolute", num_labels=2)


def write_checkpoint(path, cfg, vocab_size, seed):
    """A save_pretrained-style directory (config.json + pytorch_model.bin) of the seeded reader."""
    import torch
    os.makedirs(path, exist_ok=True)
    state = reader_state(cfg, vocab_size, seed)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(hf_config(cfg, vocab_size), f)
    torch.save({k: torch.from_numpy(v) for k, v in state.items()}, os.path.join(path, "pytorch_model.bin"))
    return state


# --------------------------------------------------------------------------------------------------
# the world of the end-to-end test
# --------------------------------------------------------------------------------------------------
def make_world(seed=0, n_words=600, n_passages=80, n_questions=16, M=24):
    """vocabulary, passages, questions (with search_indices / search_scores, some with fewer than M results or none) and the
    same results as a JSON run.  Deterministic in the arguments."""
    rng = np.random.default_rng(seed)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    words = set()
    while len(words) < n_words:
        words.add("".join(rng.choice(letters, int(rng.integers(3, 8)))))
    words = sorted(words)
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(10)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words
    vocab += ["##" + w for w in words[:40]] + [".", ",", "'", "?", "the", "a", "an"]
    passages = []
    for i in range(n_passages):
        n = int(rng.integers(12, 70)) if i != 7 else 260  # passage 7 is truncated at max_length
        toks = list(rng.choice(words, n))
        for k in rng.choice(n, max(1, n // 10), replace=False):
            toks[k] = str(rng.choice(["the", "a", "an"])) + " " + toks[k]
        passages.append(" ".join(toks) + ".")
    questions = []
    for q in range(n_questions):
        n_res = {9: 0, 12: 5, 14: 17}.get(q, M + 6)  # ragged (second batch): no result, fewer than M
        ids = rng.choice(n_passages, n_res, replace=False).tolist()
        scores = np.sort(rng.uniform(-6.0, 12.0, n_res).astype(F32))[::-1].tolist()
        if q >= 8:
            scores = [s + 5.0 for s in scores]  # the second batch has another minimum: another shift
        rel = passages[ids[0]].rstrip(".").split() if ids else words[:3]
        k = int(rng.integers(0, max(1, len(rel) - 2)))
        answer = " ".join(rel[k: k + 2])
        questions.append({
            "id": f"q{q:02d}",
            "input": " ".join(rng.choice(words, int(rng.integers(5, 12)))) + "?",
            "output": {"original_answer": answer, "answer": [answer, answer.upper() + "!", str(rng.choice(words))]},
            "search_indices": [int(i) for i in ids],
            "search_scores": [float(s) for s in scores],
        })
    run = {q["id"]: {str(i): s for i, s in zip(q["search_indices"], q["search_scores"])} for q in questions}
    return {"vocab": vocab, "passages": passages, "questions": questions, "run": run}


def write_world(root, world):
    """tokenizer (vocab.txt), kb and dataset (datasets.save_to_disk) and run.json under ``root`` -> their paths."""
    import datasets
    paths = {k: os.path.join(root, k) for k in ("tokenizer", "kb", "dataset")}
    paths["run"] = os.path.join(root, "run.json")
    os.makedirs(paths["tokenizer"], exist_ok=True)
    with open(os.path.join(paths["tokenizer"], "vocab.txt"), "w") as f:
        f.write("\n".join(world["vocab"]) + "\n")
    datasets.Dataset.from_dict({"passage": world["passages"], "index": list(range(len(world["passages"])))}).save_to_disk(paths["kb"])
    qs = world["questions"]
    test = datasets.Dataset.from_dict({k: [q[k] for q in qs] for k in qs[0]})
    datasets.DatasetDict({"test": test}).save_to_disk(paths["dataset"])
    with open(paths["run"], "w") as f:
        json.dump(world["run"], f)
    return paths


def load_golden():
    with open(os.path.join(GOLDEN, "reader.json")) as f:
        return json.load(f)
