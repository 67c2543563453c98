"""The planted world of the BM25 parameter-search tests (tests/test_bm25_hp_gpu.py, conditions in tests/test_bm25_grid_cpu.py): 48
questions over 144 passages in which the length normalisation decides the rank of the only relevant passage.  For question i:
    passage 3i     ``alpha{i} beta{i}`` + 120 filler words ``w{(7i+j) % 97}``
    passage 3i+1   ``alpha{i} beta{i} gold{i}`` + (10 + 7 (i % 12)) filler words ``w{(13i+j) % 97}``     -- the relevant one
    passage 3i+2   ``alpha{i}`` repeated 2 + i % 3 times
    question       ``who mentions alpha{i} beta{i}``, answer ``gold{i}``
and the grid b in {0, 0.5, 1.0} x k1 in {0, 0.4, 1.2, 2.9}, k = 10."""
import numpy as np

from tests import bm25_restatement as br

NQ, K = 48, 10
HYP_HYP = {"b": {"bounds": [0, 1.5], "step": 0.5}, "k1": {"values": [0, 0.4, 1.2, 2.9]}}
GRID = [(b, k1) for b in (0.0, 0.5, 1.0) for k1 in (0.0, 0.4, 1.2, 2.9)]   # b-major, then k1


def passages(nq=NQ):
    out = []
    for i in range(nq):
        out.append(" ".join([f"alpha{i}", f"beta{i}"] + [f"w{(7 * i + j) % 97}" for j in range(120)]))
        out.append(" ".join([f"alpha{i}", f"beta{i}", f"gold{i}"] + [f"w{(13 * i + j) % 97}" for j in range(10 + 7 * (i % 12))]))
        out.append(" ".join([f"alpha{i}"] * (2 + i % 3)))
    return out


def questions(nq=NQ):
    return [f"who mentions alpha{i} beta{i}" for i in range(nq)]


def restated_mrr(nq=NQ, k=K):
    """mrr@k of every grid point, from the numpy restatement alone -> list in grid order."""
    tokens = [br.tokenize(t) for t in passages(nq)]
    vocabulary = sorted({t for doc in tokens for t in doc})
    term_id = {t: i for i, t in enumerate(vocabulary)}
    docs = [np.array([term_id[t] for t in doc], dtype=np.int64) for doc in tokens]
    qs = [[term_id.get(t, -1) for t in br.tokenize(q)] for q in questions(nq)]
    rest = br.Restatement(docs, len(vocabulary))
    values = []
    for b, k1 in GRID:
        rest.set_bm25(k1, b)
        _, I = rest.search(qs, k)
        rr = [1.0 / (int(np.flatnonzero(I[i] == 3 * i + 1)[0]) + 1) if (I[i] == 3 * i + 1).any() else 0.0 for i in range(nq)]
        values.append(float(np.mean(rr)))
    return values


def build(root, nq=NQ, n_test=20):
    """Writes the KB (``data/meerqat_passages``, the path the shipped config names), the train split and a test split (the first
    ``n_test`` questions) under ``root`` -> (train path, test path)."""
    import os
    import datasets
    datasets.Dataset.from_dict({"passage": passages(nq)}).save_to_disk(os.path.join(root, "data", "meerqat_passages"))
    rows = {"id": [f"q{i}" for i in range(nq)], "input": questions(nq),
            "output": [{"original_answer": f"gold{i}", "answer": [f"gold{i}"]} for i in range(nq)]}
    train, test = os.path.join(root, "train"), os.path.join(root, "test")
    datasets.Dataset.from_dict(rows).save_to_disk(train)
    datasets.Dataset.from_dict({name: column[:n_test] for name, column in rows.items()}).save_to_disk(test)
    return train, test
