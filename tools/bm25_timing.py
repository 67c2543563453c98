#!/usr/bin/env python3
"""BM25 search (viquae_amd.ir.bm25.MI355XBM25Index) on a synthetic Zipfian corpus: milliseconds per batch of 256 questions -- the
device time of the search entry alone (events around mq_bm25_search_f32: scoring + top-k of every query chunk) and the host call
``search_batch`` around it (clause packing, copies, one synchronisation) -- and the postings bytes the scoring kernel sweeps per
second (8 bytes per posting of every clause: document id + impact) against the HBM peak.  That rate is a whole-search figure, not a
kernel's share of peak: the same time also pays for the dense score matrix (written once, read by each selection pass) and for the
top-k.  Seeded; one JSON line.  Each figure is the median of ``--repeats`` windows of ``--steps`` batches after warm-up.

    python tools/bm25_timing.py [--docs 1000000] [--terms 100000] [--mean-length 100] [--questions 256] [--k 100]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK, HBM_MEASURED = 8.0e12, 6.29e12   # bytes/s: the datasheet figure and a float4 copy on the MI355X


def progress(what):
    print(what, file=sys.stderr, flush=True)


def zipf_corpus(rng, docs, terms, mean_length):
    """Flat term ids of `docs` documents (lengths uniform in [mean/5, 9 mean/5]) drawn from a Zipfian (s = 1) vocabulary."""
    lengths = rng.integers(max(1, mean_length // 5), mean_length * 9 // 5 + 1, size=docs)
    cdf = np.cumsum(1.0 / np.arange(1, terms + 1))
    flat = np.searchsorted(cdf, rng.random(int(lengths.sum())) * cdf[-1]).astype(np.int64)
    return flat, lengths


def zipf_questions(rng, n, terms, mean_terms=12):
    """Questions of about `mean_terms` terms from the same distribution: the commonest terms ("the / of / in") come up in most."""
    cdf = np.cumsum(1.0 / np.arange(1, terms + 1))
    return [np.searchsorted(cdf, rng.random(int(m)) * cdf[-1]).tolist() for m in rng.integers(mean_terms // 2, mean_terms * 3 // 2 + 1, size=n)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--terms", type=int, default=100_000)
    ap.add_argument("--mean-length", type=int, default=100)
    ap.add_argument("--questions", type=int, default=256)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from viquae_amd import _lib
    from viquae_amd.ir.bm25 import MI355XBM25Index
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    flat, lengths = zipf_corpus(rng, a.docs, a.terms, a.mean_length)
    docs = np.split(flat, np.cumsum(lengths)[:-1])
    progress(f"corpus: {a.docs} documents, {flat.size} tokens ({time.perf_counter() - t0:.1f} s)")
    t0 = time.perf_counter()
    index = MI355XBM25Index()
    index.add_token_ids(docs, a.terms)
    build_s = time.perf_counter() - t0
    nnz = len(index.doc)
    progress(f"index: {nnz} postings ({build_s:.1f} s)")
    del docs, flat

    questions = zipf_questions(rng, a.questions, a.terms)
    qptr, cterm, cweight = index.pack_clauses(questions)
    swept = int(index.doc_freq[cterm].sum()) * 8
    dev = index._torch_device
    qptr_d, cterm_d, cweight_d = (torch.from_numpy(x).to(dev) for x in (qptr, cterm, cweight))

    def device_window():
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(a.steps):
            index.search_device(qptr_d, cterm_d, cweight_d, a.k)
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / a.steps

    def host_window():
        t = time.perf_counter()
        for _ in range(a.steps):
            index.search_batch(questions, a.k)
        return (time.perf_counter() - t) * 1e3 / a.steps

    for _ in range(2):
        index.search_batch(questions, a.k)
    device = sorted(device_window() for _ in range(a.repeats))
    host = sorted(host_window() for _ in range(a.repeats))
    # re-weighting the resident index: one pass of the impact kernel
    t = time.perf_counter()
    index.set_bm25(0.5, 0.3)
    reweight_ms = (time.perf_counter() - t) * 1e3
    med = statistics.median(device)
    result = {
        "corpus": {"documents": a.docs, "terms": a.terms, "tokens": int(index.sum_total_term_freq), "postings": nnz, "zipf_s": 1.0},
        "index_bytes_per_posting_on_device": 12, "index_build_host_s": round(build_s, 1),
        "questions": a.questions, "clauses": int(len(cterm)), "k": a.k, "steps": a.steps, "repeats": a.repeats,
        "query_chunk": index.query_chunk(a.questions), "workspace_budget_bytes": index.workspace_bytes,
        "device_ms_per_batch": round(med, 3), "device_ms_min_max": [round(device[0], 3), round(device[-1], 3)],
        "search_batch_ms_per_batch": round(statistics.median(host), 3), "search_batch_ms_min_max": [round(host[0], 3), round(host[-1], 3)],
        "postings_bytes_swept_per_batch": swept,
        "postings_bytes_per_s": round(swept / (med * 1e-3), 1),
        "fraction_of_hbm_peak": round(swept / (med * 1e-3) / HBM_PEAK, 4),
        "fraction_of_measured_copy_rate": round(swept / (med * 1e-3) / HBM_MEASURED, 4),
        "set_bm25_ms": round(reweight_ms, 3),
        "library": _lib.load().mq_version().decode(), "gpu": torch.cuda.get_device_name(0),
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
