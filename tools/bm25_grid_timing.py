#!/usr/bin/env python3
"""BM25 parameter grid on the synthetic Zipfian corpus of tools/bm25_timing.py (1M passages x 100 tokens, 256 questions, k = 100,
seeded): milliseconds per batch of questions for a grid of one tile of settings (mq_bm25_grid_tile(), 8 where the library lacks the
entry) and for the reference's default grid of 10 x 30 = 300 settings, scored one of two ways:

    --method loop   per setting, ``set_bm25`` (a new norm cache + one pass of the impact kernel) + ``search_device``; only entries a
                    build without the grid kernel has too, so the same file times a checkout of the commit before it
    --method grid   ``search_grid_device``: one sweep of the postings per tile of settings

Device time between two events on the stream, around the whole grid of one batch; the median and min-max of ``--repeats`` windows
after warm-up.  One JSON line; with ``--out`` the record is filed under ``--label`` in that JSON file (other labels are kept).

    python tools/bm25_grid_timing.py --method grid --label grid --out profiles/bm25_grid_timing.json
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bm25_timing import progress, zipf_corpus, zipf_questions  # noqa: E402


def default_grid():
    """The reference's default search space, b-major then k1 -> [(k1, b)]."""
    return [(float(k1), float(b)) for b in np.arange(0, 1, 0.1).tolist() for k1 in np.arange(0, 3, 0.1).tolist()]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--method", choices=("loop", "grid"), required=True)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--terms", type=int, default=100_000)
    ap.add_argument("--mean-length", type=int, default=100)
    ap.add_argument("--questions", type=int, default=256)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tile-steps", type=int, default=5, help="batches per window for the one-tile grid")
    ap.add_argument("--label")
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from viquae_amd import _lib
    from viquae_amd.ir.bm25 import MI355XBM25Index, norm_cache
    _lib.require_gpu()
    lib = _lib.load()
    tile = int(lib.mq_bm25_grid_tile()) if hasattr(lib, "mq_bm25_grid_tile") else 8
    rng = np.random.default_rng(0)
    flat, lengths = zipf_corpus(rng, a.docs, a.terms, a.mean_length)
    docs = np.split(flat, np.cumsum(lengths)[:-1])
    t0 = time.perf_counter()
    index = MI355XBM25Index()
    index.add_token_ids(docs, a.terms)
    progress(f"index: {len(index.doc)} postings ({time.perf_counter() - t0:.1f} s)")
    del docs, flat
    questions = zipf_questions(rng, a.questions, a.terms)
    dev = index._torch_device
    qptr, cterm, cweight = (torch.from_numpy(x).to(dev) for x in index.pack_clauses(questions))
    grids = {"tile": default_grid()[137:137 + tile], "default_300": default_grid()}

    def run(params):
        if a.method == "loop":
            for k1, b in params:
                index.set_bm25(k1, b)
                index.search_device(qptr, cterm, cweight, a.k)
        else:
            caches = torch.from_numpy(np.stack([norm_cache(k1, b, index.avgdl) for k1, b in params])).to(dev)
            index.search_grid_device(qptr, cterm, cweight, caches, a.k)

    def window(params, steps):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(steps):
            run(params)
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / steps

    record = {"method": a.method, "corpus": {"documents": a.docs, "terms": a.terms, "postings": len(index.doc)},
              "questions": a.questions, "clauses": int(cterm.numel()), "k": a.k, "repeats": a.repeats, "tile": tile,
              "workspace_budget_bytes": index.workspace_bytes, "library": lib.mq_version().decode(), "gpu": torch.cuda.get_device_name(0)}
    for name, params in grids.items():
        steps = a.tile_steps if name == "tile" else 1
        window(params, 1)  # warm-up: workspace allocation, code objects
        ms = sorted(window(params, steps) for _ in range(a.repeats))
        record[name] = {"settings": len(params), "steps_per_window": steps, "ms_per_batch": round(statistics.median(ms), 3),
                        "ms_min_max": [round(ms[0], 3), round(ms[-1], 3)],
                        "ms_per_setting": round(statistics.median(ms) / len(params), 4)}
        progress(f"{a.method} {name}: {record[name]}")
    line = json.dumps(record)
    print(line)
    if a.out:
        filed = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                filed = json.load(f)
        filed[a.label or a.method] = record
        with open(a.out, "w") as f:
            json.dump(filed, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
