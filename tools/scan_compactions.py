"""Counts the compaction rounds of the screening scan's tile kernel on the data of tests/test_scan_mfma_shape_gpu.py::rising_data,
per matrix instruction (MQ_KNN_OPT_SCAN_MFMA 0 / 1): needs the -DMQ_CLOCK diagnostic build of knn.hip (how to build it:
tools/scan_clock.py), whose kernels write their number of compaction rounds into a debug buffer nothing else reads.
usage: MEERQAT_HIP_LIB=ab/lib_clock.so python tools/scan_compactions.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from test_scan_mfma_shape_gpu import NQ, rising_data
from viquae_amd import _lib
from viquae_amd.index import MI355XFlatIndex

dbg = torch.zeros(3 * 4096, dtype=torch.int64, device="cuda")
os.environ["MQ_DBG_PTR"] = str(dbg.data_ptr())  # read by the diagnostic build at each call
X, Q, Do, Io = rising_data()
idx = MI355XFlatIndex(string_factory="Flat", metric_type=0, screen=True)
idx.add_vectors(X)
out = {"shape": [len(X), X.shape[1], NQ, 100]}
for arm in (0, 1):
    with _lib.knn_option(_lib.KNN_OPT_SCAN_MFMA, arm):
        dbg.zero_()
        D, I = idx.search_batch(Q, 100)
        stats = idx.screen_stats(NQ, 100)
    rounds = dbg.view(-1, 3)[:, 2].cpu().numpy()
    out[f"arm{arm}"] = {"identical_to_oracle": bool(np.array_equal(np.asarray(I), Io) and np.array_equal(np.asarray(D), Do)),
                        "query_tiles_recomputed_exactly": stats[0], "slabs": stats[6], "fullest_pool": stats[3],
                        "workgroups_that_compacted": int((rounds > 0).sum()), "compaction_rounds_per_workgroup": sorted(set(int(r) for r in rounds if r > 0)),
                        "compaction_rounds_total": int(rounds.sum())}
print(json.dumps(out))
