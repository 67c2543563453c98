"""The clock the chip holds inside the screening scan's tile kernel, per matrix instruction (MQ_KNN_OPT_SCAN_MFMA 0 / 1): needs a
-DMQ_CLOCK build of knn.hip (MEERQAT_HIP_LIB=<that library>), whose kernels stamp s_memtime and s_memrealtime once around their
chunk loop into a debug buffer nothing else reads.  That library is built from the tree (every other object as the ordinary
build leaves it under viquae_amd/csrc/_obj):
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-fast-math -ffp-contract=off -DMQ_CLOCK -c viquae_amd/csrc/knn.hip -o ab/knn_clock.o
    hipcc --offload-arch=gfx950 -shared -fPIC ab/knn_clock.o <viquae_amd/csrc/_obj/*.o except knn.hip.o> -lpthread -o ab/lib_clock.so  Two seconds of back-to-back headline calls per arm first, then the median over
the workgroups of the last call.  usage: MEERQAT_HIP_LIB=ab/lib_clock.so python tools/scan_clock.py"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from viquae_amd import _lib
from viquae_amd.index import MI355XFlatIndex

N, d, nq, k = 1_500_000, 768, 4096, 100
dev = torch.device("cuda")
dbg = torch.zeros(3 * 4096, dtype=torch.int64, device=dev)
os.environ["MQ_DBG_PTR"] = str(dbg.data_ptr())  # read by the diagnostic build at each call
idx = MI355XFlatIndex(string_factory="Flat", metric_type=0, screen=True)
g = torch.Generator(device=dev)
g.manual_seed(0)
for s in range(0, N, 1 << 16):
    idx.add(torch.randn((min(1 << 16, N - s), d), generator=g, device=dev), total_hint=N)
Q = torch.randn((nq, d), generator=g, device=dev)
out = {}
for arm in (0, 1, 0, 1):
    with _lib.knn_option(_lib.KNN_OPT_SCAN_MFMA, arm):
        t0 = time.time()
        while time.time() - t0 < 2.0:
            for _ in range(20):
                idx.search_device(Q, k)
            torch.cuda.synchronize()
        dbg.zero_()
        idx.search_device(Q, k)
        torch.cuda.synchronize()
    t = dbg.view(-1, 3).double()
    t = t[t[:, 1] > 0]
    ghz = (t[:, 0] / t[:, 1] * 0.1).median().item()
    out.setdefault(f"arm{arm}_ghz", []).append(round(ghz, 4))
    out.setdefault(f"arm{arm}_loop_us", []).append(round((t[:, 1] / 100.0).median().item(), 1))
out["workgroups"] = int(t.shape[0])
print(json.dumps(out))
