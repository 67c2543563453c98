"""A/B of the tile kernel's two matrix instructions (MQ_KNN_OPT_SCAN_MFMA: 0 = 32x32x16, 1 = 16x16x32) on ONE device in ONE process:
interleaved rounds of the headline call (4096 queries x 1.5M x 768, inner product, k = 100), HIP events around the scan kernel and
around the whole call.  Prints one JSON line; usage: python tools/ab_scan_mfma.py [rounds=5] [steps=20] [d=768] [k=100]

The rule the default follows (profiles/r07_notes.md): arm 1 wins only if the median of its rounds' median step times is lower than
arm 0's by more than arm 0's own min-to-max spread over its rounds."""
import json
import os
import statistics as st
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from viquae_amd import _lib
from viquae_amd.index import MI355XFlatIndex

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
d = int(sys.argv[3]) if len(sys.argv) > 3 else 768
k = int(sys.argv[4]) if len(sys.argv) > 4 else 100
N, nq = 1_500_000, 4096
dev = torch.device("cuda")
lib = _lib.load()
idx = MI355XFlatIndex(string_factory="Flat", metric_type=0, screen=True)
g = torch.Generator(device=dev)
g.manual_seed(0)
for s in range(0, N, 1 << 16):
    idx.add(torch.randn((min(1 << 16, N - s), d), generator=g, device=dev), total_hint=N)
Q = torch.randn((nq, d), generator=g, device=dev)
D, I = idx.search_device(Q, k)
torch.cuda.synchronize()
ws, stream = idx._ws, torch.cuda.current_stream()


def call(scan_begin, scan_end):
    _lib.check(lib.mq_knn_search_screened_f32(
        idx._packed.data_ptr() if idx._packed is not None else None, idx._sqnorm.data_ptr(), idx._rowmajor.data_ptr(),
        idx._bf16.data_ptr(), idx._xmax2.data_ptr(), N, d, Q.data_ptr(), nq, k, 0, 0, 0, D.data_ptr(), I.data_ptr(), ws.data_ptr(),
        ws.numel(), stream.cuda_stream, scan_begin.cuda_event, scan_end.cuda_event))


def ev():
    return torch.cuda.Event(enable_timing=True)


def one_round(arm):
    with _lib.knn_option(_lib.KNN_OPT_SCAN_MFMA, arm):
        evs = [(ev(), ev(), ev(), ev()) for _ in range(steps + 2)]
        for a, b, c, e in evs:  # (events are created by their first record: keep that out of the timed calls)
            a.record(stream); b.record(stream); c.record(stream); e.record(stream)
        torch.cuda.synchronize()
        for a, b, c, e in evs:
            a.record(stream)
            call(b, c)
            e.record(stream)
        torch.cuda.synchronize()
        res = (D.clone(), I.clone(), idx.screen_stats(nq, k)[0])
    timed = evs[2:]  # two warm-up calls per round: the clock settles on the arm's own load
    return [b.elapsed_time(c) for a, b, c, e in timed], [a.elapsed_time(e) for a, b, c, e in timed], res


per = {0: {"scan": [], "step": []}, 1: {"scan": [], "step": []}}
results = {}
for r in range(rounds):
    for arm in ((0, 1) if r % 2 == 0 else (1, 0)):
        scan, step, res = one_round(arm)
        per[arm]["scan"].append(st.median(scan))
        per[arm]["step"].append(st.median(step))
        results[arm] = res
out = {"shape": [N, d, nq, k], "rounds": rounds, "steps": steps, "device": torch.cuda.get_device_name(0)}
for arm in (0, 1):
    for what in ("scan", "step"):
        v = per[arm][what]
        out[f"arm{arm}_{what}_ms"] = {"median": round(st.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                                      "rounds": [round(x, 4) for x in v]}
out["results_identical_between_arms"] = bool(torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]))
out["query_tiles_recomputed_exactly"] = [results[0][2], results[1][2]]
spread0 = max(per[0]["step"]) - min(per[0]["step"])
gain = st.median(per[0]["step"]) - st.median(per[1]["step"])
out["arm0_step_spread_ms"] = round(spread0, 4)
out["arm1_step_gain_ms"] = round(gain, 4)
out["arm1_wins"] = bool(gain > spread0)
print(json.dumps(out))
