"""Mints tests/golden/knn_plan.json: what the kNN planner of libmeerqat_hip.so answers, and what the two search entries return
for calls they must refuse, as recorded from the library built at the commit BEFORE the host side of csrc/knn.hip was
reorganised around one search plan.  tests/test_knn_plan_cpu.py asserts the same answers of the current library.

Everything here runs without a GPU: the planner entries are host arithmetic (the CU count falls back to 256, the MI355X's own),
and every recorded search call is refused by validation before any HIP call -- so the placeholder pointers are never read.

    python tools/make_golden_knn_plan.py            # writes the table from the library in the tree
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "knn_plan.json")

NS = (255, 20000, 70000, 1500000)
DS = (64, 767, 768, 2048)
NQS = (19, 20, 256, 257, 4096)
KS = (100, 128, 129, 224, 225, 1792, 1793)
METRICS = (0, 1, 2)
CUS = 256  # the table's CU count
# Beside the grid, for the scan kinds only: 65,300 rows are 2041 tiles of 32 rows, under the streaming scan's default floor of 8 per
# workgroup (2048) and over a floor of 1 (256) -- the one switch whose value no grid shape feels (20,000 rows are fewer than the
# 256 chunks of 256 rows the streaming scan needs at any floor; 70,000 rows clear the default floor)
FLOOR_SHAPES = [(65300, 64, 256, 100), (65300, 768, 256, 128)]


def shapes():
    return list(itertools.product(NS, DS, NQS, KS))


def option_variants(_lib):
    """name -> (option key, value) of the variants whose scan kinds are recorded beside the defaults'"""
    return {"default": (_lib.KNN_OPT_SMALL_SCAN, 1), "SMALL_SCAN=0": (_lib.KNN_OPT_SMALL_SCAN, 0), "PARTITIONS=0": (_lib.KNN_OPT_PARTITIONS, 0),
            "SMALL_MIN_TILES=1": (_lib.KNN_OPT_SMALL_MIN_TILES, 1)}


def scan_kinds(lib, shape):
    return [int(lib.mq_knn_screen_scan_kind(*shape, m)) for m in METRICS]


def plan_row(lib, shape):
    """[scan kind x 3 metrics, workspace bytes x 3 metrics, workspace bytes of either metric, the 8 launch-info words]"""
    info = (ctypes.c_int64 * 8)()
    assert lib.mq_knn_launch_info(*shape, info) == 0
    return (scan_kinds(lib, shape) + [int(lib.mq_knn_workspace_bytes_metric(*shape, m)) for m in METRICS]
            + [int(lib.mq_knn_workspace_bytes(*shape))] + [int(x) for x in info])


# ---- calls the search entries must refuse ---------------------------------------------------------------------------------
EXACT_ARGS = ("packed", "sqnorm", "N", "d", "queries", "nq", "k", "metric", "flags", "id_offset", "D", "I", "ws", "ws_bytes", "stream")
SCREENED_ARGS = ("packed", "sqnorm", "rowmajor", "bf16", "xstats", "N", "d", "queries", "nq", "k", "metric", "flags", "id_offset",
                 "D", "I", "ws", "ws_bytes", "stream", "ev0", "ev1")
POINTERS = {"exact": ("packed", "sqnorm", "queries", "D", "I", "ws"),
            "screened": ("sqnorm", "rowmajor", "bf16", "xstats", "queries", "D", "I", "ws")}  # (a screened index may keep no panel copy)
BASE = dict(N=20000, d=64, nq=256, k=100, metric=0, flags=0, id_offset=0)
SHORT = "one byte short"    # ws_bytes: one less than mq_knn_workspace_bytes_metric of the call
NO_RANGES = "no row ranges"  # ws_bytes: what mq_knn_workspace_bytes reports with MQ_KNN_OPT_PARTITIONS = 0


def invalid_calls():
    """[(name, entry, overrides)]: every call ends in validation.  Calls that are otherwise valid get a workspace one byte short,
    so that the last check refuses them too (MQ_EWORKSPACE then proves that every earlier check passed)."""
    calls = []
    for entry in ("exact", "screened"):
        calls += [
            (f"{entry}: a valid call, workspace one byte short", entry, dict(ws_bytes=SHORT)),
            (f"{entry}: unknown flag bit", entry, dict(flags=32)),
            (f"{entry}: unknown flag bit, high", entry, dict(flags=1 << 20)),
            (f"{entry}: bad metric 3", entry, dict(metric=3)),
            (f"{entry}: bad metric -1", entry, dict(metric=-1)),
            (f"{entry}: centred inner product", entry, dict(metric=2, ws_bytes=SHORT)),
            (f"{entry}: phase flags", entry, dict(flags=8 | 16, ws_bytes=SHORT)),
            (f"{entry}: k = 2049", entry, dict(k=2049)),
            (f"{entry}: k = 2048, workspace one byte short", entry, dict(k=2048, ws_bytes=SHORT)),
            (f"{entry}: k = 0", entry, dict(k=0)),
            (f"{entry}: d = 0", entry, dict(d=0)),
            (f"{entry}: nq = -1", entry, dict(nq=-1)),
            (f"{entry}: N = -1", entry, dict(N=-1)),
            (f"{entry}: N = 2^32 - 1", entry, dict(N=2 ** 32 - 1)),
            (f"{entry}: N = 2^32 - 2, workspace one byte short", entry, dict(N=2 ** 32 - 2, ws_bytes=SHORT)),
            (f"{entry}: nq = 0", entry, dict(nq=0)),
            (f"{entry}: nq = 0 and nothing else valid", entry,
             dict(nq=0, k=5000, N=-1, d=0, metric=7, flags=1 << 20, ws_bytes=0, **{p: None for p in POINTERS[entry]})),
            (f"{entry}: N = 0, workspace one byte short", entry, dict(N=0, ws_bytes=SHORT)),
            (f"{entry}: N = 0, workspace of zero bytes", entry, dict(N=0, ws_bytes=0)),
            # precedence: MQ_EINVAL before MQ_EUNSUPPORTED before MQ_EWORKSPACE
            (f"{entry}: null queries and k = 2049", entry, dict(queries=None, k=2049)),
            (f"{entry}: unknown flag bit and N = 2^32 - 1", entry, dict(flags=64, N=2 ** 32 - 1)),
            (f"{entry}: k = 2049 and workspace of zero bytes", entry, dict(k=2049, ws_bytes=0)),
            (f"{entry}: N = 2^32 - 1 and workspace of zero bytes", entry, dict(N=2 ** 32 - 1, ws_bytes=0)),
            (f"{entry}: L2, 19 queries, workspace one byte short", entry, dict(metric=1, nq=19, ws_bytes=SHORT)),
            (f"{entry}: k = 1800, workspace one byte short", entry, dict(k=1800, ws_bytes=SHORT)),
        ]
        calls += [(f"{entry}: null {p}", entry, {p: None}) for p in POINTERS[entry]]
    calls += [
        ("screened: null packed (no panel copy), workspace one byte short", "screened", dict(packed=None, ws_bytes=SHORT)),
        # row ranges need their scratch behind the plain workspace: without it the call is refused, not served by exact rounds
        ("screened: k = 300 over 1.5M rows with the bytes of PARTITIONS = 0", "screened",
         dict(N=1500000, d=768, nq=256, k=300, ws_bytes=NO_RANGES)),
        ("screened: k = 300 over 1.5M rows, L2, 4096 queries, with the bytes of PARTITIONS = 0", "screened",
         dict(N=1500000, d=768, nq=4096, k=300, metric=1, ws_bytes=NO_RANGES)),
        ("screened: k = 300 over 1.5M rows, workspace one byte short", "screened", dict(N=1500000, d=768, nq=256, k=300, ws_bytes=SHORT)),
    ]
    return calls


def run_call(lib, _lib, entry, overrides):
    """Return code of one call of invalid_calls() (row ranges switched on for the call: the default)."""
    buf = ctypes.create_string_buffer(4096)
    place = (ctypes.addressof(buf) + 255) & ~255  # non-null, aligned, never read: validation refuses the call
    a = dict(BASE, stream=None, ev0=None, ev1=None)
    a.update({p: place for p in ("packed", "sqnorm", "rowmajor", "bf16", "xstats", "queries", "D", "I", "ws")})
    a.update({key: v for key, v in overrides.items() if key != "ws_bytes"})
    with _lib.knn_option(_lib.KNN_OPT_PARTITIONS, 1):
        want = overrides.get("ws_bytes", SHORT)
        if want == SHORT:
            full = int(lib.mq_knn_workspace_bytes_metric(a["N"], a["d"], a["nq"], a["k"], a["metric"]))
            want = max(full - 1, 0)  # (0: the size entry itself refuses the shape)
        elif want == NO_RANGES:
            with _lib.knn_option(_lib.KNN_OPT_PARTITIONS, 0):
                want = int(lib.mq_knn_workspace_bytes(a["N"], a["d"], a["nq"], a["k"]))
        a["ws_bytes"] = want
        if entry == "exact":
            return int(lib.mq_knn_search_f32(*[a[n] for n in EXACT_ARGS]))
        return int(lib.mq_knn_search_screened_f32(*[a[n] for n in SCREENED_ARGS]))


def table(lib, _lib):
    out = {"cus": CUS, "grid": {"N": NS, "d": DS, "nq": NQS, "k": KS},
           "columns": "scan kind of metric 0, 1, 2 | workspace bytes of metric 0, 1, 2 | workspace bytes | launch info [8]",
           "default": [plan_row(lib, s) for s in shapes()], "scan_kinds": {}}
    for name, (key, value) in option_variants(_lib).items():
        with _lib.knn_option(key, value):
            out["scan_kinds"][name] = [scan_kinds(lib, s) for s in shapes() + FLOOR_SHAPES]
    out["return_codes"] = [[name, run_call(lib, _lib, entry, ov)] for name, entry, ov in invalid_calls()]
    # nothing but an empty batch gets past validation (MQ_EHIP = a call reached the runtime)
    assert all(rc in (-1, -2, -4) or (rc == 0 and "nq = 0" in name) for name, rc in out["return_codes"]), out["return_codes"]
    return out


def main():
    from viquae_amd import _lib
    lib = _lib.load()
    t = table(lib, _lib)
    with open(GOLDEN, "w") as f:
        f.write(json.dumps(t, separators=(",", ":")).replace('],[', '],\n[') + "\n")
    kinds = [x for row in t["default"] for x in row[:3]]
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes;", len(t["default"]), "shapes; none / tile / stream =",
          [kinds.count(v) for v in (0, 1, 2)], "; return codes:", sorted({rc for _, rc in t["return_codes"]}))


if __name__ == "__main__":
    main()
