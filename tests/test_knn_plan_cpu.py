"""CPU suite: the kNN planner and the argument checks of the two search entries answer what tests/golden/knn_plan.json records
(tools/make_golden_knn_plan.py, minted from the library as it was before the host side of csrc/knn.hip was rebuilt around one
search plan): which scan serves a call, the workspace it needs and the launch geometry for 560 shapes x 3 metrics, the scan kinds
again under each planner switch, and the return code of every kind of call the entries must refuse.  All host arithmetic: no
call here reaches the HIP runtime."""
import json

import pytest

from tools import make_golden_knn_plan as mk


@pytest.fixture(scope="module")
def golden(hip_lib):
    import torch
    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        if cus != mk.CUS:
            pytest.skip(f"the table is for {mk.CUS} CUs, this device has {cus}")
    with open(mk.GOLDEN) as f:
        g = json.load(f)
    assert g["cus"] == mk.CUS and [tuple(g["grid"][a]) for a in ("N", "d", "nq", "k")] == [mk.NS, mk.DS, mk.NQS, mk.KS]
    return g


def _mismatches(shapes, got, want):
    return [(s, a, b) for s, a, b in zip(shapes, got, want) if a != b]


def test_plan_table_at_default_options(hip_lib, golden):
    from viquae_amd import _lib
    shapes = mk.shapes()
    assert len(shapes) == len(golden["default"]) == 560
    for key in (_lib.KNN_OPT_SMALL_SCAN, _lib.KNN_OPT_PARTITIONS):
        assert hip_lib.mq_knn_get_option(key) == 1
    assert hip_lib.mq_knn_get_option(_lib.KNN_OPT_SMALL_MIN_TILES) == 0
    bad = _mismatches(shapes, [mk.plan_row(hip_lib, s) for s in shapes], golden["default"])
    assert not bad, (len(bad), bad[:5])
    # every route is in the table: no screening scan, the tile kernel, the streaming kernel
    kinds = [x for row in golden["default"] for x in row[:3]]
    assert [kinds.count(v) for v in (0, 1, 2)] == [616, 988, 76]


@pytest.mark.parametrize("variant", ["default", "SMALL_SCAN=0", "PARTITIONS=0", "SMALL_MIN_TILES=1"])
def test_scan_kinds_under_each_switch(hip_lib, golden, variant):
    from viquae_amd import _lib
    key, value = mk.option_variants(_lib)[variant]
    shapes = mk.shapes() + mk.FLOOR_SHAPES
    before = [hip_lib.mq_knn_get_option(k) for k in range(5)]
    with _lib.knn_option(key, value):
        got = [mk.scan_kinds(hip_lib, s) for s in shapes]
    assert [hip_lib.mq_knn_get_option(k) for k in range(5)] == before
    bad = _mismatches(shapes, got, golden["scan_kinds"][variant])
    assert not bad, (len(bad), bad[:5])
    if variant == "default":
        assert got[:560] == [row[:3] for row in golden["default"]]
    else:
        assert got != golden["scan_kinds"]["default"]  # the switch reaches the planner


def test_refused_calls_keep_their_return_codes(hip_lib, golden):
    from viquae_amd import _lib
    calls = mk.invalid_calls()
    want = dict(map(tuple, golden["return_codes"]))
    assert [name for name, _, _ in calls] == [name for name, _ in golden["return_codes"]] and len(want) == len(calls)
    # the table itself: nothing but an empty batch is accepted, and no recorded call reached the runtime
    assert all(rc in (-1, -2, -4) or (rc == 0 and "nq = 0" in name) for name, rc in want.items())
    assert {-1, -2, -4, 0} == set(want.values())
    assert want["exact: N = 0, workspace one byte short"] == -2 and want["screened: N = 0, workspace one byte short"] == -1
    assert want["screened: k = 300 over 1.5M rows with the bytes of PARTITIONS = 0"] == -2
    hip_lib.mq_internal_set_hip_error(0)
    got = {name: mk.run_call(hip_lib, _lib, entry, ov) for name, entry, ov in calls}
    assert got == want, {n: (got[n], want[n]) for n in want if got[n] != want[n]}
    assert hip_lib.mq_last_hip_error() == 0
