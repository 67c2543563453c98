"""What tests/test_topk_rows_gpu.py takes for granted about its cases (tests/topk_rows_cases.py), checked on the numpy restatements
alone: the two references agree on every case, every row family reaches the regime it is listed for, the launch geometry (read
from the library's host-only getter) is the intended one.  No test here touches a GPU."""
import functools

import numpy as np
import pytest

from tests import bm25_restatement as br
from tests import topk_rows_cases as tc


@functools.lru_cache(maxsize=None)
def _cases(lib):
    return {c.name: c for c in tc.cases(lib)}


@functools.lru_cache(maxsize=None)
def _matrix(lib, name):
    case = _cases(lib)[name]
    X = tc.matrix(case, tc.split_of(lib, len(case.rows), case.N))
    X.setflags(write=False)
    return X


def _row(lib, name, family, arg=None):
    case = _cases(lib)[name]
    return _matrix(lib, name)[case.rows.index(tc.Row(family, arg))]


def test_the_getter_reports_the_layout_the_restatement_assumes(hip_lib):
    split, shifts = tc.launch_info(hip_lib, 1, 1)
    assert split == 1 and shifts == sorted(shifts, reverse=True) and shifts[-1] == 0 and shifts[2] == 32   # score digits, then id digits
    widths = [a - b for a, b in zip([64] + shifts, shifts)]
    assert sum(widths) == 64 and max(widths) <= 11                                     # 2048 histogram bins hold every digit
    assert tc.rows_per_wg(hip_lib) == 16 * tc.TT and tc.max_split(hip_lib) == 64


def test_both_references_agree_on_every_case(hip_lib):
    """The keys `schedule` selects (no sort) are the keys br.topk returns (a sort): scores as uint32, ids exactly."""
    shifts = tc.shifts_of(hip_lib)
    checked = 0
    for case in _cases(hip_lib).values():
        X = _matrix(hip_lib, case.name)
        for tie in case.tie_orders:
            for r in range(len(case.rows)):
                d, i = br.topk(X[r], max(case.ks), tie)
                for k in case.ks:
                    s = tc.schedule(X[r], k, tie, shifts)
                    order = np.argsort(s.keys)[::-1]
                    bits, ids = tc.split_keys(s.keys[order], tie)
                    assert np.array_equal(bits, d[:k].view(np.uint32)) and np.array_equal(ids, i[:k]), (case.name, r, k, tie)
                    assert (s.passes == "all") == (np.count_nonzero(X[r].view(np.uint32)) <= k)
                    checked += 1
    assert checked > 5000


def test_case_list_covers_the_table(hip_lib):
    cases = _cases(hip_lib)
    W, S = tc.rows_per_wg(hip_lib), tc.max_split(hip_lib)
    sizes = {c.N for c in cases.values()}
    assert sizes >= {1, 2, tc.TT - 1, tc.TT, tc.TT + 1, W, W + 1, 70_001, 50_001, 17_000, (S - 1) * W + 1, 2 ** 21 + 100}
    for c in cases.values():
        assert c.tie_orders == tc.TIE_ORDERS and 1 <= len(c.rows) <= tc.MAX_ROWS and all(1 <= k <= tc.MAX_K for k in c.ks)
        assert c.id_offset == (tc.BIG_OFFSET if c.name == "N70001-mixed" else 0)
        if c.N in (1, 2):
            assert len(c.rows) == 1 and c.ks == (1, 2, 3)
        if c.N in (tc.TT - 1, tc.TT, tc.TT + 1):
            assert len(c.rows) == 3 and c.ks == (1, 300, 2048)
        if c.N in (W, W + 1):
            assert len(c.rows) == 2 and c.ks == (1, 300, 2048)
        if c.N == 70_001 and c.name != "N70001-kpads":
            assert c.ks == (1, 2, 3, 100, 300, 1024, 1025, 2047, 2048)
    mixed = cases["N70001-mixed"]
    assert {r.family for r in mixed.rows} == set(tc.FAMILIES)
    alone = {c.rows[0].family for c in cases.values() if c.N == 70_001 and len(c.rows) == 1}
    assert alone == set(tc.FAMILIES)
    assert (len(cases["N50001-rows700"].rows), cases["N50001-rows700"].ks) == (700, (100,))
    assert (len(cases["N17000-rows2048"].rows), cases["N17000-rows2048"].ks) == (2048, (100,))
    assert (len(cases["cap-first"].rows), cases["cap-first"].ks) == (1, (300,))
    big = cases["N2^21+100"]
    assert [r.family for r in big.rows] == ["all_equal", "chunk_edges"] and big.ks == (1, 300, 2048)
    # every kpad from 2 to 2048 occurs
    assert {tc.kpad_of(k) for c in cases.values() for k in c.ks} == {2 ** e for e in range(1, 12)}
    assert any(tc.kpad_of(k) != k for k in mixed.ks) and {2, 3, 1025, 2047} <= set(mixed.ks)


def test_split_values_are_the_intended_ones(hip_lib):
    W, S = tc.rows_per_wg(hip_lib), tc.max_split(hip_lib)
    cases = _cases(hip_lib)
    split = lambda name: tc.split_of(hip_lib, len(cases[name].rows), cases[name].N)
    assert split(f"N{W}-split") == 1 and split(f"N{W + 1}-split") == 2
    assert split("N70001-mixed") == 5 and split("N70001-distinct") == 5 and -(-70_001 // W) == 5
    assert split("N50001-rows700") == 3 < -(-50_001 // W)           # the row count caps it
    assert split("N17000-rows2048") == 1 < -(-17_000 // W)
    assert split("cap-first") == S == 64 and tc.split_of(hip_lib, 1, (S - 1) * W) == S - 1 == 63
    assert split("N2^21+100") == S < -(-(2 ** 21 + 100) // W)       # MAX_SPLIT caps it
    # two workgroups over W + 1 elements: the second one's chunk is one element short
    (edge,) = tc.boundaries(W + 1, 2)
    assert edge == W // 2 + 1 and W + 1 - edge == edge - 1
    for N in (tc.TT - 1, tc.TT, tc.TT + 1):
        assert split(f"N{N}-stride") == 1


def test_distinct_rows_finish_within_the_score_passes(hip_lib):
    shifts = tc.shifts_of(hip_lib)
    row = _row(hip_lib, "N70001-mixed", "distinct")
    for k in tc.K_SWEEP:
        for tie in tc.TIE_ORDERS:
            assert tc.schedule(row, k, tie, shifts).passes <= 3


def test_all_equal_rows_are_decided_by_the_id_passes(hip_lib):
    shifts = tc.shifts_of(hip_lib)
    P = len(shifts)
    row = _row(hip_lib, "N70001-mixed", "all_equal")
    for k in tc.K_SWEEP:
        for tie in tc.TIE_ORDERS:
            s = tc.schedule(row, k, tie, shifts)
            # ascending ids: the winners are ids 0 ... k - 1, which fill whole buckets of the shift-10 digit when k is a multiple of
            # 1024 -- that pass then ends the selection; descending ids start inside a bucket (70,001 is no multiple of 1024)
            assert s.passes == (P - 1 if tie == "id_asc" and k % 1024 == 0 else P), (k, tie)
            assert [p.nonempty for p in s.per_pass[:3]] == [1, 1, 1]


def test_two_ulp_rows_are_decided_by_the_lowest_score_digit(hip_lib):
    shifts = tc.shifts_of(hip_lib)
    row = _row(hip_lib, "N70001-mixed", "two_ulp", tc.TWO_ULP_UPPER)
    upper = int(np.count_nonzero(row.view(np.uint32) == tc.ONE + 1))
    assert upper == tc.TWO_ULP_UPPER and np.nextafter(np.float32(1), np.float32(2)).view(np.uint32) == tc.ONE + 1
    assert set(np.unique(row.view(np.uint32)).tolist()) == {tc.ONE, tc.ONE + 1}
    below, above = 300, 1024
    assert below in tc.K_SWEEP and above in tc.K_SWEEP and below < upper < above
    for k in (below, above):
        for tie in tc.TIE_ORDERS:
            s = tc.schedule(row, k, tie, shifts)
            assert s.passes == len(shifts), (k, tie)
            assert [p.nonempty for p in s.per_pass[:3]] == [1, 1, 2] and s.per_pass[2].shift == 32
            assert s.per_pass[2].above == (0 if k == below else upper)


def test_shift_21_pass_separates_rows_only_beyond_2_21(hip_lib):
    shifts = tc.shifts_of(hip_lib)
    at = shifts.index(21)
    small = tc.schedule(_row(hip_lib, "N70001-mixed", "all_equal"), 300, "id_desc", shifts)
    assert small.per_pass[at].nonempty == 1
    row = _row(hip_lib, "N2^21+100", "all_equal")
    for tie in tc.TIE_ORDERS:
        for k in tc.K_EDGES:
            assert tc.schedule(row, k, tie, shifts).per_pass[at].nonempty == 2
    s = tc.schedule(row, 300, "id_desc", shifts)
    # the upper bucket (ids 2^21 ... 2^21 + 99) gives 100 rows, the lower one the other 200
    assert (s.per_pass[at].above, s.per_pass[at].want, s.per_pass[at].bucket) == (100, 200, 2 ** 21)
    _, ids = tc.split_keys(s.keys, "id_desc")
    assert sorted(ids.tolist()) == list(range(2 ** 21 - 200, 2 ** 21 + 100))
    edges = tc.schedule(_row(hip_lib, "N2^21+100", "chunk_edges"), 2048, "id_desc", shifts)
    assert edges.passes != "all"


def test_sparse_rows_sit_at_k_minus_1_k_and_k_plus_1(hip_lib):
    shifts = tc.shifts_of(hip_lib)
    case = _cases(hip_lib)["N70001-mixed"]
    X = _matrix(hip_lib, case.name)
    hits = {row.arg: r for r, row in enumerate(case.rows) if row.family == "sparse"}
    assert set(hits) == set(tc.SPARSE_HITS)
    for h, r in hits.items():
        assert np.count_nonzero(X[r].view(np.uint32)) == h
        if h >= 2:
            assert X[r, 0] > 0 and X[r, -1] > 0
    for k in (1, 300, 2048):
        assert k in case.ks
        for h in (k - 1, k, k + 1):
            s = tc.schedule(X[hits[h]], k, "id_asc", shifts)
            assert (s.passes == "all") == (h <= k) and len(s.keys) == min(h, k)
    for name, k in (("N50001-rows700", 100), ("N17000-rows2048", 100)):
        c = _cases(hip_lib)[name]
        counts = np.count_nonzero(_matrix(hip_lib, name).view(np.uint32), axis=1)
        assert counts[:5].tolist() == [0, 1, k - 1, k, k + 1] == [r.arg for r in c.rows[:5]]
        assert counts.max() <= c.N // 10 and (counts > k).sum() > len(c.rows) // 2


def test_extremes_hold_every_listed_pattern(hip_lib):
    row = _row(hip_lib, "N70001-mixed", "extremes")
    assert set(np.unique(row.view(np.uint32)).tolist()) == set(tc.EXTREME_BITS)
    assert np.float32(np.finfo(np.float32).max).view(np.uint32) == 0x7F7FFFFF and np.float32(np.finfo(np.float32).tiny).view(np.uint32) == 0x00800000
    assert np.isfinite(row).all()


def test_chunk_edges_plant_both_sides_of_every_boundary(hip_lib):
    for name in ("N16385-split", "N70001-mixed", "N70001-chunk_edges", "cap-first", "N2^21+100", "N1025-stride"):
        case = _cases(hip_lib)[name]
        split = tc.split_of(hip_lib, len(case.rows), case.N)
        row = _row(hip_lib, name, "chunk_edges")
        edges = tc.boundaries(case.N, split)
        assert len(edges) == split - 1
        per = -(-case.N // split)
        fillers_max = row[np.setdiff1d(np.arange(case.N), [0, case.N - 1] + edges + [e - 1 for e in edges])].max()
        assert row[0] > fillers_max and row[-1] > fillers_max
        for c, e in enumerate(edges, start=1):
            assert e == c * per and row[e - 1] == row[e] > fillers_max               # an equal pair straddles the boundary
        assert len({float(row[e]) for e in edges}) == len(edges)
        assert np.count_nonzero(row) > max(case.ks) or case.N < 2 * tc.MAX_K          # more than k plants where N allows
        # the winners for k = plants at the edges are exactly those
        k = 2 + 2 * len(edges)
        _, ids = br.topk(row, k, "id_asc")
        assert sorted(ids.tolist()) == sorted([0, case.N - 1] + edges + [e - 1 for e in edges])


def test_getter_arguments(hip_lib):
    import ctypes
    out = (ctypes.c_int64 * 8)()
    for rows, N in ((0, 10), (-1, 10), (65536, 10), (1, 0), (1, -5), (1, 2 ** 31)):
        assert hip_lib.mq_topk_rows_launch_info(rows, N, out) == -1, (rows, N)
    assert hip_lib.mq_topk_rows_launch_info(1, 10, None) == -1
    assert hip_lib.mq_topk_rows_launch_info(65535, 2 ** 31 - 1, out) == 0 and out[0] == 1
    with pytest.raises(ValueError):
        tc.launch_info(hip_lib, 0, 10)
