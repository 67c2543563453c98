"""CPU suite of the BM25 parameter grid (csrc/bm25.hip: mq_bm25_search_grid_f32; viquae_amd/ir/hp.py): the conditions under which
the GPU cases (tests/test_bm25_grid_gpu.py, tests/test_bm25_hp_gpu.py) mean something, checked on the numpy restatement alone; the
host-only entries of the C ABI; the job's search space and its first-maximum rule.  No GPU: the library loads without one."""
import copy

import numpy as np
import pytest

from tests import bm25_hp_world as world
from tests import bm25_restatement as br

SETTINGS = [(1.2, 0.75), (0.0, 0.3), (0.5, 0.0), (0.5, 0.3), (3.0, 1.0), (0.1, 0.1), (2.9, 0.9), (1.2, 0.0), (0.0, 0.0), (0.7, 0.5),
            (0.5, 0.30000000000000004)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(x, y):
    return np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1])


def test_conditions_of_the_gpu_cases_hold_on_the_restatement(hip_lib):
    """At the grid kernel's own block size: every setting changes the returned ids against (1.2, 0.75) at the three larger corpora
    and -- (1.2, 0.0) at N = 1 excepted, where the single document's length is avgdl -- the scores at every size; k1 = 0 leaves a
    handful of distinct scores over ~2000 hits (ties decide the selection); (0, 0.3) and (0, 0) agree; 0.30000000000000004 is
    0.3 in fp32.  A grid search that ignored its settings could therefore not pass."""
    Rg = hip_lib.mq_bm25_grid_block_rows(hip_lib.mq_bm25_grid_tile())
    assert Rg >= 64 and Rg & (Rg - 1) == 0
    qs = br.queries()
    for N in br.corpus_sizes(Rg):
        base = br.restated(N, Rg)
        D0, I0 = base.search(qs, 100)
        rest = copy.copy(base)           # set_bm25 rebinds the cache and the impacts: the shared restatement stays as it is
        got = {}
        for k1, b in SETTINGS[1:]:
            rest.set_bm25(k1, b)
            D, I = got[(k1, b)] = rest.search(qs, 100)
            if N > 1:
                assert not np.array_equal(I, I0), (N, k1, b)
            same_scores = np.array_equal(_bits(D), _bits(D0))
            assert same_scores == (N == 1 and (k1, b) == (1.2, 0.0)), (N, k1, b)
        assert _same(got[(0.0, 0.3)], got[(0.0, 0.0)]) and _same(got[(0.5, 0.3)], got[(0.5, 0.30000000000000004)])
    assert np.float32(0.30000000000000004) == np.float32(0.3) and 0.30000000000000004 != 0.3
    rest = copy.copy(br.restated(Rg - 1, Rg))
    rest.set_bm25(0.0, 0.3)
    scores = rest.scores(qs[0])
    hits = scores[scores > 0]
    assert hits.size > 0.9 * (Rg - 1) and np.unique(hits).size == 7


def test_conditions_of_the_job_test_hold_on_the_restatement():
    """A guard, on the restatement alone, against the job test passing vacuously; the grid it restates is the job's own."""
    from viquae_amd.ir import hp
    assert [(p["b"], p["k1"]) for p in hp.grid_points(hp.search_space(world.HYP_HYP))] == world.GRID
    values = world.restated_mrr()
    assert len(values) == 12 and len(set(values)) == 7
    assert values[0] == 0.5 and max(values) == 1.0
    assert [g for g, v in enumerate(values) if v == 1.0] == [5, 9]
    assert world.GRID[5] == (0.5, 0.4) and world.GRID[9] == (1.0, 0.4)


def test_grid_entries_validate_before_any_hip_call(hip_lib):
    lib = hip_lib
    GT = lib.mq_bm25_grid_tile()
    assert GT >= 1
    assert lib.mq_bm25_grid_block_rows(1) == lib.mq_bm25_block_rows()
    rows = [lib.mq_bm25_grid_block_rows(g) for g in range(1, GT + 1)]
    assert all(r > 0 and r & (r - 1) == 0 for r in rows) and rows == sorted(rows, reverse=True)
    assert lib.mq_bm25_grid_block_rows(0) == 0 and lib.mq_bm25_grid_block_rows(GT + 1) == 0
    assert lib.mq_bm25_grid_chunk_queries(1000, 37, 4, 1000 * 4 * 4 * 5) == 5
    assert lib.mq_bm25_grid_chunk_queries(1000, 37, 4, 0) == 1
    assert lib.mq_bm25_grid_chunk_queries(1000, 37, 1, 1 << 40) == 37
    assert lib.mq_bm25_grid_chunk_queries(1000, 100000, GT, 1 << 50) == 65535 // GT      # the rows of one selection launch
    assert lib.mq_bm25_grid_workspace_bytes(1000, 37, 4, 5000, 1 << 30) == 0             # k above MQ_KNN_MAX_K
    assert lib.mq_bm25_grid_workspace_bytes(1000, 37, 4, 10, 1 << 30) > 4 * 37 * 1000 * 4
    null = lambda G, k, ws_bytes: lib.mq_bm25_search_grid_f32(None, None, None, None, None, G, 1000, 50, None, None, None, 37, k, 0, 0,
                                                              None, None, None, ws_bytes, 1 << 30, None)
    assert null(4, 10, 1 << 30) == -1                                                     # MQ_EINVAL: NULL pointers
    # the remaining codes need non-NULL pointers; nothing is dereferenced before the checks
    import ctypes
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    call = lambda G, k, ws_bytes, flags=0: lib.mq_bm25_search_grid_f32(p, p, p, p, p, G, 1000, 50, p, p, p, 37, k, flags, 0, p, p, p, ws_bytes,
                                                                       1 << 30, None)
    assert call(0, 10, 1 << 30) == -1                                                     # G < 1
    assert call(4, 10, 1 << 30, flags=1) == -1                                            # an unknown flag
    assert call(4, 5000, 1 << 30) == -4                                                   # MQ_EUNSUPPORTED: k > MQ_KNN_MAX_K
    assert call(4, 10, 16) == -2                                                          # MQ_EWORKSPACE
    assert lib.mq_strerror(-4) and lib.mq_strerror(-2) == b"workspace too small"


def test_default_search_space_is_the_references_grid():
    """What get_objective hands the sampler for the default hyp_hyp: 10 values of b x 30 of k1, b-major."""
    from viquae_amd.ir import hp
    space = hp.search_space(None)
    assert space == dict(b=np.arange(0, 1, 0.1).tolist(), k1=np.arange(0, 3, 0.1).tolist())
    points = hp.grid_points(hp.GridSampler(space).search_space)
    assert len(points) == 300 and len(space["b"]) == 10 and len(space["k1"]) == 30
    assert points[0] == {"b": 0.0, "k1": 0.0} and points[1] == {"b": 0.0, "k1": 0.1} and points[30] == {"b": 0.1, "k1": 0.0}
    assert points[-1] == {"b": space["b"][-1], "k1": space["k1"][-1]} and points[-1]["b"] < 1 and points[-1]["k1"] < 3
    assert [p["b"] for p in points] == sorted(p["b"] for p in points)
    assert hp.search_space(world.HYP_HYP) == dict(b=[0.0, 0.5, 1.0], k1=[0.0, 0.4, 1.2, 2.9])
    assert [(p["b"], p["k1"]) for p in hp.grid_points(hp.search_space(world.HYP_HYP))] == world.GRID


def test_best_params_is_the_first_maximum_in_grid_order():
    from viquae_amd.ir import hp
    study = hp.Study()
    study.trials = [{"b": 0.0, "k1": 0.0, "value": 0.5}, {"b": 0.0, "k1": 0.4, "value": 0.75}, {"b": 0.5, "k1": 0.0, "value": 0.25},
                    {"b": 0.5, "k1": 0.4, "value": 0.75}, {"b": 1.0, "k1": 0.0, "value": 0.75}]
    assert study.best_params == {"b": 0.0, "k1": 0.4} and study.best_value == 0.75
    assert hp.first_maximum([0.1, 0.1, 0.1]) == 0 and hp.first_maximum([0.3, 0.1, 0.3], "minimize") == 1
    with pytest.raises(ValueError):
        hp.first_maximum([])
