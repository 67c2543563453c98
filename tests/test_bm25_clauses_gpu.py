"""GPU tests of the clause batches of the two BM25 scoring kernels (csrc/bm25.hip: bm25_score_kernel, bm25_score_grid_kernel): RAW
clause arrays through MI355XBM25Index.search_device / search_grid_device -- not through clauses(), which de-duplicates terms and
drops ids outside the vocabulary -- against the raw restatement (tests/bm25_restatement.py: scores_raw), BIT FOR BIT.  The kernels
search the posting ranges of CB = mq_bm25_clause_batch() clauses at once; the batch of bm25_restatement.clause_queries holds
queries of 0, 1, CB - 1, CB, CB + 1, 2 CB, 2 CB + 1 and 3 CB + 5 clauses in ONE launch, none of the longer ones starting at a
multiple of CB in cterm, with a planted term at clause CB - 1 (the last of a batch), CB (the first of the next) and the last
clause: a term in every block, a term without postings, and ids outside [0, n_terms), which the kernels turn into an empty range
before anything is read through them.  tests/test_bm25_cpu.py checks what this file takes for granted.  k = 2048, id_asc."""
import copy
import functools

import numpy as np
import pytest

from tests import bm25_restatement as br

pytestmark = pytest.mark.gpu

K = 2048
PLANTS = tuple(br.CLAUSE_PLANTS)
GRID_LENGTHS = ("1", "GT", "GT+1")


def _lib():
    from viquae_amd import _lib
    return _lib.load()


def _CB():
    return int(_lib().mq_bm25_clause_batch())


def _plain(size):
    """(index, restatement) of the plain kernel's corpus of that size, both shared with tests/test_bm25_gpu.py."""
    from tests import test_bm25_gpu as plain
    N = plain._size(size)
    index = plain._index(N)
    index.tie_order = "id_asc"
    return index, br.restated(N, plain._R())


def _grid(size):
    from tests import test_bm25_grid_gpu as grid
    N = grid._size(size)
    index = grid._index(N)
    index.tie_order = "id_asc"
    return index, N, grid._Rg()


@functools.lru_cache(maxsize=None)
def _rest_under(N, R, setting):
    """A copy of the shared restatement under another (k1, b); the shared one stays as it is."""
    rest = copy.copy(br.restated(N, R))
    rest.set_bm25(*setting)
    return rest


def _upload(index, queries):
    import torch
    return tuple(torch.from_numpy(a).to(index._torch_device) for a in br.pack_raw(queries))


def _download(D, I):
    import torch
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


def _same(got, want, what):
    D, I = got
    assert D.dtype == np.float32 and D.shape == want[0].shape and I.shape == want[1].shape, what
    assert np.array_equal(np.asarray(I, dtype=np.int64), want[1]), what
    assert np.array_equal(np.ascontiguousarray(D).view(np.uint32), np.ascontiguousarray(want[0]).view(np.uint32)), what


def _no_hits(got, row):
    return bool((got[1][row] == -1).all()) and bool(np.isneginf(got[0][row]).all())


@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("size", ["R+37", "3R+1"])
def test_plain_kernel_equals_the_raw_restatement(size, plant):
    index, rest = _plain(size)
    queries = br.clause_queries(_CB(), br.CLAUSE_PLANTS[plant])
    got = _download(*index.search_device(*_upload(index, queries), K))
    _same(got, br.search_raw(rest, queries, K), (size, plant))
    assert _no_hits(got, br.ZERO_WEIGHT_QUERY) and _no_hits(got, 2)          # weight 0: every product is +0; no clause at all
    assert _no_hits(got, 1) == (plant != "every")                            # the one-clause query IS the planted term
    assert got[1][br.LONG_QUERY, K - 1] >= 0                                 # the long queries fill all k slots


@pytest.mark.parametrize("size", ["R+37", "3R+1"])
def test_plain_kernel_one_query_of_a_batch_and_one_clause(size):
    """The CB + 1 query alone: its clauses start at cterm[0], the second batch is a single clause."""
    index, rest = _plain(size)
    CB = _CB()
    for plant in ("every", "unused", "int32_min"):
        query = br.clause_queries(CB, br.CLAUSE_PLANTS[plant])[br.clause_counts(CB).index(CB + 1)]
        assert len(query[0]) == CB + 1
        got = _download(*index.search_device(*_upload(index, [query]), K))
        _same(got, br.search_raw(rest, [query], K), (size, plant))


@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("length", GRID_LENGTHS)
@pytest.mark.parametrize("size", ["Rg+37", "3Rg+1"])
def test_grid_kernel_equals_the_raw_restatement_and_the_loop(size, length, plant):
    import torch
    from tests import test_bm25_grid_gpu as grid
    from viquae_amd.ir.bm25 import norm_cache
    index, N, Rg = _grid(size)
    params = grid._settings(grid._length(length))
    queries = br.clause_queries(_CB(), br.CLAUSE_PLANTS[plant])
    arrays = _upload(index, queries)
    caches = torch.from_numpy(np.stack([norm_cache(k1, b, index.avgdl) for k1, b in params])).to(index._torch_device)
    D, I = _download(*index.search_grid_device(*arrays, caches, K))
    assert D.shape == (len(params), len(queries), K) and I.shape == D.shape
    own = (index.k1, index.b)
    try:
        for g, setting in enumerate(params):
            _same((D[g], I[g]), br.search_raw(_rest_under(N, Rg, setting), queries, K), (size, length, plant, g, "restatement"))
            index.set_bm25(*setting)
            _same((D[g], I[g]), _download(*index.search_device(*arrays, K)), (size, length, plant, g, "loop"))
            assert _no_hits((D[g], I[g]), br.ZERO_WEIGHT_QUERY)
    finally:
        index.set_bm25(*own)


@pytest.mark.parametrize("size", ["Rg+37", "3Rg+1"])
def test_grid_kernel_one_query_of_a_batch_and_one_clause(size):
    import torch
    from tests import test_bm25_grid_gpu as grid
    from viquae_amd.ir.bm25 import norm_cache
    index, N, Rg = _grid(size)
    CB = _CB()
    params = grid._settings(grid._GT() + 1, start=3)
    caches = torch.from_numpy(np.stack([norm_cache(k1, b, index.avgdl) for k1, b in params])).to(index._torch_device)
    query = br.clause_queries(CB, br.T_EVERY)[br.clause_counts(CB).index(CB + 1)]
    D, I = _download(*index.search_grid_device(*_upload(index, [query]), caches, K))
    for g, setting in enumerate(params):
        _same((D[g], I[g]), br.search_raw(_rest_under(N, Rg, setting), [query], K), (size, g))
