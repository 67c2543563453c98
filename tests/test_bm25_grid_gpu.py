"""GPU suite of the BM25 parameter grid (MI355XBM25Index.search_grid, csrc/bm25.hip: bm25_score_grid_kernel): for every setting g,
slice g of the result equals BIT FOR BIT -- scores as uint32, ids exactly -- what the numpy restatement (tests/bm25_restatement.py)
returns after ``set_bm25(*params[g])`` and what ``set_bm25(*params[g])`` + ``search_batch`` return on the same index.  Corpus sizes
follow the grid kernel's document block Rg = mq_bm25_grid_block_rows(mq_bm25_grid_tile()): 1, Rg - 1, Rg + 37, 3 Rg + 1, so the
planted block-boundary terms sit at ITS block edges.  tests/test_bm25_grid_cpu.py checks that the settings change the results.
Indexes, restated scores and the loop's results are computed once each and shared."""
import copy
import functools

import numpy as np
import pytest

from tests import bm25_restatement as br

pytestmark = pytest.mark.gpu

SETTINGS = [(1.2, 0.75), (0.0, 0.3), (0.5, 0.0), (0.5, 0.3), (3.0, 1.0), (0.1, 0.1), (2.9, 0.9), (1.2, 0.0), (0.0, 0.0), (0.7, 0.5),
            (0.5, 0.30000000000000004)]
SIZES = ("1", "Rg-1", "Rg+37", "3Rg+1")
LENGTHS = ("1", "GT", "GT+1", "2GT+3")


def _lib():
    from viquae_amd import _lib
    return _lib.load()


def _GT():
    return int(_lib().mq_bm25_grid_tile())


def _Rg():
    return int(_lib().mq_bm25_grid_block_rows(_GT()))


def _size(name):
    return dict(zip(SIZES, br.corpus_sizes(_Rg())))[name]


def _settings(n, start=0):
    """n settings, the list above repeated as needed (beyond 11 a setting comes twice)."""
    return [SETTINGS[(start + i) % len(SETTINGS)] for i in range(n)]


def _length(name):
    GT = _GT()
    return {"1": 1, "GT": GT, "GT+1": GT + 1, "2GT+3": 2 * GT + 3}[name]


def _queries(nq):
    qs = br.queries()
    return qs if nq > 1 else [qs[4]]  # the single query: the 40-term one


@functools.lru_cache(maxsize=None)
def _index(N):
    from viquae_amd.ir.bm25 import MI355XBM25Index
    index = MI355XBM25Index()
    index.add_token_ids(br.corpus(N, _Rg()), br.VOCABULARY_SIZE)
    return index


@functools.lru_cache(maxsize=None)
def _restated_scores(N, setting):
    """The 37 queries' dense scores under ``setting``, from a copy of the shared restatement (which stays as it is)."""
    rest = copy.copy(br.restated(N, _Rg()))
    rest.set_bm25(*setting)
    return [rest.scores(q) for q in br.queries()]


@functools.lru_cache(maxsize=None)
def _restated(N, setting, nq, k, tie_order):
    scores = _restated_scores(N, setting)
    scores = scores if nq > 1 else [scores[4]]
    D = np.full((len(scores), k), -np.inf, dtype=np.float32)
    I = np.full((len(scores), k), -1, dtype=np.int64)
    for row, s in enumerate(scores):
        d, i = br.topk(s, k, tie_order)
        D[row, :len(d)], I[row, :len(i)] = d, i
    return D, I


@functools.lru_cache(maxsize=None)
def _looped(N, setting, nq, k, tie_order):
    """set_bm25 + search_batch on the shared index, its own parameters restored."""
    index = _index(N)
    index.tie_order = tie_order
    own = (index.k1, index.b)
    index.set_bm25(*setting)
    try:
        got = index.search_batch(_queries(nq), k)
    finally:
        index.set_bm25(*own)
    return got.total_scores, np.asarray(got.total_indices, dtype=np.int64)


def _same(got, want, what=None):
    D, I = got
    assert D.dtype == np.float32 and D.shape == want[0].shape and I.shape == want[1].shape, what
    assert np.array_equal(np.asarray(I, dtype=np.int64), want[1]), what
    assert np.array_equal(np.ascontiguousarray(D).view(np.uint32), np.ascontiguousarray(want[0]).view(np.uint32)), what


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("tie_order", ["id_asc", "id_desc"])
@pytest.mark.parametrize("k", br.K_VALUES)
@pytest.mark.parametrize("nq", [1, 37])
@pytest.mark.parametrize("size", SIZES)
def test_every_slice_equals_the_restatement_and_the_loop(size, nq, k, tie_order, length):
    N = _size(size)
    index = _index(N)
    index.tie_order = tie_order
    params = _settings(_length(length))
    D, I = index.search_grid(_queries(nq), params, k, method="grid")
    assert D.shape == (len(params), nq, k) and D.dtype == np.float32 and I.shape == D.shape and I.dtype == np.int64
    for g, setting in enumerate(params):
        _same((D[g], I[g]), _restated(N, setting, nq, k, tie_order), (g, setting, "restatement"))
        _same((D[g], I[g]), _looped(N, setting, nq, k, tie_order), (g, setting, "loop"))
    first = {}
    for g, setting in enumerate(params):  # the same setting twice: two identical slices
        if setting in first:
            _same((D[g], I[g]), (D[first[setting]], I[first[setting]]), (g, setting, "repeat"))
        first.setdefault(setting, g)
    if len(params) > len(SETTINGS):
        assert len(first) < len(params)


def test_search_grid_leaves_the_index_as_it_was():
    N = _size("Rg+37")
    index = _index(N)
    index.tie_order = "id_asc"
    before = (index.k1, index.b, index.impacts().copy())
    for method in ("grid", "loop"):
        index.search_grid(br.queries(), _settings(_GT() + 1, start=1), 100, method=method)
        assert (index.k1, index.b) == before[:2] == (1.2, 0.75)
        assert np.array_equal(index.impacts().view(np.uint32), before[2].view(np.uint32))
    _same(index.search_batch(br.queries(), 100), _restated(N, (1.2, 0.75), 37, 100, "id_asc"))


@pytest.mark.parametrize("tie_order", ["id_asc", "id_desc"])
def test_loop_method_gives_the_same_arrays(tie_order):
    N = _size("Rg+37")
    index = _index(N)
    index.tie_order = tie_order
    params = _settings(_GT() + 1)
    D, I = index.search_grid(br.queries(), params, 100, method="loop")
    for g, setting in enumerate(params):
        _same((D[g], I[g]), _restated(N, setting, 37, 100, tie_order), (g, setting))
    _same(index.search_grid(br.queries(), params, 100), (D, I))  # the default method, whichever it is


@pytest.mark.parametrize("tie_order", ["id_asc", "id_desc"])
def test_identical_documents_tie_under_every_setting(tie_order):
    """2 Rg identical documents: every score ties under every setting, the k-th place lies in a tied run across the block boundary."""
    from viquae_amd.ir.bm25 import MI355XBM25Index
    Rg = _Rg()
    index = MI355XBM25Index(tie_order=tie_order)
    index.add_token_ids(br.tie_corpus(Rg), 16)
    qs, params = [[4, 3], [9, 9]], _settings(2 * _GT() + 3)
    D, I = index.search_grid(qs, params, 100, method="grid")
    rest = br.Restatement(br.tie_corpus(Rg), 16)
    first = list(range(100)) if tie_order == "id_asc" else list(range(2 * Rg - 1, 2 * Rg - 101, -1))
    for g, setting in enumerate(params):
        rest.set_bm25(*setting)
        _same((D[g], I[g]), rest.search(qs, 100, tie_order), (g, setting))
        assert I[g, 0].tolist() == first and np.unique(D[g, 0]).size == 1


def test_query_chunk_boundaries_change_nothing():
    """A workspace budget of 5 GT score rows: a full tile takes the 37 queries five at a time; the results are those of one launch."""
    GT, N = _GT(), _size("Rg+37")
    index, qs = _index(N), br.queries()
    index.tie_order = "id_asc"
    params = _settings(GT + 1, start=2)
    whole = index.search_grid(qs, params, 100, method="grid")
    budget = index.workspace_bytes
    try:
        index.workspace_bytes = N * 4 * 5 * GT
        assert index.grid_query_chunk(len(qs), GT) == 5
        pieces = index.search_grid(qs, params, 100, method="grid")
    finally:
        index.workspace_bytes = budget
    assert index.grid_query_chunk(len(qs), GT) == 37
    _same(pieces, whole)
    for g, setting in enumerate(params):
        _same((whole[0][g], whole[1][g]), _restated(N, setting, 37, 100, "id_asc"), (g, setting))


def test_every_instantiated_tile_width():
    """Lists of 1 ... GT settings: each goes through the kernel instance of its width (and, between powers of two, a partial tile)."""
    GT, N = _GT(), _size("3Rg+1")
    index = _index(N)
    index.tie_order = "id_asc"
    widths = set()
    for n in range(1, GT + 1):
        widths.add(int(_lib().mq_bm25_grid_block_rows(n)))
        params = _settings(n, start=n)
        D, I = index.search_grid(br.queries(), params, 100, method="grid")
        for g, setting in enumerate(params):
            _same((D[g], I[g]), _looped(N, setting, 37, 100, "id_asc"), (n, g, setting))
            _same((D[g], I[g]), _restated(N, setting, 37, 100, "id_asc"), (n, g, setting))
    R = int(_lib().mq_bm25_block_rows())
    assert widths == {R >> s for s in range(GT.bit_length())} and min(widths) == _Rg()


def test_arguments():
    index = _index(_size("Rg-1"))
    qs = br.queries()
    for bad in ([], [(-0.1, 0.5)], [(float("inf"), 0.5)], [(float("nan"), 0.5)], [(1.2, -0.01)], [(1.2, 1.01)], [(1.2, float("nan"))]):
        with pytest.raises(ValueError):
            index.search_grid(qs, bad, 10)
    with pytest.raises(ValueError):
        index.search_grid(qs, SETTINGS[:2], 0)
    with pytest.raises(ValueError):
        index.search_grid(qs, SETTINGS[:2], 10, method="optuna")
    with pytest.raises(NotImplementedError):
        index.search_grid(qs, SETTINGS[:2], 2049)
    D, I = index.search_grid([], SETTINGS[:3], 7)
    assert D.shape == (3, 0, 7) and D.dtype == np.float32 and I.shape == (3, 0, 7) and I.dtype == np.int64
