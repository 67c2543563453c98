"""CPU suite: the host layer the three flat index classes share (viquae_amd/index.py) -- the whole-panel batching of
``add_vectors`` and the numpy boundary ``search`` / ``search_batch``, the latter off the GPU through a stub whose
``search_device`` answers from the oracle (the branch the gloo tests of ShardedFlatIndex take)."""
import numpy as np
import pytest

RAGGED = (1, 62, 1, 100, 7, 64, 129, 300, 5, 331)  # row counts of the pieces a column arrives in (1000 rows)


def _blocks(d=12):
    rng = np.random.default_rng(0)
    return [rng.integers(-4, 5, (n, d)).astype(np.float32) for n in RAGGED]


def test_whole_panel_blocks_recuts_ragged_blocks_into_multiples_of_64():
    from viquae_amd.index import whole_panel_blocks
    blocks = _blocks()
    out = list(whole_panel_blocks(iter(blocks)))
    assert all(b.shape[0] % 64 == 0 and b.shape[0] for b in out[:-1]) and out[-1].shape[0]
    assert [b.shape[0] for b in out] == [64, 64, 64, 128, 320, 320, 40]  # cut where the pending rows + a block reach a panel
    got, want = np.concatenate(out), np.concatenate(blocks)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()


def test_whole_panel_blocks_passes_whole_blocks_on_uncopied():
    from viquae_amd.index import whole_panel_blocks
    a, b, c = np.zeros((128, 12), np.float32), np.ones((64, 12), np.float32), np.ones((5, 12), np.float32)
    out = list(whole_panel_blocks([a, b, c]))
    assert len(out) == 3 and out[0] is a and out[1] is b and out[2] is c
    assert list(whole_panel_blocks([])) == []
    only = list(whole_panel_blocks([c]))
    assert len(only) == 1 and only[0] is c
    # an empty block between two others neither shows up nor cuts anything
    out = list(whole_panel_blocks([c, np.zeros((0, 12), np.float32), a]))
    assert [x.shape[0] for x in out] == [128, 5] and np.array_equal(np.concatenate(out), np.concatenate([c, a]))


def _oracle_index(X, metric):
    """A HostBoundaryIndex with a "cpu" query device and the oracle behind search_device."""
    import torch
    from oracle import knn as ok
    from viquae_amd.index import HostBoundaryIndex

    class OracleIndex(HostBoundaryIndex):
        def __init__(self):
            super().__init__()
            self.seen = []

        def _query_device(self):
            return "cpu"

        def search_device(self, q, k):
            assert q.dtype == torch.float32 and q.device.type == "cpu"
            self.seen.append(tuple(q.shape))
            D, I = ok.knn(X, q.numpy(), k, metric=metric)
            return torch.from_numpy(D), torch.from_numpy(I)

    return OracleIndex()


@pytest.fixture(scope="module")
def lattice():
    rng = np.random.default_rng(1)
    return rng.integers(-4, 5, (200, 12)).astype(np.float32), rng.integers(-4, 5, (30, 12)).astype(np.float32)


@pytest.mark.parametrize("metric", [0, 1])
def test_search_batch_off_the_gpu_returns_what_search_device_returns(lattice, metric):
    from oracle import knn as ok
    X, Q = lattice
    idx = _oracle_index(X, metric)
    for queries in (Q, Q.astype(np.float64), Q.astype(np.int64), Q[:0]):
        D, I = idx.search_batch(queries, 7)
        Do, Io = ok.knn(X, Q[:len(queries)], 7, metric=metric)
        assert D.dtype == np.float32 and I.dtype == np.dtype(int) and D.shape == I.shape == (len(queries), 7)
        assert np.array_equal(I, Io) and np.array_equal(D, Do)
    assert idx.seen == [(30, 12)] * 3 + [(0, 12)] and idx._io is None  # no pinned staging off the GPU
    with pytest.raises(ValueError, match="Shape of query must be 2D"):
        idx.search_batch(Q[0], 7)


def test_search_takes_one_query_as_a_vector_or_a_one_row_matrix(lattice):
    from oracle import knn as ok
    X, Q = lattice
    idx = _oracle_index(X, 0)
    Do, Io = ok.knn(X, Q[:1], 5, metric=0)
    for query in (Q[0], Q[:1]):
        scores, indices = idx.search(query, 5)
        assert scores.shape == indices.shape == (5,) and indices.dtype == np.dtype(int)
        assert np.array_equal(indices, Io[0]) and np.array_equal(scores, Do[0])
    with pytest.raises(ValueError, match=r"Shape of query is incorrect, it has to be either a 1D array or 2D \(1, N\)"):
        idx.search(Q[:2], 5)
