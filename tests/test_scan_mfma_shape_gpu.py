"""GPU: the 256 x 256 tile kernel of the screened search on either matrix instruction (MQ_KNN_OPT_SCAN_MFMA: 0 =
v_mfma_f32_32x32x16_bf16, 1 = v_mfma_f32_16x16x32_bf16; csrc/knn_screen.inc).  The two instances share everything but the K loop
and the accumulator layout the selection epilogue walks, so every case runs under both values and compares scores, ids and tie
order bit for bit with the CPU oracle.  300 queries throughout: two query tiles, which only the tile kernel serves.

What a wrong epilogue would get wrong, case by case:
  * the (accumulator, lane, register) -> KB row and (accumulator, lane) -> query maps: one planted winner per query, every row
    position of a wave's 64 x 64 tile against every query column of it;
  * the 16x16x32 instance's two writer lanes per pool slice (lane, lane ^ 16): runs of consecutive rows that straddle a lane
    pair, inside one group of ballot-gated sites and across two;
  * the ragged last chunk (its own compile-time instance), the winner in the shard's last row;
  * tie-heavy lattice data, where whole pools fill with equal scores;
  * the L2 metric's two extra columns (13 K blocks at d = 768).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ = 300
SHAPES = pytest.mark.parametrize("shape", [0, 1], ids=["mfma32x32x16", "mfma16x16x32"])


def _index(X, metric=0):
    from viquae_amd.index import MI355XFlatIndex
    idx = MI355XFlatIndex(string_factory="Flat", metric_type=metric, screen=True)
    idx.add_vectors(X)
    assert idx.screen
    return idx


def _search(idx, Q, k, shape):
    from viquae_amd import _lib
    assert idx.scan_kind(len(Q), k) == "tile"
    with _lib.knn_option(_lib.KNN_OPT_SCAN_MFMA, shape):
        D, I = idx.search_batch(Q, k)
        stats = idx.screen_stats(len(Q), k)
    return np.asarray(D), np.asarray(I), stats


@pytest.fixture(scope="module")
def sweep_data():
    """512 x 64 Gaussian rows and, per shift t, 300 queries that are scaled copies of chosen rows: query j's unique best row
    (|x|^2 ~ 64 against ~ 26 for the best of the other 511) sits at row position (j + t) % 64 of its wave's tile while the query
    sits at column j % 64 -- over t = 0 .. 63 every (row position, query column) pair, in varying row panels and chunks."""
    from oracle import knn as ok
    rng = np.random.default_rng(64)
    X = rng.standard_normal((512, 64), dtype=np.float32)
    cases = []
    for t in range(64):
        j = np.arange(NQ)
        rows = 64 * ((j // 64 + 3 * t) % 8) + (j + t) % 64
        Q = np.ascontiguousarray(X[rows] * np.float32(1.5))
        D, I = ok.knn(X, Q, 1)
        assert np.array_equal(I[:, 0], rows)  # the plant is the unique winner
        cases.append((Q, D, I))
    return X, cases


@SHAPES
def test_c_layout_sweep(sweep_data, shape):
    X, cases = sweep_data
    idx = _index(X)
    for t, (Q, Do, Io) in enumerate(cases):
        D, I, stats = _search(idx, Q, 1, shape)
        assert np.array_equal(I, Io), (t, np.flatnonzero(I[:, 0] != Io[:, 0])[:8])
        assert np.array_equal(D, Do), t
        assert stats[0] == 0


# rows of one 16-row accumulator block that one query takes, relative to the block's first row:
#   eight      4g .. 4g + 7: registers 0 .. 3 of both lanes of a pair -- two site groups (registers 0 - 2, then 3 ...)
#   one_group  registers 0 - 2 of both lanes: every hit falls into ONE ballot-gated group of sites
#   shifted    4g + 2 .. 4g + 9: a pair's tail plus the first lane of the next pair (another slice)
RUNS = {"eight": (0, 1, 2, 3, 4, 5, 6, 7), "one_group": (0, 1, 2, 4, 5, 6), "shifted": (2, 3, 4, 5, 6, 7, 8, 9)}


@pytest.fixture(scope="module")
def paired_data():
    """2048 x 64 Gaussian rows in which query j < 256 owns the run that starts at row 8 j (8 rows apart: lane pairs (0, 1) and
    (2, 3) of every block, every block and row panel; runs never overlap): the rows of its run are scaled copies of the query, all
    far above the rest.  Queries 256 .. 299 (the second tile) see Gaussian rows only."""
    from oracle import knn as ok
    out = {}
    for name, run in RUNS.items():
        rng = np.random.default_rng(len(name))
        X = rng.standard_normal((2048, 64), dtype=np.float32)
        Q = rng.standard_normal((NQ, 64), dtype=np.float32)
        for j in range(256):
            for e, r in enumerate(run):
                if 8 * j + r < 2048:
                    X[8 * j + r] = Q[j] * np.float32(1.0 + 0.03125 * (e + 1))
        out[name] = (X, Q, {k: ok.knn(X, Q, k) for k in (8, 100)})
    return out


@SHAPES
@pytest.mark.parametrize("k", [8, 100])
@pytest.mark.parametrize("run", list(RUNS))
def test_paired_lane_appends(paired_data, run, k, shape):
    X, Q, oracle = paired_data[run]
    Do, Io = oracle[k]
    D, I, stats = _search(_index(X), Q, k, shape)
    assert np.array_equal(I, Io), np.flatnonzero((I != Io).any(1))[:8]
    assert np.array_equal(D, Do)
    assert stats[0] == 0
    if run == "eight":  # the planted run is the head of its query's list, best (largest factor) first
        assert np.array_equal(I[:256, :8], 8 * np.arange(256)[:, None] + np.arange(7, -1, -1)[None, :])


@SHAPES
@pytest.mark.parametrize("d", [768, 96])
@pytest.mark.parametrize("n", [257, 3 * 256 + 5])
def test_ragged_last_chunk(n, d, shape):
    from oracle import knn as ok
    rng = np.random.default_rng(n + d)
    X = rng.standard_normal((n, d), dtype=np.float32)
    Q = rng.standard_normal((NQ, d), dtype=np.float32)
    X[n - 1] = Q[5] * np.float32(2.0)   # the shard's last row wins query 5 ...
    Q[261] = X[n - 1]                   # ... and a query of the second tile
    Do, Io = ok.knn(X, Q, 10)
    assert Io[5, 0] == n - 1 and Io[261, 0] == n - 1
    D, I, stats = _search(_index(X), Q, 10, shape)
    assert np.array_equal(I, Io) and np.array_equal(D, Do)
    assert stats[0] == 0


RMAX = 1024  # candidate rows per query the re-scoring takes (csrc/knn_screen.inc): more raise the tile's overflow flag


@pytest.fixture(scope="module")
def lattice_data():
    """40 000 rows drawn from 96 distinct integer vectors (entries -3 .. 3, d = 64): every score is an integer shared by ~ 417
    rows, so whatever passes a threshold passes it hundreds of times over and the pool slices take runs of equal keys from both
    writer lanes.  Checked against the oracle before any device work: for every query the rows at or above its 100-th best score
    stay below the candidate bound, so the overflow fallback has no reason to serve the result."""
    from oracle import knn as ok
    rng = np.random.default_rng(2)
    V = rng.integers(-3, 4, (96, 64)).astype(np.float32)
    X = np.ascontiguousarray(V[rng.integers(0, 96, 40000)])
    Q = rng.integers(-3, 4, (NQ, 64)).astype(np.float32)
    D, I = ok.knn(X, Q, 100)
    at_or_above = ((Q @ X.T) >= D[:, 99:100] - 0.5).sum(1)  # integer scores: exact in fp32, and the bf16 margin is far below 1
    assert D[:, 99].min() > -1e30 and at_or_above.max() <= RMAX - 64, at_or_above.max()
    return X, Q, D, I


@SHAPES
def test_tie_lattice_fills_pools_without_fallback(lattice_data, shape, monkeypatch):
    """Equal-score runs through both writer lanes of the slices, bit-exact results, no tile recomputed exactly.  (At this size
    the slabs are one or two chunks long, so no slice reaches the compaction trigger: that is test_compaction_with_two_writers.)"""
    X, Q, Do, Io = lattice_data
    # uncentred copy: integers are exact in bf16, the margin is then the accumulation term alone (~ 0.01 against score steps of 1);
    # rows minus their mean are not, and a margin above 1 would let the next score level -- hundreds of rows -- into every pool
    monkeypatch.setenv("MQ_KNN_CENTER", "0")
    D, I, stats = _search(_index(X), Q, 100, shape)
    assert np.array_equal(I, Io) and np.array_equal(D, Do)
    assert stats[0] == 0                    # query_tiles_recomputed_exactly
    assert stats[1] >= NQ * 100 and stats[2] <= RMAX


RISING_ROWS = 12 * 256  # the tail of the shard whose scores rise with the row id, for every query


def rising_data():
    """Data that drives the pools of the shard's last slab through the compaction trigger several times at 300 queries.

    Two query tiles make a 256-CU device cut the shard into 128 slabs, a slice takes at most 32 keys per chunk and query, and
    the trigger is "more than 64 keys in a slice": a slab needs at least four chunks, so the shard has 128 x 12 chunks =
    393 216 rows, not the ~ 40 000 of smaller cases (whose slabs are one or two chunks long).  Rows: Gaussian (scores ~ N(0, 10^2)
    against the queries below), except the last 12 chunks, which are u (16 + 0.05 i), i = 0 .. 3071, for one unit vector u; the
    queries are Gaussian + 8 u, so every query's score rises strictly with the row id there, from ~ 130 to ~ 1350.  Every row of
    those chunks then beats every threshold its slab has seen: each slice takes 32 keys per chunk from its two writer lanes -- 96
    after the third chunk (flagged), exactly 128 after the fourth, compacted to the ~ 130 best of the pool, then again every third
    chunk.  The final candidates of a query are the rows within the margin of its 100-th best: checked against the oracle to
    stay far below the 1024 the re-scoring takes, so no tile has a reason to fall back."""
    from oracle import knn as ok
    n, d = 128 * 12 * 256, 64
    rng = np.random.default_rng(12)
    X = rng.standard_normal((n, d), dtype=np.float32)
    u = rng.standard_normal(d).astype(np.float32)
    u /= np.linalg.norm(u)
    X[n - RISING_ROWS:] = u[None, :] * (np.float32(16.0) + np.float32(0.05) * np.arange(RISING_ROWS, dtype=np.float32))[:, None]
    Q = rng.standard_normal((NQ, d), dtype=np.float32) + np.float32(8.0) * u[None, :]
    D, I = ok.knn(X, Q, 100)
    tail = Q @ X[n - RISING_ROWS:].T
    assert (np.diff(tail, axis=1) > 0).all() and tail[:, 0].min() > (Q @ X[:n - RISING_ROWS].T).max()  # rising, above every ordinary row
    assert np.array_equal(I[:, 0], np.full(NQ, n - 1))
    # margin = 2 eps, eps <= ||q|| max ||x - bf16(x)|| + ||q - bf16(q)|| max ||x|| + accumulation ~ 2 x 14 x 170 x 2^-9 = 9.3: 40 is generous
    assert ((tail >= D[:, 99:100] - 40.0).sum(1)).max() <= RMAX // 2
    return X, Q, D, I


@pytest.fixture(scope="module")
def rising():
    return rising_data()


@SHAPES
def test_compaction_with_two_writers(rising, shape):
    """Bit-exact results and no tile recomputed exactly while the last slab's pools are compacted again and again (rising_data).
    That the trigger fires is counted in a diagnostic build (tools/scan_compactions.py, figures in profiles/r07_notes.md); here
    the end state shows it: the last slab was handed 12 x 256 keys per query, eight times what a pool holds, and its pools end
    above half full without any overflow."""
    X, Q, Do, Io = rising
    idx = _index(X)
    D, I, stats = _search(idx, Q, 100, shape)
    assert np.array_equal(I, Io) and np.array_equal(D, Do)
    assert stats[0] == 0                    # query_tiles_recomputed_exactly
    slabs = stats[6]
    if (len(X) // 256) // slabs >= 12:      # the rising rows lie in one slab (any device with at most 256 CUs)
        assert 512 < stats[3] <= 1024, stats  # fullest pool of the call: past the trigger (8 x 64), within its 8 x 128 slots


@SHAPES
def test_l2_metric_thirteen_k_blocks(shape):
    """L2 at d = 768: the bf16 copy carries the (h, l) pair of -||x||^2 / 2 in columns 768, 769 -- 832 columns, 13 K blocks (an odd
    count: the two LDS stages swap roles from chunk to chunk) -- on a ragged shape."""
    from oracle import knn as ok
    n = 5 * 256 + 77
    rng = np.random.default_rng(13)
    X = rng.standard_normal((n, 768), dtype=np.float32)
    Q = rng.standard_normal((NQ, 768), dtype=np.float32)
    Q[0] = X[n - 1]  # distance 0 in the last row
    Do, Io = ok.knn(X, Q, 10, metric=1)
    assert Io[0, 0] == n - 1
    D, I, stats = _search(_index(X, metric=1), Q, 10, shape)
    assert np.array_equal(I, Io) and np.array_equal(D, Do)
    assert stats[0] == 0
