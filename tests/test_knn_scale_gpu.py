"""GPU: the screened kNN search stays exact over the whole range of finite fp32 inputs, not just its middle.

The screen's margin is computed in fp32 from squared norms (csrc/knn_screen.inc: row_err_stats_kernel, screen_margin_kernel),
and those squares overflow or underflow long before the scores they bound do.  Scaling by a power of two commutes with every
fp32 and bf16 rounding (tests/knn_scale_data.py), so each route below must give, for every scale of the sweep:
  inner product  (X 2^s, Q 2^-s) and (X 2^-s, Q 2^s): D and I bit-identical to the unscaled search;
  L2             (X 2^s, Q 2^s):                      D = 4^s D0, I = I0;
  "L2norm,"                                           D and I bit-identical to the unscaled search;
and the unscaled search equals the CPU oracle without any tile falling back to the exact scan (tests/test_oracle_cpu.py checks
the same invariances on the oracle itself).  Outside those ranges the oracle decides.  At the extreme scales the margin may be
infinite -- the tiles then go to the exact scan -- but never too small, and never NaN."""
import numpy as np
import pytest
import torch

from tests.knn_scale_data import IP_SWEEP, L2_SWEEP, L2NORM_SWEEP, planted, scaled

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_switches():
    from viquae_amd import _lib
    lib = _lib.load()
    yield
    lib.mq_knn_set_option(_lib.KNN_OPT_SMALL_SCAN, 1)
    lib.mq_knn_set_option(_lib.KNN_OPT_SMALL_MIN_TILES, 0)


def _index(X, metric, screen=True, factory="Flat", tie_order=None, l2norm_form=None, shards=0):
    if shards:
        from viquae_amd.sharded import LocalShardsFlatIndex
        idx = LocalShardsFlatIndex([0] * shards, string_factory=factory, metric_type=metric, screen=screen,
                                   allow_repeated_devices=True, tie_order=tie_order, l2norm_form=l2norm_form)
    else:
        from viquae_amd.index import MI355XFlatIndex
        idx = MI355XFlatIndex(string_factory=factory, metric_type=metric, screen=screen, tie_order=tie_order,
                              l2norm_form=l2norm_form)
    idx.add_vectors(X)
    return idx


def _search(X, Q, k, metric, **kw):
    idx = _index(X, metric, **kw)
    D, I = idx.search_batch(Q, k)
    return np.asarray(D), np.asarray(I), idx


def _zero_margin_would_lose(X, Q, k, metric):
    """Share of the queries whose exact top-k holds a row with a bf16 score strictly below the k-th best bf16 score: what a
    screen without a margin would get wrong.  float64 from bf16(q) . bf16(x) (L2: the screen's q.x - ||x||^2 / 2)."""
    x, q = torch.from_numpy(X).cuda(), torch.from_numpy(Q).cuda()
    sb = q.bfloat16().double() @ x.bfloat16().double().T
    se = q.double() @ x.double().T
    if metric == 1:
        h = 0.5 * x.double().pow(2).sum(1)
        sb, se = sb - h, se - h
    kth = sb.topk(k, dim=1).values[:, -1:]
    lost = (sb.gather(1, se.topk(k, dim=1).indices) < kth).any(1)
    return float(lost.double().mean())


def _check_anchor(X, Q, k, metric, D, I, idx, screened, tie_order="id_asc", **okw):
    from oracle import knn as ok
    Do, Io = ok.knn(X, Q, k, metric=metric, tie_order=tie_order, **okw)
    assert np.array_equal(I, Io) and np.array_equal(D, Do), "the unscaled search differs from the oracle"
    if screened:
        assert idx.screen_stats(len(Q), k)[0] == 0, "the unscaled search fell back to the exact scan: the screen went untested"


# name: (n, d, nq, k, clones per base, bases, index options, environment, option switches, expected scan kind, screened)
_IP_ROUTES = {
    "tile": (30000, 128, 300, 50, 80, 8, {}, {}, {}, "tile", True),
    "tile_id_desc": (30000, 128, 300, 50, 80, 8, {"tie_order": "id_desc"}, {}, {}, "tile", True),
    "tile_centred": (30000, 128, 300, 50, 80, 8, {}, {"MQ_KNN_CENTER_QUERIES": "1"}, {}, "tile", True),
    "tile_uncentred": (30000, 128, 300, 50, 80, 8, {}, {"MQ_KNN_CENTER": "0"}, {}, "tile", True),
    "stream": (66000, 768, 40, 100, 150, 4, {}, {}, {}, "stream", True),
    "stream_centred_d768": (66000, 768, 40, 100, 150, 4, {}, {"MQ_KNN_CENTER_QUERIES": "1"}, {}, "stream", True),
    "stream_d256_k64": (66000, 256, 40, 64, 100, 4, {}, {}, {}, "stream", True),
    "exact": (20000, 64, 300, 50, 80, 8, {"screen": False}, {}, {}, "none", False),
    "wide_d1024": (8000, 1024, 280, 20, 40, 8, {}, {}, {}, "tile", True),
    "wide_d2048": (5000, 2048, 270, 20, 40, 8, {}, {}, {}, "tile", True),
    "big_k_partitioned": (170000, 32, 30, 1024, 1500, 3, {}, {}, {}, "tile", False),
    "k2048_exact_rounds": (20000, 32, 30, 2048, 2500, 3, {}, {}, {}, "none", False),
    "sharded": (30000, 64, 300, 50, 80, 8, {"shards": 4}, {}, {}, "tile", False),
}


def _route(name, monkeypatch):
    from viquae_amd import _lib
    n, d, nq, k, clones, bases, kw, env, opts, kind, screened = _IP_ROUTES[name]
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    for key, v in opts.items():
        _lib.load().mq_knn_set_option(getattr(_lib, "KNN_OPT_" + key), v)
    return n, d, nq, k, clones, bases, kw, kind, screened


def _assert_kind(idx, nq, k, kind, name):
    one = idx.shards[0] if hasattr(idx, "shards") else idx
    assert one.scan_kind(nq, k) == kind, (name, one.scan_kind(nq, k))
    if "_centred" in name:
        assert one._screen_metric == 2, one._screen_metric  # MQ_METRIC_IP_CENTRED
    if "uncentred" in name:
        assert one._center is None and one._screen_metric in (0, 1), one._screen_metric


@pytest.mark.parametrize("name", list(_IP_ROUTES))
def test_inner_product_is_bit_identical_under_opposite_power_of_two_scales(name, monkeypatch):
    n, d, nq, k, clones, bases, kw, kind, screened = _route(name, monkeypatch)
    X, Q = planted(1000 + d + k, n, d, nq, clones, bases)
    assert _zero_margin_would_lose(X, Q, k, 0) >= 0.3  # the near-ties decide the k-th place: a margin too small shows
    D0, I0, idx = _search(X, Q, k, 0, **kw)
    _assert_kind(idx, nq, k, kind, name)
    _check_anchor(X, Q, k, 0, D0, I0, idx, screened, tie_order=kw.get("tie_order", "id_asc"))
    del idx
    for s in IP_SWEEP:
        if s == 0:
            continue
        for a, b in ((s, -s), (-s, s)):
            D, I, idx = _search(scaled(X, a), scaled(Q, b), k, 0, **kw)
            _assert_kind(idx, nq, k, kind, name)
            assert np.array_equal(I, I0), f"{name}: ids differ at X 2^{a}, Q 2^{b}"
            assert np.array_equal(D, D0), f"{name}: scores differ at X 2^{a}, Q 2^{b}"
            del idx


def _mixed(seed, n, d, nq, clones, bases):
    """About 1 row in 50 scaled by 2^60 ... 2^66 -- among them every near-copy of the base rows, all by 2^66 so that they stay
    near-ties and fill the top-k --, queries by 2^-62: ||x||^2 of those rows overflows, their scores stay ordinary numbers."""
    rng = np.random.default_rng(seed)
    X, Q, rows = planted(seed, n, d, nq, clones, bases, return_rows=True)
    X[rows.ravel()] = scaled(X[rows.ravel()], 66)
    rest = np.setdiff1d(np.arange(n), rows.ravel())
    for r in rng.choice(rest, n // 50 - rows.size, replace=False):
        X[r] = scaled(X[r], int(rng.integers(60, 67)))
    return X, scaled(Q, -62)


@pytest.mark.parametrize("name", ["tile", "tile_centred", "stream", "sharded"])
def test_inner_product_with_rows_whose_squared_norm_overflows(name, monkeypatch):
    """Only SOME rows overflow: their rounding error (~2^-9 ||q|| ||x||) must be in the margin -- or the margin infinite."""
    from oracle import knn as ok
    n, d, nq, k, clones, bases, kw, kind, _ = _route(name, monkeypatch)
    clones = min(clones, n // 50 // bases)
    X, Q = _mixed(77 + d, n, d, nq, clones, bases)
    assert not np.isfinite(ok.sqnorm_rows(X)).all() and np.isfinite(X).all()
    D, I, idx = _search(X, Q, k, 0, **kw)
    _assert_kind(idx, nq, k, kind, name)
    Do, Io = ok.knn(X, Q, k, metric=0)
    assert np.isfinite(Do).all()
    assert np.array_equal(I, Io), f"{name}: ids differ from the oracle"
    assert np.array_equal(D, Do), f"{name}: scores differ from the oracle"


_L2_ROUTES = {
    "tile": (30000, 128, 300, 50, 80, 8, {}, {}, {}, "tile", True),
    "tile_uncentred": (30000, 128, 300, 50, 80, 8, {}, {"MQ_KNN_CENTER": "0"}, {}, "tile", True),
    "direct": (20000, 128, 7, 50, 80, 7, {}, {}, {}, "none", False),
    "stream_d768": (66000, 768, 40, 100, 150, 4, {}, {}, {}, "stream", True),
    "sharded": (30000, 64, 300, 50, 80, 8, {"shards": 4, "tie_order": "id_desc"}, {}, {}, "tile", False),
}


@pytest.mark.parametrize("name", list(_L2_ROUTES))
def test_l2_scales_by_four_to_the_s(name, monkeypatch):
    from oracle import knn as ok
    n, d, nq, k, clones, bases, kw, env, opts, kind, screened = _L2_ROUTES[name]
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    X, Q = planted(2000 + d + nq, n, d, nq, clones, bases)
    if nq >= 20:
        assert _zero_margin_would_lose(X, Q, k, 1) >= 0.3
    D0, I0, idx = _search(X, Q, k, 1, **kw)
    _assert_kind(idx, nq, k, kind, name)
    assert (D0 > 0).all()
    _check_anchor(X, Q, k, 1, D0, I0, idx, screened, tie_order=kw.get("tie_order", "id_asc"))
    del idx
    for s in L2_SWEEP:
        D, I, idx = _search(scaled(X, s), scaled(Q, s), k, 1, **kw)
        _assert_kind(idx, nq, k, kind, name)
        assert np.array_equal(I, I0), f"{name}: ids differ at s = {s}"
        assert np.array_equal(D, scaled(D0, 2 * s)), f"{name}: scores are not 4^s D0 at s = {s}"
        del idx
    # about 1 row in 50 at 2^62: ||x||^2 overflows, the distance is infinite and such a row never enters
    rng = np.random.default_rng(d)
    Xo = X.copy()
    big = rng.choice(n, n // 50, replace=False)
    Xo[big] = scaled(Xo[big], 62)
    D, I, idx = _search(Xo, Q, k, 1, **kw)
    Do, Io = ok.knn(Xo, Q, k, metric=1, tie_order=kw.get("tie_order", "id_asc"))
    assert not np.isin(Io, big).any()
    assert np.array_equal(I, Io) and np.array_equal(D, Do), f"{name}: rows with an overflowing ||x||^2"


@pytest.mark.parametrize("form", ["numpy", "faiss"])
@pytest.mark.parametrize("metric", [0, 1])
def test_l2norm_flat_is_bit_identical_under_power_of_two_scales(form, metric):
    from oracle import knn as ok
    n, d, nq, k = 30000, 128, 300, 50
    X, Q = planted(3000 + metric, n, d, nq, 80, 8)
    kw = dict(factory="L2norm,Flat", l2norm_form=form)
    D0, I0, idx = _search(X, Q, k, metric, **kw)
    assert idx.scan_kind(nq, k) == "tile"
    _check_anchor(X, Q, k, metric, D0, I0, idx, True, l2norm=True, l2norm_form=form)
    del idx
    for s in L2NORM_SWEEP:
        for a, b in (((s, -s), (-s, s)) if metric == 0 else ((s, s),)):
            D, I, idx = _search(scaled(X, a), scaled(Q, b), k, metric, **kw)
            assert np.array_equal(I, I0) and np.array_equal(D, D0), f"L2norm {form}, metric {metric}: X 2^{a}, Q 2^{b}"
            del idx
    # beyond: every squared norm overflows and both forms make the rows zero -- the oracle decides
    Xs, Qs = scaled(X, 64), scaled(Q, 64)
    D, I, idx = _search(Xs, Qs, k, metric, **kw)
    Do, Io = ok.knn(Xs, Qs, k, metric=metric, l2norm=True, l2norm_form=form)
    assert np.array_equal(I, Io) and np.array_equal(D, Do), f"L2norm {form}, metric {metric}: overflowing squared norms"
