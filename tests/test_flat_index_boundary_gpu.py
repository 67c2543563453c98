"""One host layer for three classes: MI355XFlatIndex, ShardedFlatIndex (outside torch.distributed: one rank) and
LocalShardsFlatIndex (three shards on cuda:0) through the same ``search_batch`` staging, the same whole-panel batching of
``add_vectors(dataset, column=...)`` and the same ``load_rows``.  The data sits on an integer lattice, so every score is exact
in fp32 and the oracle's answer is the only right one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAGGED = (1, 62, 1, 100, 7, 64, 129, 300, 5, 331)  # rows of the pieces the column is concatenated from (1000 in all)
KINDS = ("single", "sharded", "local_shards")


def _make(kind, **kw):
    from viquae_amd.index import MI355XFlatIndex
    from viquae_amd.sharded import LocalShardsFlatIndex, ShardedFlatIndex
    if kind == "single":
        return MI355XFlatIndex(**kw)
    if kind == "sharded":
        return ShardedFlatIndex(**kw)
    return LocalShardsFlatIndex([0, 0, 0], allow_repeated_devices=True, **kw)


def _stored_rows(index):
    """The rows an index holds, shard after shard."""
    shards = getattr(index, "shards", None) or [getattr(index, "local", index)]
    return np.concatenate([sh.reconstruct_n() for sh in shards if sh.ntotal])


@pytest.fixture(scope="module")
def lattice():
    rng = np.random.default_rng(5)
    return rng.integers(-4, 5, (1000, 24)).astype(np.float32), rng.integers(-4, 5, (300, 24)).astype(np.float32)


@pytest.fixture(scope="module")
def oracle_top7(lattice):
    """(D, I) [300, 7] per metric: the first nq rows and k columns of it answer every (nq, k <= 7) of the same queries."""
    from oracle import knn as ok
    X, Q = lattice
    return {metric: ok.knn(X, Q, 7, metric=metric) for metric in (0, 1)}


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_search_batch_staging_is_grown_reused_rekeyed_and_bypassed(lattice, oracle_top7, kind, metric):
    X, Q = lattice
    Do, Io = oracle_top7[metric]  # (FAISS's two forms of the L2 distance, chosen by nq, are both exact on the lattice)
    index = _make(kind, string_factory="Flat", metric_type=metric)
    index.add_vectors(X)
    assert index._io is None
    staged = []
    for nq, k in ((5, 3), (300, 3), (5, 7), (0, 3), (257, 3)):
        D, I = index.search_batch(Q[:nq], k)
        assert D.dtype == np.float32 and I.dtype == np.dtype(int) and D.shape == I.shape == (nq, k)
        assert np.array_equal(I, Io[:nq, :k]) and np.array_equal(D, Do[:nq, :k]), (kind, metric, nq, k)
        staged.append(index._io)
    # 5 queries: the smallest staging (256 rows); 300: grown to 512; k = 7: other result buffers; no query: staging untouched;
    # k = 3 again: re-keyed once more
    assert [io[0].shape[0] for io in staged] == [256, 512, 256, 256, 512] and staged[3] is staged[2]
    assert [io[2].shape[1] for io in staged] == [3, 3, 7, 7, 3]
    again = index.search_batch(Q[:100], 3)
    assert index._io is staged[4] and np.array_equal(again[1], Io[:100, :3])  # fits: reused as it is
    D, I = index.search_batch(Q.astype(np.float64), 3)
    assert D.dtype == np.float32 and np.array_equal(I, Io[:, :3]) and np.array_equal(D, Do[:, :3])


@pytest.fixture(scope="module")
def ragged_column(lattice):
    """The lattice rows as a `list<float>` column of several Arrow chunks, none of them a whole number of panels."""
    import datasets
    X, _ = lattice
    cuts = np.cumsum((0,) + RAGGED)
    ds = datasets.concatenate_datasets([datasets.Dataset.from_dict({"vec": list(X[a:b])}) for a, b in zip(cuts[:-1], cuts[1:])])
    assert len(ds) == len(X) and ds.data.column("vec").num_chunks >= len(RAGGED)
    return ds


@pytest.fixture(scope="module")
def rows_of_one_add(lattice):
    """factory -> what ONE MI355XFlatIndex.add of the whole matrix stores."""
    from viquae_amd.index import MI355XFlatIndex
    X, _ = lattice
    out = {}
    for factory in ("Flat", "L2norm,Flat"):
        one = MI355XFlatIndex(string_factory=factory, metric_type=0)
        one.add(X)
        out[factory] = one.reconstruct_n()
    return out


@pytest.mark.parametrize("factory,metric", [("Flat", 1), ("L2norm,Flat", 0)])
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_column_add_save_and_load_rows_keep_every_row(lattice, ragged_column, rows_of_one_add, tmp_path, monkeypatch,
                                                                kind, factory, metric):
    from viquae_amd import sharded
    monkeypatch.delenv("MQ_KNN_L2NORM_FORM", raising=False)
    index = _make(kind, string_factory=factory, metric_type=metric)
    index.add_vectors(ragged_column, column="vec")
    assert index.ntotal == 1000 and index.d == 24
    assert _stored_rows(index).tobytes() == rows_of_one_add[factory].tobytes()
    path = str(tmp_path / "kb.mqflat")
    index.save(path)
    # the constructor says the opposite of the file on both counts, and names no arithmetic for "L2norm,"
    other = dict(string_factory="Flat" if "L2norm" in factory else "L2norm,Flat", metric_type=1 - metric)
    if kind == "sharded":  # make_flat_index only builds it inside a torch.distributed job of several ranks
        empty = sharded.ShardedFlatIndex(**other)
    else:
        real = sharded.LocalShardsFlatIndex
        monkeypatch.setattr(sharded, "LocalShardsFlatIndex", lambda devices, **kw: real(devices, allow_repeated_devices=True, **kw))
        empty = sharded.make_flat_index(device=None if kind == "single" else [0, 0, 0], **other)
    assert type(empty) is type(index)
    back = empty.load_rows(path)
    assert back is empty and back.ntotal == 1000 and back.d == 24
    assert _stored_rows(back).tobytes() == rows_of_one_add[factory].tobytes()
    shards = list(getattr(back, "shards", [])) or ([back.local] if kind == "sharded" else [back])
    for part in [back] + shards:
        assert part.metric_type == metric and part.do_l2norm == ("L2norm" in factory), (kind, type(part).__name__)
    if "L2norm" in factory:  # a stored "L2norm,Flat" index is FAISS's object: its queries take FAISS's arithmetic
        assert [sh.l2norm_form for sh in shards] == ["faiss"] * len(shards)
    with pytest.raises(ValueError, match="EMPTY"):
        back.load_rows(path)


@pytest.mark.parametrize("metric", [0, 1])
def test_knowledge_base_loads_a_file_into_the_index_its_device_key_names(lattice, oracle_top7, tmp_path, monkeypatch, metric):
    import datasets
    from viquae_amd import sharded
    from viquae_amd.index import MI355XFlatIndex
    from viquae_amd.ir.search import KnowledgeBase
    X, Q = lattice
    saved = MI355XFlatIndex(string_factory="Flat", metric_type=metric)
    saved.add(X)
    want = saved.search_batch(Q, 7)
    assert np.array_equal(want[1], oracle_top7[metric][1]) and np.array_equal(want[0], oracle_top7[metric][0])
    path = str(tmp_path / "kb.index")
    saved.save(path)
    ds = datasets.Dataset.from_dict({"passage": [str(i) for i in range(len(X))]})
    real = sharded.LocalShardsFlatIndex
    monkeypatch.setattr(sharded, "LocalShardsFlatIndex", lambda devices, **kw: real(devices, allow_repeated_devices=True, **kw))
    for device, cls in ((None, MI355XFlatIndex), ([0, 0], real)):
        kb = KnowledgeBase(dataset=ds, index_kwargs={"idx": {"column": "vec", "load": True, "file": path, "device": device}})
        assert type(ds._indexes["idx"]) is cls and ds._indexes["idx"].metric_type == metric
        D, I = kb.search_batch("idx", Q, k=7)
        assert np.array_equal(I, want[1]) and np.array_equal(D, want[0])
