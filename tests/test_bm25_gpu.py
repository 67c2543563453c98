"""GPU suite of the BM25 index (viquae_amd/ir/bm25.py, csrc/bm25.hip): every result equals the numpy restatement
(tests/bm25_restatement.py) BIT FOR BIT -- scores compared as uint32, ids exactly.  Corpus sizes follow the scoring kernel's
document block R (read from the library): 1, R - 1, R + 37 and 3R + 1 documents.  Each index and each restatement is built once
per size and shared."""
import functools

import numpy as np
import pytest

from tests import bm25_restatement as br

pytestmark = pytest.mark.gpu


def _R():
    from viquae_amd import _lib
    return int(_lib.load().mq_bm25_block_rows())


@functools.lru_cache(maxsize=None)
def _index(N, tie_order="id_asc"):
    from viquae_amd.ir.bm25 import MI355XBM25Index
    index = MI355XBM25Index(tie_order=tie_order)
    index.add_token_ids(br.corpus(N, _R()), br.VOCABULARY_SIZE)
    return index


def _same(got, want):
    D, I = got
    assert D.dtype == np.float32 and D.shape == want[0].shape and I.shape == want[1].shape
    assert np.array_equal(np.asarray(I, dtype=np.int64), want[1])
    assert np.array_equal(np.ascontiguousarray(D).view(np.uint32), want[0].view(np.uint32))


SIZES = ("1", "R-1", "R+37", "3R+1")


def _size(name):
    return dict(zip(SIZES, br.corpus_sizes(_R())))[name]


@pytest.mark.parametrize("tie_order", ["id_asc", "id_desc"])
@pytest.mark.parametrize("k", br.K_VALUES)
@pytest.mark.parametrize("nq", [1, 37])
@pytest.mark.parametrize("size", SIZES)
def test_search_equals_the_restatement(size, nq, k, tie_order):
    """Covers, through tests/bm25_restatement.queries(): a term in every document, one only in the last document, one whose postings
    end at a block's last row and one that starts at a block's first row, an empty query, an all-out-of-vocabulary query (both all
    -1 / -inf), 40 distinct terms, a repeated term, fewer than k hits and more than k hits (tests/test_bm25_cpu.py checks that the
    corpora deliver these)."""
    N = _size(size)
    index = _index(N)
    index.tie_order = tie_order
    qs = br.queries()
    qs = qs[:nq] if nq > 1 else [qs[4]]  # the single query: the 40-term one
    got = index.search_batch(qs, k)
    _same(got, br.restated(N, _R()).search(qs, k, tie_order))
    if nq > 1:
        assert (got.total_indices[2:4] == -1).all() and np.isneginf(got.total_scores[2:4]).all()


def test_impacts_equal_the_restatement():
    N = _size("R+37")
    assert np.array_equal(_index(N).impacts().view(np.uint32), br.restated(N, _R()).csr()[3].view(np.uint32))


@pytest.mark.parametrize("tie_order", ["id_asc", "id_desc"])
def test_identical_documents_ties_decide_everything(tie_order):
    from viquae_amd.ir.bm25 import MI355XBM25Index
    R = _R()
    index = MI355XBM25Index(tie_order=tie_order)
    index.add_token_ids(br.tie_corpus(R), 16)
    want = br.Restatement(br.tie_corpus(R), 16).search([[4, 3], [9, 9]], 100, tie_order)
    got = index.search_batch([[4, 3], [9, 9]], 100)
    _same(got, want)
    first = list(range(100)) if tie_order == "id_asc" else list(range(2 * R - 1, 2 * R - 101, -1))
    assert got.total_indices[0].tolist() == first


def test_query_chunk_boundaries_change_nothing():
    """A workspace budget of five score rows: 37 queries take eight launches; the results are those of one."""
    N = _size("R+37")
    index, qs = _index(N), br.queries()
    index.tie_order = "id_asc"
    whole = index.search_batch(qs, 100)
    budget = index.workspace_bytes
    try:
        index.workspace_bytes = N * 4 * 5
        assert index.query_chunk(len(qs)) == 5
        pieces = index.search_batch(qs, 100)
    finally:
        index.workspace_bytes = budget
    assert index.query_chunk(len(qs)) == 37
    _same(pieces, (whole.total_scores, np.asarray(whole.total_indices, dtype=np.int64)))
    _same(whole, br.restated(N, _R()).search(qs, 100))


def test_topk_rows_primitive_on_a_plain_matrix():
    """mq_topk_rows_f32 on its own: rows with many equal values, zeros (no hits) and fewer than k positives."""
    import torch
    from viquae_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(5)
    N, k = 70_001, 300
    X = np.zeros((4, N), dtype=np.float32)
    X[0] = rng.integers(0, 50, N).astype(np.float32) / 7          # 50 distinct values: long tied runs
    X[1, rng.choice(N, 120, replace=False)] = rng.random(120).astype(np.float32) + 0.1   # fewer than k hits
    X[2] = rng.random(N).astype(np.float32) + 1e-3                # distinct values
    x = torch.from_numpy(X).cuda()
    for flags, tie in ((0, "id_asc"), (2, "id_desc")):
        D = torch.empty((4, k), dtype=torch.float32, device="cuda")
        I = torch.empty((4, k), dtype=torch.int64, device="cuda")
        ws = torch.empty(int(lib.mq_topk_rows_workspace_bytes(4, k)), dtype=torch.uint8, device="cuda")
        _lib.check(lib.mq_topk_rows_f32(x.data_ptr(), 4, N, k, flags, 1000, D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(),
                                        torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        for row in range(4):
            d, i = br.topk(X[row], k, tie)
            assert np.array_equal(I[row, :len(i)].cpu().numpy(), i + 1000) and (I[row, len(i):] == -1).all()
            assert np.array_equal(D[row, :len(d)].cpu().numpy().view(np.uint32), d.view(np.uint32))
            assert torch.isneginf(D[row, len(d):]).all()


@functools.lru_cache(maxsize=None)
def _text_index():
    from viquae_amd.ir.bm25 import MI355XBM25Index
    index = MI355XBM25Index(k1=0.5, b=0.3)
    index.add_documents(br.TEXTS)
    return index


def _text_ids():
    tokens = [br.tokenize(t) for t in br.TEXTS]
    vocabulary = sorted(set(t for doc in tokens for t in doc))
    term_id = {t: i for i, t in enumerate(vocabulary)}
    docs = [np.array([term_id[t] for t in doc], dtype=np.int64) for doc in tokens]
    qs = [[term_id.get(t, -1) for t in br.tokenize(q)] for q in br.TEXT_QUERIES]
    return vocabulary, docs, qs


def test_text_path_equals_token_ids_of_the_restatements_tokenisation():
    from viquae_amd.ir.bm25 import MI355XBM25Index
    vocabulary, docs, qs = _text_ids()
    text = _text_index()
    assert text.vocabulary == vocabulary
    ids = MI355XBM25Index(k1=0.5, b=0.3)
    ids.add_token_ids(docs, len(vocabulary))
    for name in ("ptr", "doc", "tf", "codes"):
        assert np.array_equal(getattr(text, name), getattr(ids, name))
    got = text.search_batch(br.TEXT_QUERIES, 4)
    _same(got, tuple(np.asarray(a) for a in ids.search_batch(qs, 4)))
    _same(got, br.Restatement(docs, len(vocabulary), 0.5, 0.3).search(qs, 4))
    assert got.total_indices[0, 0] == 4  # "the the the fox" is the best match for "the fox"
    one = text.search(br.TEXT_QUERIES[0], 4)
    assert np.array_equal(one.indices, got.total_indices[0]) and np.array_equal(one.scores, got.total_scores[0])


def test_set_bm25_equals_a_fresh_build():
    from viquae_amd.ir.bm25 import MI355XBM25Index
    R = _R()
    N = R - 1
    index = MI355XBM25Index()
    index.add_token_ids(br.corpus(N, R), br.VOCABULARY_SIZE)
    index.set_bm25(0.5, 0.3)
    fresh = MI355XBM25Index(k1=0.5, b=0.3)
    fresh.add_token_ids(br.corpus(N, R), br.VOCABULARY_SIZE)
    assert np.array_equal(index.impacts().view(np.uint32), fresh.impacts().view(np.uint32))
    qs = br.queries()
    want = br.Restatement(br.corpus(N, R), br.VOCABULARY_SIZE, 0.5, 0.3).search(qs, 100)
    _same(index.search_batch(qs, 100), want)
    _same(fresh.search_batch(qs, 100), want)


def test_save_load_round_trip(tmp_path):
    from viquae_amd.ir.bm25 import MI355XBM25Index
    text = _text_index()
    path = tmp_path / "bm25.mqbm25"
    text.save(path)
    back = MI355XBM25Index.load(path)
    for name in ("ptr", "doc", "tf", "codes", "doc_freq", "idf"):
        assert np.array_equal(getattr(text, name), getattr(back, name)), name
    assert (back.vocabulary, back.k1, back.b, back.doc_count, back.sum_total_term_freq, back.ntotal) == \
           (text.vocabulary, 0.5, 0.3, text.doc_count, text.sum_total_term_freq, len(br.TEXTS))
    assert np.array_equal(text.impacts().view(np.uint32), back.impacts().view(np.uint32))
    _same(back.search_batch(br.TEXT_QUERIES, 3), tuple(np.asarray(a) for a in text.search_batch(br.TEXT_QUERIES, 3)))
    ids = _index(1)
    ids.save(tmp_path / "ids.mqbm25")
    again = MI355XBM25Index.load(tmp_path / "ids.mqbm25")
    assert again.vocabulary is None and np.array_equal(again.doc, ids.doc)
    with pytest.raises(ValueError):
        again.search_batch(["a string"], 1)  # a token-id index has no vocabulary


def test_dataset_level_api_and_errors(tmp_path):
    import datasets
    from datasets.search import MissingIndex
    from viquae_amd.ir.search import IndexKind, KnowledgeBase
    ds = datasets.Dataset.from_dict({"passage": br.TEXTS})
    kb = KnowledgeBase(dataset=ds)
    kb.add_or_load_index(column="passage", index_name="BM25", kind="BM25", key="input", k1=0.5, b=0.3, save_path=str(tmp_path / "i"))
    assert kb.indexes["BM25"].kind == IndexKind.BM25 and ds.list_indexes() == ["BM25"]
    want = _text_index().search_batch(br.TEXT_QUERIES, 3)
    _same(kb.search_batch("BM25", br.TEXT_QUERIES, k=3), tuple(np.asarray(a) for a in want))
    _same(ds.search_batch("BM25", br.TEXT_QUERIES, k=3), tuple(np.asarray(a) for a in want))
    res = ds.get_nearest_examples_batch("BM25", ["the the fox", "identifier"], k=2)
    assert [e["passage"][0] for e in res.total_examples] == [br.TEXTS[4], br.TEXTS[1]]
    scores, indices = kb.search_batch_if_not_None("BM25", ["the fox", None, "identifier"], k=3)
    assert len(scores[1]) == 0 and indices[2][0] == 1 and np.array_equal(indices[0], want.total_indices[0])
    with pytest.raises(ValueError):
        ds.search_batch("BM25", "the fox", k=3)            # a string, not a list of them
    with pytest.raises(MissingIndex):
        ds.search_batch("nope", ["the fox"], k=3)
    with pytest.raises(NotImplementedError):
        ds.search_batch("BM25", ["the fox"], k=2049)
    # load: the file `save_path` wrote, with the parameters of an es_index_config
    kb2 = KnowledgeBase(dataset=datasets.Dataset.from_dict({"passage": br.TEXTS}))
    es = {"settings": {"similarity": {"s": {"k1": 0.5, "b": 0.3}}}, "mappings": {"properties": {"text": {"analyzer": "standard", "similarity": "s"}}}}
    kb2.add_or_load_index(column="passage", index_name="BM25", kind="BM25", key="input", load=True, file=str(tmp_path / "i"),
                          es_index_config=es, es_index_name="ignored")
    _same(kb2.search_batch("BM25", br.TEXT_QUERIES, k=3), tuple(np.asarray(a) for a in want))
