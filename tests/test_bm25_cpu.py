"""CPU suite of the BM25 index (viquae_amd/ir/bm25.py): the host-side analysis and statistics, the numpy restatement the GPU tests
compare with (tests/bm25_restatement.py) against a worked example, the config surface of ``kind: "BM25"``, and the properties the
GPU cases rely on, checked on the restatement alone.  No test here touches a GPU."""
import math

import numpy as np
import pytest

from tests import bm25_restatement as br
from tests import config_surface

TOKENISER_TABLE = [
    ("The Quick BROWN Fox", ["the", "quick", "brown", "fox"]),                   # case folding
    ("Shaquille O'Neil", ["shaquille", "o'neil"]),                                # apostrophe between letters
    ("pi is 3.14", ["pi", "is", "3.14"]),                                         # full stop between digits
    ("see a.b now", ["see", "a.b", "now"]),                                       # full stop between letters
    ("1,000 men; 2;3", ["1,000", "men", "2;3"]),                                  # comma / semicolon between digits
    ("foo_bar _x_ __", ["foo_bar", "_x_"]),                                       # underscore joins; alone it is nothing
    ("well-known state-of-the-art", ["well", "known", "state", "of", "the", "art"]),  # hyphens separate
    ("Really?! Yes. 12: a, b.", ["really", "yes", "12", "a", "b"]),               # trailing punctuation
    ("x" * 600, ["x" * 255, "x" * 255, "x" * 90]),                                # a run of 600 letters
    ("Café MÜNCHEN naïve", ["café", "münchen", "naïve"]),                         # accented letters
    ("日本語のカナ abc", ["日", "本", "語", "の", "カ", "ナ", "abc"]),                  # Han / Hiragana / Katakana
    ("", []),                                                                     # empty
    ("?!... -- ;:'", []),                                                         # pure punctuation
    ("a1b2 1.a a:b 1:2 3'4", ["a1b2", "1", "a", "a:b", "1", "2", "3", "4"]),      # mixed runs; joins need matching neighbours
]


@pytest.mark.parametrize("text, expected", TOKENISER_TABLE, ids=[f"case{i}" for i in range(len(TOKENISER_TABLE))])
def test_tokeniser_table(text, expected):
    from viquae_amd.ir.bm25 import standard_tokenize
    assert standard_tokenize(text) == expected
    assert br.tokenize(text) == expected  # the restatement's independent scan agrees


def test_tokenisers_agree_on_the_shared_texts():
    from viquae_amd.ir.bm25 import standard_tokenize
    for text in br.TEXTS + br.TEXT_QUERIES + ["_'a a__ __a 1.a a.b.c 1,2,3 éa x­b 日゙本", "O’Neil ١٢٣ abc̀.def"]:
        assert standard_tokenize(text) == br.tokenize(text), text


def test_length_code_all_256_codes():
    from viquae_amd.ir.bm25 import LENGTH_TABLE, byte4_to_int, encode_lengths, int_to_byte4
    decoded = [byte4_to_int(c) for c in range(256)]
    assert all(a < b for a, b in zip(decoded, decoded[1:]))               # strictly increasing
    assert all(int_to_byte4(decoded[c]) == c for c in range(256))         # encode(decode(c)) == c
    assert decoded[:24] == list(range(24))                                # exact below 24
    assert decoded == [br.decode_length(c) for c in range(256)] == LENGTH_TABLE.tolist()
    lengths = list(range(0, 5000)) + [2 ** e + d for e in range(13, 31) for d in (-1, 0, 1)] + [2 ** 31 - 1]
    for n in lengths:
        c = int_to_byte4(n)
        back = byte4_to_int(c)
        assert c == br.encode_length(n) and 0 <= c <= 255
        assert back <= n and (n < 24) <= (back == n)
        assert n == 0 or (n - back) / n < 1 / 8                           # four significant bits
    assert np.array_equal(encode_lengths(np.array(lengths)), [int_to_byte4(n) for n in lengths])


def _worked_example():
    # a=0 b=1 c=2 d=3 e=4; "zzz" is term 9, which no document holds
    docs = [[0, 1, 1, 2], [1, 2, 2, 2, 3], [0, 0, 4]]
    query = [1, 1, 9, 0]  # b b zzz a -> clauses (b, x2), (a, x1)
    return docs, query


def test_restatement_against_a_worked_example():
    docs, query = _worked_example()
    k1, b = 1.2, 0.75
    r = br.Restatement([np.array(d) for d in docs], 10, k1, b)
    assert (r.doc_count, r.sum_total_term_freq, float(r.avgdl)) == (3, 12, 4.0)
    assert r.doc_freq.tolist() == [2, 2, 2, 1, 1, 0, 0, 0, 0, 0]
    assert [t for t, _ in r.clauses(query)] == [1, 0]

    def idf(df):
        return math.log(1 + (3 - df + 0.5) / (df + 0.5))

    def impact(tf, length):  # lengths below 24 are stored exactly
        return tf / (tf + k1 * ((1 - b) + b * length / 4.0))

    expected = [2 * idf(2) * impact(2, 4) + idf(2) * impact(1, 4),   # d0: b twice, a once
                2 * idf(2) * impact(1, 5),                           # d1: b once
                idf(2) * impact(2, 3)]                               # d2: a twice
    got = r.scores(query)
    assert got.dtype == np.float32 and np.allclose(got.astype(np.float64), expected, rtol=0, atol=1e-6)
    D, I = r.search([query, [9], []], 4)
    order = sorted(range(3), key=lambda i: -expected[i])   # by the float64 formula: d0 (1.18...), d1 (0.38...), d2 (0.31...)
    assert order == [0, 1, 2] and I[0].tolist() == order + [-1] and D[0, 3] == -np.inf and np.array_equal(D[0, :3], got[order])
    assert (I[1:] == -1).all() and np.isneginf(D[1:]).all()


def test_host_statistics_match_the_restatement():
    """The product's host code (CSR, codes, cache, idf) and the restatement's agree bit for bit on a corpus with every special term."""
    from viquae_amd.ir import bm25
    R = 64
    r = br.Restatement(br.corpus(3 * R + 1, R), br.VOCABULARY_SIZE, 0.5, 0.3)
    ptr, doc, tf, lengths = bm25.build_csr(br.corpus(3 * R + 1, R), br.VOCABULARY_SIZE)
    rptr, rdoc, rtf, _ = r.csr()
    assert np.array_equal(ptr, rptr) and np.array_equal(doc, rdoc) and np.array_equal(tf, rtf)
    assert ptr.dtype == np.int64 and doc.dtype == np.int32 and tf.dtype == np.int32
    assert np.array_equal(bm25.encode_lengths(lengths), r.codes)
    assert np.array_equal(bm25.norm_cache(0.5, 0.3, r.avgdl).view(np.uint32), r.cache.view(np.uint32))
    assert np.array_equal(bm25.idf_weights(r.doc_count, r.doc_freq).view(np.uint32), r.idf.view(np.uint32))


def test_index_kind_bm25_exists():
    from viquae_amd.ir.search import IndexKind
    assert IndexKind["BM25"].name == "BM25"
    assert {k.name for k in IndexKind} >= {"FAISS", "ES", "PYSERINI", "BM25"}


def _shipped_bm25_index_kwargs():
    config = config_surface.configs()["experiments/ir/viquae/bm25/config.json"]
    (kb,) = config["kb_kwargs"].values()
    return kb["index_kwargs"]["BM25"]


def test_es_index_config_parsing():
    import copy
    from viquae_amd.ir.bm25 import parse_es_index_config
    es = _shipped_bm25_index_kwargs()["es_index_config"]
    assert parse_es_index_config(es) == (0.5, 0.3)
    assert parse_es_index_config(None) == (1.2, 0.75) and parse_es_index_config({}) == (1.2, 0.75)
    other = copy.deepcopy(es)
    other["mappings"]["properties"]["text"]["analyzer"] = "english"
    with pytest.raises(NotImplementedError, match="analyzer"):
        parse_es_index_config(other)
    missing = copy.deepcopy(es)
    missing["settings"]["similarity"] = {}
    with pytest.raises(ValueError):
        parse_es_index_config(missing)


def test_bm25_kind_refuses_before_touching_a_device():
    """The argument checks of ``add_or_load_index(kind="BM25")`` that need no GPU: another analyzer, and load without a file."""
    import copy
    from viquae_amd.ir.search import KnowledgeBase
    kb = KnowledgeBase(load_dataset=False)
    kwargs = copy.deepcopy(_shipped_bm25_index_kwargs())
    kwargs.pop("es")
    with pytest.raises(ValueError, match="file"):
        kb.add_or_load_index(index_name="BM25", kind="BM25", **kwargs)          # "load": true without `file`
    kwargs["es_index_config"]["mappings"]["properties"]["text"]["analyzer"] = "whitespace"
    with pytest.raises(NotImplementedError, match="analyzer"):
        kb.add_or_load_index(index_name="BM25", kind="BM25", **{**kwargs, "load": False})
    # the unmodified entry still stops with the documented out-of-scope error
    with pytest.raises(NotImplementedError, match="Elasticsearch"):
        kb.add_or_load_index(index_name="BM25", **_shipped_bm25_index_kwargs())


def test_conditions_of_the_gpu_cases(hip_lib):
    """What tests/test_bm25_gpu.py takes for granted about its corpora, on the restatement alone (R from the library)."""
    R = hip_lib.mq_bm25_block_rows()
    assert R >= 1024 and R & (R - 1) == 0
    qs = br.queries()
    assert len(qs) == 37 and max(len(set(q)) for q in qs) >= 40 and [] in qs
    for N in br.corpus_sizes(R):
        r = br.restated(N, R)
        hits = [r.hits(q) for q in qs]
        # a query with fewer hits than some tested k (and at least one hit), one with none at all ...
        assert any(0 < h < k for h in hits for k in br.K_VALUES) and 0 in hits
        # ... and, where the corpus can hold more than k documents, one with more hits than every tested k
        if N > max(br.K_VALUES):
            assert max(hits) > max(br.K_VALUES)
        elif N > 1:
            assert max(hits) > min(br.K_VALUES)
        assert r.doc_freq[br.T_EVERY] == N and r.doc_freq[br.T_UNUSED] == 0
        assert r.post_docs[br.T_LAST].tolist() == [N - 1]
        if N > R + 2:
            assert r.post_docs[br.T_BLOCK_END].tolist() == [R - 3, R - 2, R - 1]       # ends at block 0's last row
            assert r.post_docs[br.T_BLOCK_START].tolist() == [R, R + 1, R + 2]         # starts at block 1's first row
        # the every-document term's postings cross every block boundary
        every = r.post_docs[br.T_EVERY]
        assert all(b - 1 in every and b in every for b in range(R, N, R))
    # the tie corpus: one score for all 2R documents, so the tied run across the 100th place spans the block boundary
    tie = br.Restatement(br.tie_corpus(R), 16)
    s = tie.scores([4, 3])
    assert len(s) == 2 * R and len(np.unique(s.view(np.uint32))) == 1 and s[0] > 0
    assert tie.search([[4, 3]], 100, "id_asc")[1][0].tolist() == list(range(100))
    assert tie.search([[4, 3]], 100, "id_desc")[1][0].tolist() == list(range(2 * R - 1, 2 * R - 101, -1))
    # ties inside a Zipfian corpus too: the every-document term scores by length code alone
    s = br.restated(3 * R + 1, R).scores([br.T_EVERY])
    kth = np.sort(s)[::-1][99]
    tied = np.flatnonzero(s == kth)
    assert len(tied) > 1 and tied.min() < R <= tied.max()


def test_conditions_of_the_clause_batch_cases(hip_lib):
    """What tests/test_bm25_clauses_gpu.py takes for granted, on the restatement alone (CB and R from the library)."""
    CB, R = hip_lib.mq_bm25_clause_batch(), hip_lib.mq_bm25_block_rows()
    counts = br.clause_counts(CB)
    assert counts[br.ZERO_WEIGHT_QUERY] == 1 and counts[br.LONG_QUERY] == 2 * CB + 1
    assert sorted(counts[1:]) == [0, 1, CB - 1, CB, CB + 1, 2 * CB, 2 * CB + 1, 3 * CB + 5]
    batches = [-(-c // CB) for c in counts[1:]]                  # batches a workgroup walks for each query
    assert batches == [1, 0, 1, 1, 2, 2, 3, 4]
    assert counts[3] < CB == counts[4] < counts[5] and counts[6] == 2 * CB < counts[7] and counts[8] > 3 * CB
    # the planted positions: the last clause of the first batch, the first clause of the second, the query's last clause
    assert br.plant_positions(2 * CB + 1, CB) == [CB - 1, CB, 2 * CB]
    assert (CB - 1) // CB == 0 and CB // CB == 1 and (CB - 2) // CB == 0
    assert br.plant_positions(CB + 1, CB) == [CB - 1, CB] and br.plant_positions(CB, CB) == [CB - 1]
    assert br.plant_positions(CB - 1, CB) == [CB - 2] and br.plant_positions(1, CB) == [0] and br.plant_positions(0, CB) == []
    V = br.VOCABULARY_SIZE
    assert sorted(br.CLAUSE_PLANTS.values()) == sorted([br.T_EVERY, br.T_UNUSED, -1, V, V + 7, 2 ** 31 - 1, -2 ** 31])
    rest = br.restated(R + 37, R)
    assert rest.V == V and rest.doc_freq[br.T_UNUSED] == 0 and rest.doc_freq[br.T_EVERY] == rest.N
    named = set()
    for name, plant in br.CLAUSE_PLANTS.items():
        queries = br.clause_queries(CB, plant)
        assert [len(t) for t, _ in queries] == counts and all(t.dtype == np.int32 and w.dtype == np.float32 for t, w in queries)
        qptr, cterm, cweight = br.pack_raw(queries)
        assert qptr[-1] == len(cterm) == len(cweight) == sum(counts)
        # in ONE launch no query of a batch or more starts at a multiple of CB in cterm (its batches are not the array's)
        assert all(qptr[j] % CB for j, c in enumerate(counts) if c >= CB)
        for j, (t, w) in enumerate(queries):
            if j == br.ZERO_WEIGHT_QUERY:
                assert t.tolist() == [br.T_EVERY] and w.tolist() == [0.0]
                continue
            at = br.plant_positions(len(t), CB)
            assert (t[at] == plant).all() and (w >= 0.1).all() and (w < 3).all()
            rest_of = np.delete(t, at)
            assert ((rest_of >= 0) & (rest_of < V)).all() and (rest.doc_freq[rest_of] > 0).all()     # in-vocabulary ids
            named.update(rest_of.tolist())
            if len(t) > CB:   # a term recurs inside the first batch, and across batches
                assert len(set(t[:CB].tolist())) < CB and set(t[:CB].tolist()) & set(t[CB:].tolist())
        # the weight-0 query has no hits: every product is +0
        assert not br.scores_raw(rest, *queries[br.ZERO_WEIGHT_QUERY]).view(np.uint32).any()
    assert named >= set(range(br.ZIPF_TERMS)) | {br.T_EVERY, br.T_LAST, br.T_BLOCK_END, br.T_BLOCK_START}
    # scores_raw: what Restatement.scores gives on de-duplicated clauses, and no de-duplication of its own
    q = br.queries()[4]
    terms, weights = zip(*rest.clauses(q))
    assert np.array_equal(br.scores_raw(rest, terms, weights).view(np.uint32), rest.scores(q).view(np.uint32))
    twice = br.scores_raw(rest, [br.T_EVERY, br.T_EVERY], [1.5, 1.5])
    assert np.array_equal(twice, br.scores_raw(rest, [br.T_EVERY, -1, V, br.T_UNUSED, br.T_EVERY], [1.5, 9, 9, 9, 1.5]))
    assert (twice > br.scores_raw(rest, [br.T_EVERY], [1.5])).all()
    # the order of the clauses is visible in the bits: a kernel that added the batches (or the clauses) in another order would be seen
    t, w = br.clause_queries(CB, br.T_EVERY)[br.LONG_QUERY]
    forward, backward = br.scores_raw(rest, t, w), br.scores_raw(rest, t[::-1], w[::-1])
    assert (forward.view(np.uint32) != backward.view(np.uint32)).any()
    swapped = np.concatenate([np.arange(CB, 2 * CB), np.arange(CB), [2 * CB]])          # the first two batches exchanged
    assert (forward.view(np.uint32) != br.scores_raw(rest, t[swapped], w[swapped]).view(np.uint32)).any()
    # ... and so is a batch that is skipped
    assert (forward.view(np.uint32) != br.scores_raw(rest, t[:CB], w[:CB]).view(np.uint32)).any()
    assert (forward.view(np.uint32) != br.scores_raw(rest, np.delete(t, np.arange(CB, 2 * CB)), np.delete(w, np.arange(CB, 2 * CB))).view(np.uint32)).any()


def test_search_entry_validates_before_any_hip_call(hip_lib):
    assert hip_lib.mq_bm25_search_f32(None, None, None, 10, 5, None, None, None, 1, 5, 0, 0, None, None, None, 0, 0, None) == -1
    assert hip_lib.mq_topk_rows_f32(None, 1, 10, 5, 0, 0, None, None, None, 0, None) == -1
    assert hip_lib.mq_topk_rows_workspace_bytes(4, 2049) == 0 and hip_lib.mq_topk_rows_workspace_bytes(4, 2048) > 0
    assert hip_lib.mq_bm25_chunk_queries(1000, 37, 1000 * 4 * 5) == 5 and hip_lib.mq_bm25_chunk_queries(1000, 37, 0) == 1
    assert hip_lib.mq_bm25_chunk_queries(1000, 37, 1 << 30) == 37
    assert hip_lib.mq_bm25_clause_batch() >= 2
    import ctypes
    out = (ctypes.c_int64 * 8)()
    assert hip_lib.mq_topk_rows_launch_info(4, 70_001, out) == 0
    assert list(out) == [5, 6, 53, 42, 32, 21, 10, 0]                    # 5 workgroups a row, six passes of 11 / 11 / 10 / 11 / 11 / 10 bits
    assert hip_lib.mq_topk_rows_launch_info(1, 1, out) == 0 and out[0] == 1
    assert hip_lib.mq_topk_rows_launch_info(2048, 17_000, out) == 0 and out[0] == 1
    for rows, N in ((0, 10), (65536, 10), (1, 0), (1, 1 << 31)):          # what mq_topk_rows_f32 refuses
        assert hip_lib.mq_topk_rows_launch_info(rows, N, out) == -1
        assert hip_lib.mq_topk_rows_f32(1, rows, N, 5, 0, 0, 1, 1, 1, 1 << 40, None) == -1
    assert hip_lib.mq_topk_rows_launch_info(1, 10, None) == -1
