"""BM25 passage search on the device: text analysis, index construction and ``MI355XBM25Index``.

The reference serves its text column through Elasticsearch (``"es": true`` / ``kind: "ES"``, meerqat/ir/search.py:81-205).  This
module restates, from the published Lucene 8 sources, what such an index computes under the shipped settings -- the ``standard``
analyzer and ``BM25Similarity`` -- and scores every passage exhaustively on the GPU (csrc/bm25.hip).  No Elasticsearch, Lucene or
pyserini exists in this image: parity with a live server is UNPINNED.  What is pinned is the arithmetic below, against the numpy
restatement committed with the tests (tests/bm25_restatement.py), bit for bit.

Analysis (``standard_tokenize``): the UAX#29 word tokeniser + lower-casing, no stop words, tokens of at most 255 characters.
  Rules implemented:
    * runs of letters (Unicode categories L*) and decimal digits (Nd) form tokens, letters and digits mixed freely;
    * ``'``, ``.`` and ``:`` between two letters join them; ``.``, ``,`` and ``;`` between two digits join them;
    * ``_`` joins on both sides (and stays at a token's edges), but a run of underscores alone is no token;
    * combining marks and format characters (Mn, Mc, Me, Cf) stay with the character they follow;
    * every Han, Hiragana or Katakana character is a token of its own;
    * every other character separates; a run longer than 255 characters is cut every 255.
  Knowingly simplified against UAX#29 / Lucene's StandardTokenizer:
    * only the ASCII MidLetter / MidNum / MidNumLet characters join (not U+2019, U+00B7, U+2027, full-width forms ...), and ``'``
      between two digits does not join;
    * Katakana runs are split into characters (Lucene keeps a run as one token); Hangul, Thai and other South-East Asian scripts
      are treated as ordinary letters (runs), emoji and regional indicators separate and give no token;
    * Hebrew double-quote rules (WB7b/c) are absent;
    * lower-casing is Python's ``str.lower()`` (full case mapping: U+0130 becomes two characters, final sigma is contextual),
      Lucene's is ``Character.toLowerCase`` per code point;
    * lengths count code points, Lucene counts UTF-16 units (they differ beyond the BMP only).

Statistics and scoring (Lucene 8 ``BM25Similarity``):
    docCount = documents with at least one token; docFreq[t]; sumTotalTermFreq; avgdl = float(sumTotalTermFreq / docCount)
    length code: one byte per document, ``SmallFloat.intToByte4`` (exact below 24, then 4 significant bits)
    cache[c] = k1 * ((1 - b) + b * byte4ToInt(c) / avgdl)              (float arithmetic)
    idf(t)   = float(ln(1 + (docCount - docFreq + 0.5) / (docFreq + 0.5)))
    impact   = float(tf / (tf + cache[code[doc]]))                     (double arithmetic; no (k1 + 1) numerator, as in Lucene 8)
    score    = the fp32 sum, in clause order, of weight * impact with weight = float(multiplicity) * idf
A query's clauses are its distinct in-vocabulary terms in order of first occurrence.

Layout: CSR postings, per term by ascending document id -- ptr [V + 1] int64, doc [nnz] int32, tf [nnz] int32, impact [nnz] fp32
(12 bytes per posting on the device + one length byte per document); term ids follow the lexicographic (code point) order of the
terms, so an index is a pure function of the corpus.  The CSR is built on the host with numpy (sort / unique: plumbing); the
impacts are computed on the device, so ``set_bm25`` re-weights a resident index without rebuilding it.
"""
import os
import re
import struct
import unicodedata
from pathlib import PurePath
from typing import Optional, Union

import numpy as np

from .. import _lib
from ..index import (FLAG_TIE_ID_DESC, MAX_K, TIE_ORDERS, BaseIndex, BatchedSearchResults, SearchResults, _resolve_device)

MAX_TOKEN_LENGTH = 255
DEFAULT_K1, DEFAULT_B = 1.2, 0.75            # Elasticsearch's defaults
DEFAULT_WORKSPACE_BYTES = 1 << 30            # budget of the dense [query chunk, N] fp32 score matrix
GRID_METHOD = "grid"                         # how search_grid scores a list of settings by default: "grid" | "loop" ("BM25": measured)
_MAGIC = b"MQBM2501"
_BUILD_DOCS = 1 << 16                        # documents whose (term, document) pairs are counted at once


# ---------------------------------------------------------------------------------------------------------------- analysis
def _is_cjk(cp):
    return (0x3040 <= cp <= 0x30FF or 0x31F0 <= cp <= 0x31FF or 0xFF66 <= cp <= 0xFF9F      # Hiragana, Katakana
            or 0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0xF900 <= cp <= 0xFAFF    # Han
            or 0x20000 <= cp <= 0x2FA1F or cp in (0x3005, 0x3007))


def _char_class(ch):
    """L letter, D digit, U underscore, C ideograph / kana, a ``'`` or ``:``, b ``.``, n ``,`` or ``;``, x extender, space other."""
    if ch == "_":
        return "U"
    if ch in "':":
        return "a"
    if ch == ".":
        return "b"
    if ch in ",;":
        return "n"
    cat = unicodedata.category(ch)
    if cat[0] == "L":
        # (the prolonged sound mark and the iteration marks are letters of the kana blocks: characters of their own too)
        return "C" if _is_cjk(ord(ch)) else "L"
    if cat == "Nd":
        return "D"
    if cat[0] == "M" or cat == "Cf":
        return "x"
    if cat == "Nl" and _is_cjk(ord(ch)):  # U+3007, the ideographic zero
        return "C"
    return " "


_TOKEN = re.compile(r"U*[LD](?:[LDU]|(?<=L)[ab](?=L)|(?<=D)[bn](?=D))*|Cc*")
_ASCII_CLASSES = "".join(_char_class(chr(i)) for i in range(128))
_ASCII_TABLE = {i: _ASCII_CLASSES[i] for i in range(128)}


def standard_tokenize(text):
    """Tokens of ``text`` under the ``standard`` analyzer as restated in this module's docstring (lower-cased strings)."""
    if not text:
        return []
    if text.isascii():
        classes = text.translate(_ASCII_TABLE)
    else:
        out, prev = [], " "
        for ch in text:
            c = _ASCII_CLASSES[ord(ch)] if ch < "\x80" else _char_class(ch)
            if c == "x":  # an extender takes the class of what it follows
                c = prev if prev in "LDU" else ("c" if prev in "Cc" else " ")
            out.append(c)
            prev = c
        classes = "".join(out)
    tokens = []
    for m in _TOKEN.finditer(classes):
        s, e = m.span()
        for i in range(s, e, MAX_TOKEN_LENGTH):
            tokens.append(text[i:min(i + MAX_TOKEN_LENGTH, e)].lower())
    return tokens


# ---------------------------------------------------------------------------------------------------------------- length code
_NUM_FREE_VALUES = 24  # 255 - longToInt4(Integer.MAX_VALUE)


def _long_to_int4(i):
    bits = int(i).bit_length()
    if bits < 4:
        return int(i)
    shift = bits - 4
    return ((int(i) >> shift) & 0x07) | ((shift + 1) << 3)


def _int4_to_long(c):
    bits, shift = c & 0x07, (c >> 3) - 1
    return bits if shift == -1 else (bits | 0x08) << shift


def int_to_byte4(n):
    """Lucene's ``SmallFloat.intToByte4``: a non-negative length as one byte (0 ... 255)."""
    n = int(n)
    if n < 0:
        raise ValueError("lengths are non-negative")
    return n if n < _NUM_FREE_VALUES else _NUM_FREE_VALUES + _long_to_int4(n - _NUM_FREE_VALUES)


def byte4_to_int(c):
    """Lucene's ``SmallFloat.byte4ToInt``: the length a code stands for (the smallest one that encodes to it)."""
    c = int(c)
    return c if c < _NUM_FREE_VALUES else _NUM_FREE_VALUES + _int4_to_long(c - _NUM_FREE_VALUES)


LENGTH_TABLE = np.array([byte4_to_int(c) for c in range(256)], dtype=np.int64)


def encode_lengths(lengths):
    """``int_to_byte4`` of an array of lengths -> uint8 (the code of n is the last one whose decoded length is <= n)."""
    return (np.searchsorted(LENGTH_TABLE, np.asarray(lengths, dtype=np.int64), side="right") - 1).astype(np.uint8)


def norm_cache(k1, b, avgdl):
    """cache[256] fp32 = k1 * ((1 - b) + b * length / avgdl), every operation in float as in BM25Similarity."""
    k1, b, avgdl = np.float32(k1), np.float32(b), np.float32(avgdl)
    return (k1 * ((np.float32(1) - b) + b * LENGTH_TABLE.astype(np.float32) / avgdl)).astype(np.float32)


def idf_weights(doc_count, doc_freq):
    """idf[t] fp32 = float(ln(1 + (docCount - docFreq + 0.5) / (docFreq + 0.5))), in double before the rounding."""
    df = np.asarray(doc_freq, dtype=np.float64)
    return np.log(1.0 + (float(doc_count) - df + 0.5) / (df + 0.5)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- CSR
def build_csr(docs, vocabulary_size):
    """docs: sequence of integer arrays (term ids in [0, V)) -> (ptr int64 [V + 1], doc int32 [nnz], tf int32 [nnz],
    lengths int64 [N]).  numpy only: (term, document) pairs are counted a block of documents at a time (``np.unique``), then one
    stable sort by term lines the blocks up -- documents stay ascending inside a term because blocks arrive in document order."""
    V, N = int(vocabulary_size), len(docs)
    if N >= 1 << 31:
        raise ValueError("document ids are int32")
    lengths = np.zeros(N, dtype=np.int64)
    terms, ids, tfs = [], [], []
    for s in range(0, N, _BUILD_DOCS):
        block = [np.asarray(d, dtype=np.int64).ravel() for d in docs[s:s + _BUILD_DOCS]]
        lens = np.array([len(d) for d in block], dtype=np.int64)
        lengths[s:s + len(block)] = lens
        if not lens.sum():
            continue
        t = np.concatenate(block)
        if t.min() < 0 or t.max() >= V:
            raise ValueError(f"term ids must lie in [0, {V})")
        d = np.repeat(np.arange(len(block), dtype=np.int64), lens)
        key, count = np.unique(t * len(block) + d, return_counts=True)
        terms.append(key // len(block))
        ids.append((key % len(block) + s).astype(np.int32))
        tfs.append(count.astype(np.int32))
    if not terms:
        return np.zeros(V + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), lengths
    term = np.concatenate(terms)
    order = np.argsort(term, kind="stable")
    ptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(term, minlength=V), out=ptr[1:])
    return ptr, np.concatenate(ids)[order], np.concatenate(tfs)[order], lengths


def parse_es_index_config(es_index_config):
    """(k1, b) of a shipped ``es_index_config`` (experiments/ir/viquae/bm25/config.json): the similarity the ``text`` mapping names,
    looked up under ``settings.similarity``; Elasticsearch's defaults for what is absent.  Analyzers other than ``standard`` (the
    default) are refused."""
    k1, b = DEFAULT_K1, DEFAULT_B
    if not es_index_config:
        return k1, b
    text = es_index_config.get("mappings", {}).get("properties", {}).get("text", {})
    analyzer = text.get("analyzer", "standard")
    if analyzer != "standard":
        raise NotImplementedError(f"analyzer '{analyzer}': only the 'standard' analyzer is restated (viquae_amd/ir/bm25.py)")
    name = text.get("similarity")
    if name is not None and name != "BM25":
        similarity = es_index_config.get("settings", {}).get("similarity", {}).get(name)
        if similarity is None:
            raise ValueError(f"es_index_config: the text mapping names similarity '{name}', which settings.similarity lacks")
        if similarity.get("type", "BM25") != "BM25":
            raise NotImplementedError(f"similarity type '{similarity.get('type')}': only BM25 is provided")
        k1, b = similarity.get("k1", k1), similarity.get("b", b)
    return float(k1), float(b)


# ---------------------------------------------------------------------------------------------------------------- the index
class MI355XBM25Index(BaseIndex):
    """Exhaustive BM25 over an inverted index held in HBM.  ``search_batch`` takes the query STRINGS (or, for an index built with
    ``add_token_ids``, integer sequences) and returns ``(float32 [nq, k], int64 [nq, k])``, best first; a passage that shares no
    term with the query is no hit, and slots beyond a query's hits are ``(-inf, -1)``.  ``tie_order`` as for MI355XFlatIndex."""

    def __init__(self, device: Optional[Union[int, list]] = None, k1: float = DEFAULT_K1, b: float = DEFAULT_B,
                 tie_order: Optional[str] = None, workspace_bytes: Optional[int] = None):
        tie_order = tie_order or os.environ.get("MQ_KNN_TIE_ORDER", "id_asc")
        if tie_order not in TIE_ORDERS:
            raise ValueError(f"tie_order must be one of {TIE_ORDERS}, got {tie_order!r}")
        self.device, self.tie_order = device, tie_order
        self.k1, self.b = float(k1), float(b)
        self.workspace_bytes = int(workspace_bytes or os.environ.get("MQ_BM25_WORKSPACE_BYTES", DEFAULT_WORKSPACE_BYTES))
        self.ntotal = 0
        self.vocabulary = None       # sorted list of terms (None: a token-id index)
        self._term_id = None
        self.ptr = self.doc = self.tf = self.codes = None          # host arrays (numpy)
        self.doc_freq = self.idf = None
        self.doc_count = self.sum_total_term_freq = 0
        self.avgdl = np.float32(1)
        self._dev = None             # device tensors: ptr, doc, tf, codes, impact
        self._torch_device = None
        self._ws = None

    def __reduce__(self):
        raise TypeError(f"{type(self).__name__} lives in HBM and cannot be pickled: use save() / load()")

    # ------------------------------------------------------------------ construction
    @property
    def vocabulary_size(self):
        return 0 if self.ptr is None else len(self.ptr) - 1

    def add_documents(self, documents, column: Optional[str] = None):
        """Index the strings of ``documents`` (a list, or a ``datasets.Dataset`` whose ``column`` holds them)."""
        texts = documents[column] if column is not None else documents
        tokens = [standard_tokenize(t) for t in texts]
        vocabulary = sorted(set().union(*tokens)) if tokens else []
        term_id = {t: i for i, t in enumerate(vocabulary)}
        self.add_token_ids([np.fromiter((term_id[t] for t in doc), dtype=np.int64, count=len(doc)) for doc in tokens], len(vocabulary))
        self.vocabulary, self._term_id = vocabulary, term_id

    def add_token_ids(self, docs, vocabulary_size):
        """Index pre-tokenised documents: ``docs[i]`` is the integer sequence of document i's term ids in [0, vocabulary_size)."""
        if self.ptr is not None:
            raise ValueError("the index is already built: its term ids and statistics are a function of the whole corpus")
        ptr, doc, tf, lengths = build_csr(docs, vocabulary_size)
        self._install(ptr, doc, tf, encode_lengths(lengths), int((lengths > 0).sum()), int(lengths.sum()))

    def _install(self, ptr, doc, tf, codes, doc_count, sum_total_term_freq):
        import torch
        if len(doc) and (np.any(doc < 0) or np.any(doc >= len(codes))):
            raise ValueError("posting document ids outside the corpus")
        # a term's postings strictly ascending (what the scoring kernel's range search relies on)
        if len(doc) > 1:
            rising = np.diff(doc.astype(np.int64)) > 0
            rising[ptr[1:-1][(ptr[1:-1] > 0) & (ptr[1:-1] < len(doc))] - 1] = True
            if not rising.all():
                raise ValueError("postings must be strictly ascending by document id inside a term")
        self.ptr, self.doc, self.tf, self.codes = ptr, doc, tf, codes
        self.ntotal = len(codes)
        self.doc_count, self.sum_total_term_freq = int(doc_count), int(sum_total_term_freq)
        self.avgdl = np.float32(self.sum_total_term_freq / self.doc_count) if self.doc_count else np.float32(1)
        self.doc_freq = np.diff(ptr)
        self.idf = idf_weights(self.doc_count, self.doc_freq)
        self._torch_device = _resolve_device(self.device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self._torch_device)
        self._dev = dict(ptr=up(ptr), doc=up(doc), tf=up(tf), codes=up(codes),
                         impact=torch.empty(len(doc), dtype=torch.float32, device=self._torch_device))
        self.set_bm25(self.k1, self.b)

    def set_bm25(self, k1, b):
        """Re-weight the resident index (pyserini's ``searcher.set_bm25``): a new 256-entry cache, one pass of the impact kernel."""
        import torch
        self.k1, self.b = float(k1), float(b)
        if self._dev is None:
            return
        cache = torch.from_numpy(norm_cache(self.k1, self.b, self.avgdl)).to(self._torch_device)
        d = self._dev
        with torch.cuda.device(self._torch_device):
            stream = torch.cuda.current_stream(self._torch_device)
            _lib.check(_lib.load().mq_bm25_impacts_f32(d["doc"].data_ptr(), d["tf"].data_ptr(), d["codes"].data_ptr(), cache.data_ptr(),
                                                       d["doc"].numel(), d["impact"].data_ptr(), stream.cuda_stream), "mq_bm25_impacts_f32")
            stream.synchronize()

    def impacts(self):
        """The device's impact array as numpy (tests, inspection)."""
        return self._dev["impact"].cpu().numpy()

    # ------------------------------------------------------------------ search
    def clauses(self, query):
        """(term ids int32, weights fp32) of one query: its distinct in-vocabulary terms in order of first occurrence, weight =
        float(multiplicity) * idf.  ``query`` is a string, or an integer sequence for a token-id index."""
        if isinstance(query, str):
            if self._term_id is None:
                raise ValueError("this index was built from token ids: query it with integer sequences")
            ids = [self._term_id[t] for t in standard_tokenize(query) if t in self._term_id]
        else:
            V = self.vocabulary_size
            ids = [int(t) for t in np.asarray(query, dtype=np.int64).ravel() if 0 <= t < V]
        counts = {}
        for t in ids:
            if self.doc_freq[t] > 0:
                counts[t] = counts.get(t, 0) + 1
        terms = np.fromiter(counts.keys(), dtype=np.int32, count=len(counts))
        mult = np.fromiter(counts.values(), dtype=np.float32, count=len(counts))
        return terms, mult * self.idf[terms]

    def search_batch(self, queries, k: int = 10, **kwargs) -> BatchedSearchResults:
        import torch
        if isinstance(queries, (str, bytes)) or not hasattr(queries, "__len__"):
            raise ValueError("queries must be a list of strings (or of term-id sequences)")
        if isinstance(queries, np.ndarray) and queries.dtype.kind in "fc":
            raise ValueError("a BM25 index is searched with strings, not with vectors")
        if self.ptr is None or self.ntotal == 0:
            raise ValueError("the index is empty: call add_documents first")
        if k < 1:
            raise ValueError("k must be >= 1")
        if k > MAX_K:
            raise NotImplementedError(f"k={k} > {MAX_K} (MQ_KNN_MAX_K)")
        nq = len(queries)
        if nq == 0:
            return BatchedSearchResults(np.zeros((0, k), np.float32), np.zeros((0, k), dtype=int))
        qptr, cterm, cweight = self.pack_clauses(queries)
        dev = self._torch_device
        up = lambda a: torch.from_numpy(a).to(dev)
        D, I = self.search_device(up(qptr), up(cterm), up(cweight), k)
        torch.cuda.current_stream(dev).synchronize()
        return BatchedSearchResults(D.cpu().numpy(), I.cpu().numpy().astype(int))

    def pack_clauses(self, queries):
        """The clauses of a batch as the C ABI takes them: qptr int32 [nq + 1] into cterm int32 / cweight fp32 (numpy)."""
        parts = [self.clauses(q) for q in queries]
        qptr = np.zeros(len(parts) + 1, dtype=np.int32)
        np.cumsum([len(t) for t, _ in parts], out=qptr[1:])
        cterm = np.concatenate([t for t, _ in parts]).astype(np.int32) if parts else np.zeros(0, np.int32)
        cweight = np.concatenate([w for _, w in parts]).astype(np.float32) if parts else np.zeros(0, np.float32)
        return qptr, cterm, cweight

    def search_device(self, qptr, cterm, cweight, k):
        """The raw hot path: clause arrays already on the device -> (D [nq, k] fp32, I [nq, k] int64) device tensors, enqueued on
        the current stream and not synchronised."""
        import torch
        lib, dev, d = _lib.load(), self._torch_device, self._dev
        nq = qptr.numel() - 1
        D = torch.empty((nq, k), dtype=torch.float32, device=dev)
        I = torch.empty((nq, k), dtype=torch.int64, device=dev)
        nbytes = int(lib.mq_bm25_workspace_bytes(self.ntotal, nq, k, self.workspace_bytes))
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        flags = FLAG_TIE_ID_DESC if self.tie_order == "id_desc" else 0
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            _lib.check(lib.mq_bm25_search_f32(d["ptr"].data_ptr(), d["doc"].data_ptr() or None, d["impact"].data_ptr() or None,
                                              self.ntotal, self.vocabulary_size, qptr.data_ptr(), cterm.data_ptr() or None,
                                              cweight.data_ptr() or None, nq, k, flags, 0, D.data_ptr(), I.data_ptr(),
                                              self._ws.data_ptr(), self._ws.numel(), self.workspace_bytes, stream.cuda_stream),
                       "mq_bm25_search_f32")
        return D, I

    # ------------------------------------------------------------------ parameter grid
    def search_grid(self, queries, params, k: int = 10, method: Optional[str] = None):
        """The queries under every ``(k1, b)`` of ``params`` at once: ``(D float32 [G, nq, k], I int64 [G, nq, k])`` as numpy arrays,
        best first, unfilled slots ``(-inf, -1)``; slice g is, bit for bit, what ``set_bm25(*params[g])`` followed by
        ``search_batch(queries, k)`` returns.  The index's own ``k1`` / ``b`` and its resident impacts are what they were afterwards.
        ``method``: "grid" -- one sweep of the postings per tile of settings (``search_grid_device``) -- or "loop" -- per setting,
        ``set_bm25`` + ``search_device``, the parameters restored at the end; None takes ``GRID_METHOD``.  Settings follow Lucene's
        own rule: ``k1`` finite and >= 0, ``0 <= b <= 1``."""
        import torch
        method = method or GRID_METHOD
        if method not in ("grid", "loop"):
            raise ValueError(f"method must be 'grid' or 'loop', got {method!r}")
        params = [(float(k1), float(b)) for k1, b in params]
        if not params:
            raise ValueError("params is empty: give at least one (k1, b)")
        for k1, b in params:
            if not (np.isfinite(k1) and k1 >= 0):
                raise ValueError(f"illegal k1 value: {k1}, must be a non-negative finite value")
            if not 0 <= b <= 1:  # (NaN fails both comparisons)
                raise ValueError(f"illegal b value: {b}, must be between 0 and 1")
        if isinstance(queries, (str, bytes)) or not hasattr(queries, "__len__"):
            raise ValueError("queries must be a list of strings (or of term-id sequences)")
        if self.ptr is None or self.ntotal == 0:
            raise ValueError("the index is empty: call add_documents first")
        if k < 1:
            raise ValueError("k must be >= 1")
        if k > MAX_K:
            raise NotImplementedError(f"k={k} > {MAX_K} (MQ_KNN_MAX_K)")
        G, nq = len(params), len(queries)
        if nq == 0:
            return np.zeros((G, 0, k), np.float32), np.zeros((G, 0, k), np.int64)
        qptr, cterm, cweight = self.pack_clauses(queries)
        dev = self._torch_device
        qptr, cterm, cweight = (torch.from_numpy(a).to(dev) for a in (qptr, cterm, cweight))
        if method == "grid":
            caches = torch.from_numpy(np.stack([norm_cache(k1, b, self.avgdl) for k1, b in params])).to(dev)
            D, I = self.search_grid_device(qptr, cterm, cweight, caches, k)
        else:
            D = torch.empty((G, nq, k), dtype=torch.float32, device=dev)
            I = torch.empty((G, nq, k), dtype=torch.int64, device=dev)
            own = (self.k1, self.b)
            try:
                for g, (k1, b) in enumerate(params):
                    self.set_bm25(k1, b)
                    D[g], I[g] = self.search_device(qptr, cterm, cweight, k)
            finally:
                self.set_bm25(*own)
        torch.cuda.current_stream(dev).synchronize()
        return D.cpu().numpy(), I.cpu().numpy()

    def search_grid_device(self, qptr, cterm, cweight, caches, k):
        """The raw grid entry: clause arrays and the settings' norm caches (fp32 [G, 256], ``norm_cache`` rows) on the device ->
        (D [G, nq, k] fp32, I [G, nq, k] int64) device tensors, enqueued on the current stream and not synchronised.  Reads the
        postings' term frequencies and the length codes; the resident impacts are neither read nor written."""
        import torch
        lib, dev, d = _lib.load(), self._torch_device, self._dev
        if caches.dim() != 2 or caches.shape[1] != 256 or caches.shape[0] < 1 or caches.dtype != torch.float32 or not caches.is_contiguous():
            raise ValueError("caches must be a contiguous float32 [G, 256] tensor, G >= 1")
        G, nq = caches.shape[0], qptr.numel() - 1
        D = torch.empty((G, nq, k), dtype=torch.float32, device=dev)
        I = torch.empty((G, nq, k), dtype=torch.int64, device=dev)
        tile = min(G, int(lib.mq_bm25_grid_tile()))
        nbytes = int(lib.mq_bm25_grid_workspace_bytes(self.ntotal, nq, tile, k, self.workspace_bytes))
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        flags = FLAG_TIE_ID_DESC if self.tie_order == "id_desc" else 0
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            _lib.check(lib.mq_bm25_search_grid_f32(d["ptr"].data_ptr(), d["doc"].data_ptr() or None, d["tf"].data_ptr() or None,
                                                   d["codes"].data_ptr(), caches.data_ptr(), G, self.ntotal, self.vocabulary_size,
                                                   qptr.data_ptr(), cterm.data_ptr() or None, cweight.data_ptr() or None, nq, k, flags, 0,
                                                   D.data_ptr(), I.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                                   self.workspace_bytes, stream.cuda_stream), "mq_bm25_search_grid_f32")
        return D, I

    def grid_query_chunk(self, nq, g):
        """Queries scored per launch for a tile of ``g`` settings under this index's workspace budget."""
        return int(_lib.load().mq_bm25_grid_chunk_queries(self.ntotal, int(nq), int(g), self.workspace_bytes))

    def query_chunk(self, nq):
        """Queries scored per launch under this index's workspace budget."""
        return int(_lib.load().mq_bm25_chunk_queries(self.ntotal, int(nq), self.workspace_bytes))

    def search(self, query, k: int = 10, **kwargs) -> SearchResults:
        scores, indices = self.search_batch([query], k)
        return SearchResults(scores[0], indices[0].astype(int))

    # ------------------------------------------------------------------ persistence
    def save(self, file: Union[str, PurePath], storage_options: Optional[dict] = None):
        """Own format "MQBM2501": header (N, V, nnz, docCount, sumTotalTermFreq int64; k1, b float64; vocabulary bytes int64, -1
        for a token-id index), then ptr, doc, tf, length codes, then the vocabulary as UTF-8 terms joined by newlines."""
        if self.ptr is None:
            raise ValueError("the index is empty: nothing to save")
        vocab = b"" if self.vocabulary is None else "\n".join(self.vocabulary).encode("utf-8")
        with open(os.fspath(file), "wb") as f:
            f.write(_MAGIC + struct.pack("<qqqqqddq", self.ntotal, self.vocabulary_size, len(self.doc), self.doc_count,
                                         self.sum_total_term_freq, self.k1, self.b, -1 if self.vocabulary is None else len(vocab)))
            for a, t in ((self.ptr, np.int64), (self.doc, np.int32), (self.tf, np.int32), (self.codes, np.uint8)):
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())
            f.write(vocab)

    @classmethod
    def load(cls, file: Union[str, PurePath], device=None, storage_options: Optional[dict] = None, tie_order=None, k1=None, b=None):
        """Reads a file written by :meth:`save`; ``k1`` / ``b`` override the stored parameters (the impacts are recomputed anyway)."""
        with open(os.fspath(file), "rb") as f:
            if f.read(8) != _MAGIC:
                raise ValueError(f"{file} is not an MI355XBM25Index file")
            N, V, nnz, doc_count, sttf, k1_file, b_file, vbytes = struct.unpack("<qqqqqddq", f.read(64))
            read = lambda n, t: np.frombuffer(f.read(n * np.dtype(t).itemsize), dtype=t).copy()
            ptr, doc, tf, codes = read(V + 1, np.int64), read(nnz, np.int32), read(nnz, np.int32), read(N, np.uint8)
            vocabulary = None if vbytes < 0 else (f.read(vbytes).decode("utf-8").split("\n") if V else [])
        if len(ptr) != V + 1 or len(codes) != N or len(tf) != nnz or ptr[0] != 0 or ptr[-1] != nnz or np.any(np.diff(ptr) < 0):
            raise ValueError(f"{file}: truncated or inconsistent index file")
        index = cls(device=device, k1=k1_file if k1 is None else k1, b=b_file if b is None else b, tie_order=tie_order)
        index._install(ptr, doc, tf, codes, doc_count, sttf)
        if vocabulary is not None:
            if len(vocabulary) != V:
                raise ValueError(f"{file}: vocabulary of {len(vocabulary)} terms, expected {V}")
            index.vocabulary, index._term_id = vocabulary, {t: i for i, t in enumerate(vocabulary)}
        return index
