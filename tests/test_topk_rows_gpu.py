"""Direct GPU tests of mq_topk_rows_f32 (csrc/bm25.hip: topk_hist_kernel / topk_gather_kernel / topk_sort_kernel) on the cases of
tests/topk_rows_cases.py: every D compared as uint32 and every I exactly with the sort of the 64-bit keys (bm25_restatement.topk),
slots beyond a row's hits (-inf, -1).  D, I and the workspace each end in a guard region that must stay as it was; the workspace
is exactly mq_topk_rows_workspace_bytes and holds 0xFF bytes before every call (the call must not rely on what it finds there).
tests/test_topk_rows_cases_cpu.py checks that each case reaches the regime it is listed for.  A matrix is uploaded once and all
its k values and tie orders run on it; a row's keys are sorted once on the host and sliced per k."""
import functools

import numpy as np
import pytest

from tests import bm25_restatement as br
from tests import topk_rows_cases as tc

pytestmark = pytest.mark.gpu

GUARD = 4096          # bytes behind D, I and the workspace
PATTERN = 0xA5        # what the guards (and D / I before a call) hold: as fp32 a negative number, as int64 neither an id nor -1
MQ_EWORKSPACE = -2


def _lib():
    from viquae_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _cases():
    return {c.name: c for c in tc.cases(_lib())}


def _case_names():
    # the names do not depend on the library's constants being read at collection time: they are listed here and checked below
    return ["N1-distinct", "N1-all_equal", "N1-two_ulp1", "N1-sparse0", "N1-sparse1", "N2-distinct", "N2-all_equal", "N2-two_ulp1",
            "N2-sparse0", "N2-sparse1", "N1023-stride", "N1024-stride", "N1025-stride", "N16384-split", "N16385-split", "N70001-mixed",
            "N70001-distinct", "N70001-levels50", "N70001-all_equal", "N70001-two_ulp650", "N70001-extremes", "N70001-sparse0",
            "N70001-sparse1", "N70001-sparse299", "N70001-sparse300", "N70001-sparse301", "N70001-chunk_edges", "N70001-kpads",
            "N50001-rows700", "N17000-rows2048", "cap-first", "N2^21+100"]


class Buffers:
    """D [rows, k] fp32, I [rows, k] int64 and a workspace of exactly `ws_bytes`, each followed by GUARD bytes of PATTERN."""

    def __init__(self, rows, k, ws_bytes):
        import torch
        self.rows, self.k, self.ws_bytes = rows, k, ws_bytes
        new = lambda n: torch.full((n + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        self.d, self.i, self.ws = new(rows * k * 4), new(rows * k * 8), new(ws_bytes)

    def dirty(self):
        self.ws[:self.ws_bytes] = 0xFF

    def D(self):
        return self.d[:self.rows * self.k * 4].cpu().numpy().view(np.float32).reshape(self.rows, self.k)

    def I(self):
        return self.i[:self.rows * self.k * 8].cpu().numpy().view(np.int64).reshape(self.rows, self.k)

    def guards_untouched(self):
        return all(bool((b[-GUARD:] == PATTERN).all()) for b in (self.d, self.i, self.ws))

    def results_untouched(self):
        return bool((self.d == PATTERN).all()) and bool((self.i == PATTERN).all())


def _call(x, rows, N, k, tie, id_offset, buf, ws_bytes=None):
    import torch
    rc = _lib().mq_topk_rows_f32(x.data_ptr(), rows, N, k, 2 if tie == "id_desc" else 0, id_offset, buf.d.data_ptr(), buf.i.data_ptr(),
                                 buf.ws.data_ptr(), buf.ws_bytes if ws_bytes is None else ws_bytes,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _expected(sorted_rows, k, id_offset):
    """(D, I) [rows, k] from every row's (scores, ids) sorted best first: the first k, then (-inf, -1)."""
    D = np.full((len(sorted_rows), k), -np.inf, dtype=np.float32)
    I = np.full((len(sorted_rows), k), -1, dtype=np.int64)
    for r, (d, i) in enumerate(sorted_rows):
        n = min(k, len(d))
        D[r, :n], I[r, :n] = d[:n], i[:n] + id_offset
    return D, I


def _same(buf, want, what):
    D, I = buf.D(), buf.I()
    assert np.array_equal(I, want[1]), what
    assert np.array_equal(D.view(np.uint32), want[0].view(np.uint32)), what
    assert buf.guards_untouched(), what


def test_the_listed_names_are_the_case_list():
    assert _case_names() == list(_cases())


@pytest.mark.parametrize("name", _case_names())
def test_case_equals_the_sorted_keys(name):
    import torch
    lib, case = _lib(), _cases()[name]
    rows, N = len(case.rows), case.N
    X = tc.matrix(case, tc.split_of(lib, rows, N))
    x = torch.from_numpy(X).cuda()
    for tie in case.tie_orders:
        sorted_rows = [br.topk(X[r], max(case.ks), tie) for r in range(rows)]
        for k in case.ks:
            buf = Buffers(rows, k, int(lib.mq_topk_rows_workspace_bytes(rows, k)))
            buf.dirty()
            assert _call(x, rows, N, k, tie, case.id_offset, buf) == 0
            _same(buf, _expected(sorted_rows, k, case.id_offset), (name, tie, k))


def test_results_do_not_depend_on_what_the_workspace_held():
    """Two launches of different (rows, k) back to back on ONE workspace, the big k first: the second one finds the first one's
    histograms, counters and candidates where its own will lie, and gives what a launch on a fresh workspace gives."""
    import torch
    lib = _lib()
    big, small = _cases()["N70001-mixed"], _cases()["N70001-kpads"]
    assert len(big.rows) > len(small.rows)
    Xb, Xs = (tc.matrix(c, tc.split_of(lib, len(c.rows), c.N)) for c in (big, small))
    xb, xs = torch.from_numpy(Xb).cuda(), torch.from_numpy(Xs).cuda()
    kb, ks = 2048, 5
    nbytes = int(lib.mq_topk_rows_workspace_bytes(len(big.rows), kb))
    assert nbytes >= int(lib.mq_topk_rows_workspace_bytes(len(small.rows), ks))
    for tie in tc.TIE_ORDERS:
        first = Buffers(len(big.rows), kb, nbytes)
        first.dirty()
        assert _call(xb, len(big.rows), big.N, kb, tie, 0, first) == 0
        _same(first, _expected([br.topk(r, kb, tie) for r in Xb], kb, 0), ("big", tie))
        second = Buffers(len(small.rows), ks, nbytes)
        second.ws = first.ws                               # the workspace as the first launch left it
        assert _call(xs, len(small.rows), small.N, ks, tie, 0, second) == 0
        _same(second, _expected([br.topk(r, ks, tie) for r in Xs], ks, 0), ("small after big", tie))
        # and the first problem again on what the second one left
        again = Buffers(len(big.rows), kb, nbytes)
        again.ws = first.ws
        assert _call(xb, len(big.rows), big.N, kb, tie, 0, again) == 0
        assert np.array_equal(again.D().view(np.uint32), first.D().view(np.uint32)) and np.array_equal(again.I(), first.I())
        assert again.guards_untouched()


def test_one_byte_too_few_is_refused_and_nothing_is_written():
    import torch
    lib = _lib()
    x = torch.ones((3, 1000), dtype=torch.float32, device="cuda")
    for k in (1, 300, 2048):
        nbytes = int(lib.mq_topk_rows_workspace_bytes(3, k))
        buf = Buffers(3, k, nbytes)
        assert _call(x, 3, 1000, k, "id_asc", 0, buf, ws_bytes=nbytes - 1) == MQ_EWORKSPACE
        assert buf.results_untouched() and bool((buf.ws == PATTERN).all())
        assert _call(x, 3, 1000, k, "id_asc", 0, buf) == 0
        assert buf.I()[:, :min(k, 1000)].tolist() == [list(range(min(k, 1000)))] * 3 and buf.guards_untouched()
