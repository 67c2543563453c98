"""Late fusion on the MI355X (mq_fuse_wsum_f64) against the oracle restatement and the reference-minted
golden vectors.  Tolerance: the fused scores are f64; the per-run moments are summed in a different order than
numpy's pairwise summation, so scores agree to 1e-12 relative (not bit-exact) under 'gzmuv' / 'zmuv', and
bit-exactly with norm=None.  Ranks are compared wherever neighbouring fused scores differ by more than that."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import fuse as ofuse
from viquae_amd.ir import fuse as hfuse

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "fuse.json")
RTOL = 1e-12


def cases():
    with open(GOLDEN) as file:
        return json.load(file)["cases"]


def assert_same_run(got, want, exact=False):
    assert list(got) == list(want)
    for q in want:
        g, w = got[q], want[q]
        assert g.keys() == w.keys(), q
        gs, ws = np.array([g[d] for d in w]), np.array(list(w.values()))
        if exact:
            assert np.array_equal(gs, ws), q
            assert list(g) == list(w), q
            continue
        scale = max(1.0, float(np.abs(ws).max())) if len(ws) else 1.0
        assert np.all(np.abs(gs - ws) <= RTOL * scale), (q, np.abs(gs - ws).max())
        g_scores = list(g.values())
        assert all(a >= b for a, b in zip(g_scores, g_scores[1:])), q
        # same order wherever the oracle's neighbouring scores are separated by more than the tolerance
        docs_w, docs_g = list(w), list(g)
        for i, d in enumerate(docs_w):
            sep_prev = i == 0 or ws[i - 1] - ws[i] > 4 * RTOL * scale
            sep_next = i == len(ws) - 1 or ws[i] - ws[i + 1] > 4 * RTOL * scale
            if sep_prev and sep_next:
                assert docs_g[i] == d, (q, i)


@pytest.mark.parametrize("case", cases(), ids=lambda c: c["name"])
def test_golden_gzmuv_defmin(case):
    got = hfuse.fuse_runs(case["runs"], case["weights"], norm="gzmuv", defmin=True)
    assert_same_run(got, case["unpinned_wsum_gzmuv_defmin"])
    got = hfuse.fuse_runs(case["runs"], case["weights"], norm="gzmuv", defmin=False)
    assert_same_run(got, case["unpinned_wsum_gzmuv_nodefmin"])


@pytest.mark.parametrize("case", cases(), ids=lambda c: c["name"])
def test_single_run_gzmuv_is_the_reference_norm(case):
    """One run, weight 1: the fused scores ARE gzmuv_norm's output -- compared with the reference's own values."""
    defmin = case["reference_default_minimum"]
    for run, want in zip(defmin, case["reference_gzmuv_after_defmin"]):
        got = hfuse.fuse_runs([run], [1.0], norm="gzmuv", defmin=False)
        for q in want:
            assert got[q].keys() == want[q].keys()
            for d, s in want[q].items():
                assert abs(got[q][d] - s) <= RTOL * max(1.0, abs(s))


def random_runs(seed, nq, n_runs, k, n_docs, empty_every=0):
    rng = np.random.default_rng(seed)
    runs = []
    for r in range(n_runs):
        run = {}
        for q in range(nq):
            if empty_every and (q * 7 + r) % empty_every == 0:
                run[str(q)] = {}
                continue
            kk = int(rng.integers(1, k + 1))
            docs = rng.choice(n_docs, size=kk, replace=False)
            scores = np.sort(rng.standard_normal(kk).astype(np.float32) * (r + 1) + 3 * r)[::-1]
            run[str(q)] = {str(int(d)): float(s) for d, s in zip(docs, scores)}
        runs.append(run)
    return runs


@pytest.mark.parametrize("norm", [None, "gzmuv", "zmuv"])
@pytest.mark.parametrize("defmin", [False, True])
@pytest.mark.parametrize("shape", [(40, 2, 100, 300, 0), (33, 4, 100, 150, 5), (7, 3, 1, 4, 0), (5, 8, 500, 3000, 3),
                                   (3, 32, 128, 100000, 0)])
def test_against_oracle(norm, defmin, shape):
    nq, n_runs, k, n_docs, empty_every = shape
    runs = random_runs(nq * 31 + n_runs, nq, n_runs, k, n_docs, empty_every)
    weights = list(np.random.default_rng(5).uniform(0.05, 1.0, n_runs))
    want = ofuse.fusion_test(runs, weights, norm=norm, defmin=defmin)
    got = hfuse.fuse_runs(runs, weights, norm=norm, defmin=defmin)
    assert_same_run(got, want, exact=norm is None)


def test_ties_and_signed_zero():
    runs = [{"q": {"10": 1.0, "9": 1.0, "100": 1.0, "4": -0.0, "3": 0.0}}, {"q": {"9": 0.0, "11": 1.0, "2": -1.0}}]
    want = ofuse.fusion_test(runs, [1.0, 1.0], norm=None, defmin=False)
    got = hfuse.fuse_runs(runs, [1.0, 1.0], norm=None, defmin=False)
    assert list(got["q"]) == list(want["q"]) == ["9", "10", "11", "100", "3", "4", "2"]
    assert list(got["q"].values()) == list(want["q"].values())


def test_constant_run_uses_the_1e9_floor():
    runs = [{"q": {"1": 2.0, "2": 2.0}, "p": {"5": 2.0}}, {"q": {"1": 1.0, "3": 0.0}, "p": {"5": 1.0, "6": 3.0}}]
    want = ofuse.fusion_test(runs, [0.5, 0.5], norm="gzmuv", defmin=True)
    got = hfuse.fuse_runs(runs, [0.5, 0.5], norm="gzmuv", defmin=True)
    assert_same_run(got, want)


def test_large_ids_and_non_numeric_names():
    big = 2 ** 57 + 12345
    runs = [{"q": {str(big): 1.0, "7": 0.5}}, {"q": {str(big): 0.25, "8": 2.0}}]
    got = hfuse.fuse_runs(runs, [1.0, 1.0], norm=None)
    assert got == {"q": {"8": 2.0, str(big): 1.25, "7": 0.5}}
    runs = [{"q": {"doc-b": 1.0, "doc-a": 0.5}}, {"q": {"doc-a": 1.0}}]
    got = hfuse.fuse_runs(runs, [1.0, 1.0], norm=None)
    assert got == {"q": {"doc-a": 1.5, "doc-b": 1.0}}


def test_device_tables_and_errors():
    ids = torch.tensor([[[3, 1, -1]], [[1, 2, 5]]], device="cuda:0")
    scores = torch.tensor([[[1.0, 2.0, 0.0]], [[10.0, 20.0, 30.0]]], dtype=torch.float64, device="cuda:0")
    out_ids, out_scores, counts = hfuse.fuse_tables(ids, scores, [1.0, 0.1], norm=None, defmin=True)
    assert counts.tolist() == [4]
    # run 0 fills docs 2, 5 with its minimum 1.0; run 1 fills doc 3 with its minimum 10.0
    assert out_ids[0].tolist() == [5, 1, 2, 3, -1, -1]
    assert out_scores[0, :4].tolist() == [1.0 + 0.1 * 30.0, 2.0 + 0.1 * 10.0, 1.0 + 0.1 * 20.0, 1.0 + 0.1 * 10.0]
    with pytest.raises(ValueError):
        hfuse.fuse_tables(ids, scores, [1.0], norm=None)
    with pytest.raises(NotImplementedError):
        hfuse.fuse_tables(ids, scores, [1.0, 1.0], norm="min-max")
    too_wide = torch.full((2, 1, 3000), -1, device="cuda:0")
    with pytest.raises(Exception):
        hfuse.fuse_tables(too_wide, too_wide.double(), [1.0, 1.0])


def test_fusion_class_like_dataset_search(tmp_path):
    case = cases()[0]
    fuser = hfuse.Fusion(qrels=None, runs=case["runs"], norm="gzmuv", defmin=True, output=tmp_path)
    fused = fuser.test(best_params={"weights": case["weights"]})
    fused = fused if isinstance(fused, dict) else fused.to_dict()
    assert_same_run(fused, case["unpinned_wsum_gzmuv_defmin"])
    with open(tmp_path / "test_run.json") as file:
        assert_same_run(json.load(file), case["unpinned_wsum_gzmuv_defmin"])


# ---------------------------------------------------------------------------------------------------------------------
# shapes and edges of mq_fuse_wsum_f64 that the cases above do not reach (tests/fuse_cases.py holds the shared cases)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1100, 2049])
def test_more_queries_than_the_moments_kernel_has_threads(nq):
    """fuse_moments_kernel strides over the queries by its 1024 threads: two and three steps, the default-minimum fill counted in
    closed form, some (run, query) pairs empty.  A pool of 7 documents makes the unions overlap."""
    runs = random_runs(nq, nq, 2, 3, 7, empty_every=5)
    for norm in (None, "gzmuv", "zmuv"):
        for defmin in (False, True):
            want = ofuse.fusion_test(runs, [0.7, 0.3], norm=norm, defmin=defmin)
            got = hfuse.fuse_runs(runs, [0.7, 0.3], norm=norm, defmin=defmin)
            assert_same_run(got, want, exact=norm is None)


@pytest.mark.parametrize("norm", [None, "gzmuv", "zmuv"])
@pytest.mark.parametrize("defmin", [False, True])
def test_hollow_case(norm, defmin):
    """A run without any result (its gzmuv moments have no entry to average) and a query that is empty in every run."""
    from tests import fuse_cases as fc
    runs, _, _ = fc.case_data("hollow")
    weights = [0.5, 0.25, 0.25]
    want = fc.reference_fused(runs, [weights], norm, defmin)[0]
    assert want["q3"] == {} and all(not results for results in runs[1].values())
    assert_same_run(hfuse.fuse_runs(runs, weights, norm=norm, defmin=defmin), want, exact=norm is None)
    q_ids, _, ids, scores = hfuse.runs_to_tables(runs)
    out_ids, out_scores, counts = hfuse.fuse_tables(ids, scores, weights, norm=norm, defmin=defmin)
    q = q_ids.index("q3")
    assert counts[q].item() == 0
    assert (out_ids[q] == -1).all().item() and (out_scores[q] == 0.0).all().item() and out_ids.shape[1] == 3 * 20
    assert counts.tolist() == [len(want[q_id]) for q_id in q_ids]


def test_id_edge_case():
    """Ids 2^58 - 1, 2^58 - 2 and 0 in runs 0 and 31: the sort key (id << 5) | run at both ends of both fields.  Scores and weights
    are dyadic, so the fused scores below are exact and the order is stated by hand."""
    from tests import fuse_cases as fc
    runs, _, _ = fc.case_data("id_edge")
    b, b1 = str(2 ** 58 - 1), str(2 ** 58 - 2)
    weights = [1.0] * 32
    weights[7], weights[31] = 2.0, 0.5
    got = hfuse.fuse_runs(runs, weights, norm=None, defmin=False)
    assert list(got["q0"].items()) == [(b, 4.25), (b1, 3.5), ("0", 3.25), ("7", 0.25), ("5", 0.125)]
    assert list(got["q1"].items()) == [(b, 1.5), ("0", 1.0), (b1, 1.0)]                 # equal scores: ascending id
    assert_same_run(got, ofuse.fusion_test(runs, weights, norm=None, defmin=False), exact=True)
    got = hfuse.fuse_runs(runs, weights, norm=None, defmin=True)
    # q0: run 0 fills 5 and 7 with 1.0, run 7 (weight 2) fills b, b1 and 5 with 0.125, run 31 (weight 0.5) fills 7 with 0.25
    assert list(got["q0"].items()) == [(b, 4.5), (b1, 3.75), ("0", 3.25), ("5", 1.375), ("7", 1.375)]
    assert list(got["q1"].items()) == [(b1, 2.0), ("0", 1.5), (b, 1.5)]                 # run 7 is empty here: it fills nothing
    assert_same_run(got, ofuse.fusion_test(runs, weights, norm=None, defmin=True), exact=True)
    for norm in ("gzmuv", "zmuv"):
        for defmin in (False, True):
            want = fc.reference_fused(runs, [weights], norm, defmin)[0]
            assert_same_run(hfuse.fuse_runs(runs, weights, norm=norm, defmin=defmin), want)
    with pytest.raises(ValueError):
        hfuse.fuse_runs([{"q": {str(2 ** 58): 1.0}}, {"q": {"1": 1.0}}], [1.0, 1.0], norm=None)
