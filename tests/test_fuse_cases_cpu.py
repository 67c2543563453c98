"""What the device tests of the fusion kernels take for granted about their cases (tests/fuse_cases.py), checked on the reference
alone: every case reaches the regime it is listed for, neighbouring fused scores are far enough apart for exact rank comparison
under the two norms, and the data can tell a wrong tie rule, a dropped default-minimum or a wrong cut from the right one.  No test
here touches a GPU.  Every test prints the figures it asserts (pytest -s shows them)."""
import numpy as np
import pytest

from tests import fuse_cases as fc

NAMES = list(fc.CASES)


def test_case_list_is_the_table():
    assert NAMES == ["floor", "two_pass", "dense_qrels", "cap", "many_runs", "single", "hollow", "ties", "id_edge"]
    for case in fc.cases():
        assert case.purpose
        runs, qrels, trials = fc.case_data(case.name)
        reg = fc.regime(case.name)
        assert (reg["n_runs"], reg["K"], reg["nq"]) == (case.n_runs, case.K, case.nq), case.name
        assert all(run.keys() == runs[0].keys() for run in runs)
        assert case.n_runs <= fc.MAX_RUNS and case.n_runs * case.K <= fc.FCAP
        assert 1 <= len(trials) <= 12 and all(len(w) == case.n_runs for w in trials)
    assert set(fc.CASES["floor"].metrics) == set(fc.CASES["ties"].metrics) == set(fc.ALL_METRICS)
    used = {m for case in fc.cases() if case.name not in ("floor", "ties") for m in case.metrics}
    assert used == set(fc.ALL_METRICS)                       # the rotating pairs cover every metric code and cut as well
    assert all(len(case.metrics) == 2 for case in fc.cases() if case.name not in ("floor", "ties"))


def test_trial_lists_hold_what_they_are_listed_for():
    for case in fc.cases():
        trials = fc.case_data(case.name)[2]
        n = case.n_runs
        assert trials[0] == [1.0] + [0.0] * (n - 1)
        if n == 1:
            assert trials[0] == [1.0]
            continue
        assert trials[1] == [0.0] * (n - 1) + [1.0] and trials[2] == [1.0 / n] * n
        if n >= 3:
            assert any(sum(1 for x in w if x == 0.0) >= 2 for w in trials[2:])     # several zero weights, not a unit vector of an end
        assert sum(1 for w in trials[3:] if all(abs(x * 10 - round(x * 10)) < 1e-9 for x in w)) >= 4
        assert all(all(0.0 <= x <= 1.0 for x in w) for w in trials)


def test_qrels_hold_every_kind_of_query():
    for name in ("floor", "two_pass", "many_runs", "hollow", "ties"):
        runs, qrels, _ = fc.case_data(name)
        q_ids = list(runs[0])
        assert any(q not in qrels for q in q_ids), name                                             # no judgements
        grades = {r for judged in qrels.values() for r in judged.values()}
        assert grades == {0, 1, 2}, (name, grades)
        assert any(r >= 1 and d not in fc.union_of(runs, q) for q, judged in qrels.items() for d, r in judged.items()), name
    runs, qrels, _ = fc.case_data("floor")
    ragged = sum(1 for run in runs for res in run.values() if len(res) < 100)
    assert 0 < ragged < 0.25 * 2 * 48


EXPECT = {  # nsort, dynamic LDS of the fit kernel, and bounds on the largest union / relevant count
    "floor": dict(nsort=256, lds=8 << 10, union=(101, 200), relevant=(1, 256)),
    "two_pass": dict(nsort=512, lds=16 << 10, union=(257, 400), relevant=(1, 256)),
    "dense_qrels": dict(nsort=512, lds=16 << 10, union=(257, 400), relevant=(257, 400)),
    "cap": dict(nsort=4096, lds=128 << 10, union=(3000, 4096), relevant=(1, 4096)),
    "many_runs": dict(nsort=512, lds=16 << 10, union=(41, 200), relevant=(1, 256)),
    "single": dict(nsort=256, lds=8 << 10, union=(1, 1), relevant=(1, 1)),
    "hollow": dict(nsort=256, lds=8 << 10, union=(21, 40), relevant=(1, 40)),
    "ties": dict(nsort=256, lds=8 << 10, union=(51, 80), relevant=(1, 80)),
    "id_edge": dict(nsort=256, lds=8 << 10, union=(5, 5), relevant=(2, 2)),
}


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_regime(name):
    reg = fc.regime(name)
    print(f"\n{name}: {reg}")
    want = EXPECT[name]
    case = fc.CASES[name]
    assert reg["nsort"] == want["nsort"] and reg["lds"] == want["lds"]
    # mq_fuse_wsum_f64 sorts the same entries without the raise to FT: the floor of 64 (single, hollow), 128 for id_edge's 32 x 4
    assert fc.nsort_of(case.n_runs, case.K, fit=False) == {"single": 64, "hollow": 64, "id_edge": 128}.get(name, want["nsort"])
    assert want["union"][0] <= reg["max_union"] <= want["union"][1], reg
    assert want["relevant"][0] <= reg["max_relevant"] <= want["relevant"][1], reg
    runs, qrels, trials = fc.case_data(name)
    if name == "floor":
        assert case.n_runs * case.K <= fc.FT                      # one compaction pass
    if name == "cap":
        assert case.n_runs * case.K == fc.FCAP and case.n_runs == fc.MAX_RUNS and all(len(w) == 32 for w in trials)
    if name == "many_runs":
        assert case.n_runs * case.K == 280 and reg["nsort"] - 280 == 232
        empty_in = [r for r, run in enumerate(runs) if not run["q2"]]
        assert 0 < len(empty_in) < case.n_runs
    if name == "single":
        assert trials[0] == [1.0] and fc.nsort_of(1, 1, fit=False) == 64
        assert "mrr@1" in case.metrics and reg["max_union"] == 1   # a cut EQUAL to the union size
    if name == "hollow":
        assert reg["min_union"] == 0 and "q3" in qrels             # nh = 0, with judgements
        assert any(all(not res for res in run.values()) for run in runs)
        assert any(q not in qrels for q in runs[0])
        assert all(d not in fc.union_of(runs, "q6") for d in qrels["q6"]) and any(r >= 1 for r in qrels["q6"].values())
        assert fc.union_of(runs, "q6")
    if name == "id_edge":
        ids = {int(d) for run in runs for res in run.values() for d in res}
        assert {0, fc.ID_LIMIT - 1, fc.ID_LIMIT - 2} <= ids and max(ids) < fc.ID_LIMIT
        for r in (0, 31):
            assert {"0", str(fc.BIG), str(fc.BIG - 1)} <= runs[r]["q0"].keys()
        assert ((fc.ID_LIMIT - 1) << 5 | 31) == 2 ** 63 - 1        # the largest sort key, below the EMPTY marker
    if name in ("many_runs", "hollow", "ties", "id_edge"):
        below = [m for m in case.metrics if "@" in m and int(m.split("@")[1]) < reg["max_union"]]
        assert below, name                                         # a cut below the union size
    if name == "cap":
        assert reg["max_union"] > 1000 or "precision@1000" not in case.metrics
    if name == "floor":
        assert reg["max_union"] < 1000                             # precision@1000: a cut above the union size


@pytest.mark.parametrize("name", NAMES)
def test_neighbouring_fused_scores_are_separated(name):
    """Under gzmuv / zmuv the device's moments differ from numpy's by ~1e-15 relative; ranks (and so the metric values) can only be
    compared exactly when no two distinct neighbouring scores of the reference are closer than assert_same_run's 4 * RTOL * scale."""
    for norm in ("gzmuv", "zmuv"):
        for defmin in fc.DEFMINS:
            gap = fc.smallest_gap(fc.case_fused(name, norm, defmin))
            print(f"\n{name} norm={norm} defmin={defmin}: smallest relative gap {gap:.3g}")
            assert gap > 4 * fc.RTOL, (name, norm, defmin, gap)


def test_reference_fit_shapes_and_means():
    runs, qrels, trials = fc.case_data("hollow")
    fit = fc.reference_fit(runs, qrels, trials, "gzmuv", True, "precision")
    assert fit.per_q.shape == (len(trials), 10) and fit.mean.shape == (len(trials),)
    assert np.array_equal(fit.mean, np.mean(fit.per_q, axis=1))
    assert np.array_equal(fit.per_q, fc.case_fit("hollow", "gzmuv", True, "precision").per_q)
    assert (fit.per_q[:, 3] == 0).all() and (fit.per_q[:, 6] == 0).all()       # the empty union; only unreachable relevants
    for fused in fit.fused:
        assert fused["q3"] == {} and list(fused) == list(runs[0])


def test_ties_case_depends_on_the_tie_rule():
    """norm=None: recomputed with equal scores by DESCENDING id, some query's metric changes for some trial -- for every metric
    family, so a kernel with the wrong tie rule cannot pass."""
    _, qrels, _ = fc.case_data("ties")
    for defmin in fc.DEFMINS:
        fused = fc.case_fused("ties", None, defmin)
        assert any(len(set(res.values())) < len(res) for f in fused for res in f.values())
        other = [fc.descending_id_ties(f) for f in fused]
        changed = {m: int((fc.per_query(fused, qrels, m) != fc.per_query(other, qrels, m)).sum()) for m in fc.ALL_METRICS}
        print(f"\nties defmin={defmin}: (trial, query) cells the opposite tie rule changes: {changed}")
        for m in ("mrr@100", "mrr@1", "precision@5", "hit_rate@3", "recall@10"):
            assert changed[m] > 0, (m, defmin)


@pytest.mark.parametrize("name,norm,metric", [("floor", "gzmuv", "mrr@100"), ("many_runs", "gzmuv", "precision@5"),
                                              ("two_pass", None, "recall@10")])
def test_default_minimum_shows_in_the_metric(name, norm, metric):
    a, b = fc.case_fit(name, norm, True, metric).per_q, fc.case_fit(name, norm, False, metric).per_q
    print(f"\n{name} {norm} {metric}: cells defmin changes: {int((a != b).sum())} of {a.size}")
    assert (a != b).any()


def test_floor_tells_the_cuts_apart():
    for norm in fc.NORMS:
        for defmin in fc.DEFMINS:
            m1, m100, mall = [fc.case_fit("floor", norm, defmin, m).per_q for m in ("mrr@1", "mrr@100", "mrr")]
            assert (m1 != m100).any() and (m100 != mall).any() and (m1 != mall).any(), (norm, defmin)


def test_runs_to_tables_refuses_ids_the_sort_key_cannot_hold():
    torch = pytest.importorskip("torch")
    from viquae_amd.ir import fuse as hfuse
    ok = [{"q": {str(2 ** 58 - 1): 1.0, "0": 0.5}}, {"q": {"7": 1.0}}]
    q_ids, names, ids, scores = hfuse.runs_to_tables(ok, device="cpu")
    assert names is None and ids[0, 0].tolist() == [2 ** 58 - 1, 0] and ids.dtype == torch.int64
    for bad in (2 ** 58, 2 ** 58 + 1, 2 ** 63 - 1, 2 ** 63, 10 ** 30):
        with pytest.raises(ValueError):
            hfuse.runs_to_tables([{"q": {"1": 1.0}}, {"q": {str(bad): 1.0}}], device="cpu")
    runs, _, _ = fc.case_data("id_edge")
    _, names, ids, _ = hfuse.runs_to_tables(runs, device="cpu")
    assert names is None and tuple(ids.shape) == (32, 2, 4) and int(ids.max()) == 2 ** 58 - 1
