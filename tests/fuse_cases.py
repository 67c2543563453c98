"""Cases, seeded generators and the reference side of the direct tests of the fusion kernels (csrc/fuse.hip): numpy only, imports
without torch and without a GPU.  tests/test_fuse_fit_gpu.py and tests/test_fuse_gpu.py run the cases on the device,
tests/test_fuse_cases_cpu.py checks on the reference alone that every case reaches the regime it is listed for.

What the kernels' code makes a regime (restated here because no getter reports it):
  nsort      entries one query workgroup sorts: n_runs * K rounded up to a power of two, at least 64 -- and at least FT = 256 in
             mq_fuse_fit_wsum_f64, whose head compaction walks nsort in steps of FT.  Refused above FCAP = 4096.
  union      distinct documents of one query over all runs ("heads"): above FT the per-head loops of fuse_fit_kernel take a
             second step
  relevant   union documents judged >= 1: above FT the rank count of fuse_fit_kernel takes a second step
  LDS        fuse_fit_kernel asks for 32 * nsort bytes of dynamic LDS: 8 KB at the floor, 128 KB at nsort = 4096

Runs are ``{q: {doc: score}}`` with decimal document ids, float32-valued scores (normals scaled by r + 1 and shifted by 3 r in run
r, as random_runs of tests/test_fuse_gpu.py; the "levels" variant draws from four dyadic levels instead, so that fused scores tie
EXACTLY under norm=None).  Most queries hold K results, the ragged ones ((5 q + r) % 7 == 3) fewer.  Qrels judge a share of each
query's union with 0 / 1 / 2, leave every fifth query without judgements, give every third a single relevant document and add
relevant documents that no run holds.  A case's trial list stands in for ranx's grid: the unit vectors of the first and last run,
the uniform vector, vectors with several zero weights and a few random multiples of 0.1.

The reference (`reference_fit`) is composed of oracle.fuse.default_minimum, NORMS, wsum and rank_metric only."""
import collections
import functools
import warnings

import numpy as np

from oracle import fuse as ofuse

RTOL = 1e-12            # assert_same_run's constant (tests/test_fuse_gpu.py); neighbours must be 4 * RTOL * scale apart
FT = 256                # threads of a query workgroup
FCAP = 4096             # n_runs * K limit
MAX_RUNS = 32           # MQ_FUSE_MAX_RUNS
ID_LIMIT = 1 << 58      # document ids: 0 <= id < 2^58 (include/meerqat_hip.h)
NORMS = (None, "gzmuv", "zmuv")
DEFMINS = (False, True)
ALL_METRICS = ("mrr@100", "mrr", "mrr@1", "precision@5", "precision", "hit_rate@3", "recall@10", "recall", "precision@1000")

Case = collections.namedtuple("Case", "name n_runs K nq metrics purpose build")
Fit = collections.namedtuple("Fit", "per_q mean gap fused")   # per_q [T, nq], mean [T], smallest relative gap, the fused runs


def nsort_of(n_runs, K, fit=True):
    """The sort size the library computes (next_pow2 in csrc/fuse.hip, floor 64; the fit entry raises it to FT)."""
    p = 64
    while p < n_runs * K:
        p <<= 1
    return max(p, FT) if fit else p


def fit_lds_bytes(n_runs, K):
    """Dynamic LDS of fuse_fit_kernel: keys, scores, fused scores (8 bytes each), head positions and relevant heads (4 each)."""
    return nsort_of(n_runs, K) * (3 * 8 + 2 * 4)


# ---------------------------------------------------------------------------------------------------------------- generators
def make_runs(seed, nq, n_runs, K, n_docs, levels=False):
    rng = np.random.default_rng(seed)
    runs = []
    for r in range(n_runs):
        run = {}
        for q in range(nq):
            kk = K if (5 * q + r) % 7 != 3 else int(rng.integers(1, K + 1))
            docs = rng.choice(n_docs, size=kk, replace=False)
            if levels:
                base = rng.integers(0, 4, kk).astype(np.float32) * np.float32(0.5)
            else:
                base = rng.standard_normal(kk).astype(np.float32)
            scores = np.sort(base * (r + 1) + 3 * r)[::-1]
            run[f"q{q}"] = {str(int(d)): float(s) for d, s in zip(docs, scores)}
        runs.append(run)
    return runs


def union_of(runs, q):
    return set().union(*[run[q].keys() for run in runs])


def make_qrels(seed, runs, n_docs, density, p_zero=1 / 3, single_every=3):
    """Judgements over each query's union: `density` of it judged, 0 with probability p_zero, else 1 or 2; queries 2, 7, 12, ...
    without judgements; every `single_every`-th query (1, 4, ...) with ONE relevant document; every fourth query also holds a
    relevant document outside the pool (no run can hold it)."""
    rng = np.random.default_rng(seed)
    qrels = {}
    for n, q in enumerate(runs[0]):
        if n % 5 == 2:
            continue
        union = sorted(union_of(runs, q), key=int)
        if single_every and n % single_every == 1:
            judged = {union[int(i)]: 1 for i in rng.choice(len(union), size=min(1, len(union)), replace=False)}
        else:
            take = int(round(density * len(union)))
            judged = {union[int(i)]: (0 if rng.random() < p_zero else int(rng.integers(1, 3)))
                      for i in rng.choice(len(union), size=take, replace=False)}
        if n % 4 == 0:
            judged[str(n_docs + n)] = 1
        qrels[q] = judged
    return qrels


def make_trials(seed, n_runs, n_random=5):
    rng = np.random.default_rng(seed)
    unit = lambda i: [1.0 if j == i else 0.0 for j in range(n_runs)]
    out = [unit(0), unit(n_runs - 1), [1.0 / n_runs] * n_runs]
    if n_runs >= 3:
        out.append([0.5 if j in (0, n_runs // 2) else 0.0 for j in range(n_runs)])
        out.append([0.3 if j % 2 else 0.0 for j in range(n_runs)])
    for _ in range(200):
        if len(out) >= (5 if n_runs >= 3 else 3) + n_random:
            break
        out.append([int(k) / 10 for k in rng.integers(0, 11, n_runs)])
    trials = []
    for w in out:
        if any(w) and w not in trials:
            trials.append(w)
    return trials


# ---------------------------------------------------------------------------------------------------------------- reference
def reference_fused(runs, trials, norm, defmin):
    """The fused run of every trial, best first (equal scores by ascending id: oracle.fuse.wsum's rule)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # np.mean / np.std of a run without any result (gzmuv)
        prepared = ofuse.default_minimum(runs) if defmin else runs
        prepared = [ofuse.NORMS[norm](run) for run in prepared]
    return [ofuse.wsum(prepared, w) for w in trials]


def smallest_gap(fused_runs):
    """Smallest difference of distinct neighbouring fused scores relative to max(1, max |score|) of the query; inf without any."""
    gap = np.inf
    for fused in fused_runs:
        for results in fused.values():
            s = np.array(list(results.values()), dtype=np.float64)
            if len(s) < 2:
                continue
            d = s[:-1] - s[1:]
            d = d[d > 0]
            if len(d):
                gap = min(gap, float(d.min()) / max(1.0, float(np.abs(s).max())))
    return gap


def descending_id_ties(fused):
    """The same fused run under the OPPOSITE tie rule: equal scores by descending id."""
    return {q: dict(sorted(results.items(), key=lambda kv: (-kv[1], -int(kv[0])))) for q, results in fused.items()}


def per_query(fused_runs, qrels, metric):
    return np.array([ofuse.rank_metric(fused, qrels, metric)[1] for fused in fused_runs], dtype=np.float64).reshape(len(fused_runs), -1)


def reference_fit(runs, qrels, trials, norm, defmin, metric, fused=None):
    """Every trial fused and scored by the restatement: per-query values [T, nq], their np.mean per trial, the smallest relative
    gap between distinct neighbouring fused scores.  `fused`: the result of reference_fused for the same arguments, to share."""
    if fused is None:
        fused = reference_fused(runs, trials, norm, defmin)
    per_q = per_query(fused, qrels, metric)
    mean = np.array([np.mean(row) if len(row) else 0.0 for row in per_q], dtype=np.float64)
    return Fit(per_q, mean, smallest_gap(fused), fused)


# ---------------------------------------------------------------------------------------------------------------- the cases
def _random_case(seed, nq, n_runs, K, n_docs, density, levels=False, p_zero=1 / 3, single_every=3):
    def build():
        runs = make_runs(seed, nq, n_runs, K, n_docs, levels)
        return runs, make_qrels(seed + 1, runs, n_docs, density, p_zero, single_every)
    return build


def _many_runs():
    runs = make_runs(50, 9, 7, 40, 200)
    runs[1]["q2"], runs[4]["q2"] = {}, {}
    return runs, make_qrels(51, runs, 200, 0.2)


def _hollow():
    runs = make_runs(60, 10, 3, 20, 60)
    runs[1] = {q: {} for q in runs[1]}            # a run without any result
    for run in runs:
        run["q3"] = {}                            # a query empty in every run
    qrels = make_qrels(61, runs, 60, 0.3)
    assert "q2" not in qrels and "q7" not in qrels   # queries without judgements
    qrels["q3"] = {"5": 1}                        # judged, but the query retrieved nothing
    qrels["q6"] = {"1000": 1, "1001": 2, "1002": 0}  # every relevant document is outside the pool
    return runs, qrels


BIG = ID_LIMIT - 1


def _id_edge():
    """Dyadic scores: with dyadic weights every fused score is exact, tests/test_fuse_gpu.py states the order by hand."""
    b, b1 = str(BIG), str(BIG - 1)
    runs = [{"q0": {}, "q1": {}} for _ in range(MAX_RUNS)]
    runs[0] = {"q0": {b: 4.0, b1: 2.0, "0": 1.0}, "q1": {"0": 1.0, b: 1.0}}
    runs[7] = {"q0": {"0": 0.5, "7": 0.125}, "q1": {}}
    runs[31] = {"q0": {b1: 3.0, "0": 2.5, b: 0.5, "5": 0.25}, "q1": {b1: 2.0, b: 1.0}}
    qrels = {"q0": {b: 1, "0": 2, b1: 0}, "q1": {b1: 1, str(BIG - 2): 1}}
    return runs, qrels


def cases():
    C = Case
    return [
        C("floor", 2, 100, 48, ALL_METRICS, "the shipped dpr+clip shape: nsort 256, one compaction pass", _random_case(10, 48, 2, 100, 400, 0.1)),
        C("two_pass", 4, 100, 24, ("mrr@100", "recall@10"), "nsort 512; a union above 256: the per-head loops step twice",
          _random_case(20, 24, 4, 100, 1000, 0.1)),
        C("dense_qrels", 4, 100, 12, ("precision", "recall"), "above 256 relevant union documents: the rank count steps twice",
          _random_case(30, 12, 4, 100, 600, 0.98, p_zero=0.02, single_every=0)),
        C("cap", 32, 128, 3, ("precision@1000", "mrr"), "n_runs * K = 4096: nsort 4096, 128 KB of dynamic LDS, 32 weights",
          _random_case(40, 3, 32, 128, 100000, 0.05, single_every=0)),
        C("many_runs", 7, 40, 9, ("hit_rate@3", "precision@5"), "7 runs, 280 entries in nsort 512; a query empty in some runs", _many_runs),
        C("single", 1, 1, 5, ("mrr@1", "recall"), "K = 1, one run, trial [1.0]; nsort raised 64 -> 256; one-element zmuv std at the floor",
          _random_case(70, 5, 1, 1, 3, 1.0)),
        C("hollow", 3, 20, 10, ("precision", "hit_rate@3"), "an empty union, a run without results, no judgements, unreachable relevants",
          _hollow),
        C("ties", 3, 50, 10, ALL_METRICS, "levels scores, a small pool: exact ties decide the rank of relevant documents (norm=None)",
          _random_case(80, 10, 3, 50, 80, 0.3, levels=True)),
        C("id_edge", 32, 4, 2, ("mrr@1", "precision@5"), "ids 2^58 - 1, 2^58 - 2 and 0 in runs 0 and 31: every bit of the sort key",
          _id_edge),
    ]


CASES = {c.name: c for c in cases()}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(runs, qrels, trials) of a case; shared, not to be modified."""
    runs, qrels = CASES[name].build()
    return runs, qrels, make_trials(len(name) + 100 * len(runs), len(runs))


@functools.lru_cache(maxsize=None)
def case_fused(name, norm, defmin):
    runs, _, trials = case_data(name)
    return reference_fused(runs, trials, norm, defmin)


def case_fit(name, norm, defmin, metric):
    runs, qrels, trials = case_data(name)
    return reference_fit(runs, qrels, trials, norm, defmin, metric, fused=case_fused(name, norm, defmin))


def regime(name):
    """The figures the case table speaks of, from the data alone."""
    case = CASES[name]
    runs, qrels, trials = case_data(name)
    unions = {q: union_of(runs, q) for q in runs[0]}
    relevant = {q: sum(1 for d in u if qrels.get(q, {}).get(d, 0) >= 1) for q, u in unions.items()}
    return {"n_runs": len(runs), "K": max([1] + [len(res) for run in runs for res in run.values()]), "nq": len(runs[0]),
            "nsort": nsort_of(case.n_runs, case.K), "lds": fit_lds_bytes(case.n_runs, case.K), "trials": len(trials),
            "max_union": max(len(u) for u in unions.values()), "min_union": min(len(u) for u in unions.values()),
            "max_relevant": max(relevant.values())}
