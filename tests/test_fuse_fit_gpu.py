"""The weight search of ``Fusion.fit`` on the MI355X (mq_fuse_fit_wsum_f64: fuse_stats_kernel, fuse_moments_kernel,
fuse_fit_kernel, np_mean_rows_kernel) against the restatement, on the cases of tests/fuse_cases.py: every sort size from the
256-entry floor to the 4096-entry cap, unions and relevant lists beyond one pass of the 256 threads, 32 runs, empty unions, K = 1
and ids at the limit of the sort key.

Everything is compared EXACTLY.  Metric values are ratios of small integers computed in f64 from ranks; under norm=None the fused
scores are bit-identical to the restatement's by construction, and under 'gzmuv' / 'zmuv' tests/test_fuse_cases_cpu.py proves that
distinct neighbouring fused scores of every case lie more than 4e-12 (relative) apart, so the ~1e-15 difference of the moments
cannot move a rank."""
import numpy as np
import pytest
import torch

from oracle import fuse as ofuse
from tests import fuse_cases as fc
from viquae_amd import _lib
from viquae_amd.ir import fuse as hfuse
from viquae_amd.ir import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_TABLES = {}


def tables(name):
    """The case on the device, built the way fit_wsum builds it: (q_ids, ids, scores, rel_ptr, rel_ids, trials)."""
    if name not in _TABLES:
        runs, qrels, trials = fc.case_data(name)
        q_ids, doc_names, ids, scores = hfuse.runs_to_tables(runs, DEV)
        assert doc_names is None and tuple(ids.shape) == (fc.CASES[name].n_runs, fc.CASES[name].nq, fc.CASES[name].K)
        ptr, rel = M.qrels_to_csr(qrels, q_ids, None)
        _TABLES[name] = (q_ids, ids, scores, torch.from_numpy(ptr).to(DEV),
                         torch.from_numpy(rel if rel.size else np.zeros(1, np.int64)).to(DEV),
                         torch.tensor(trials, dtype=torch.float64))
    return _TABLES[name]


@pytest.mark.parametrize("defmin", fc.DEFMINS)
@pytest.mark.parametrize("norm", fc.NORMS)
@pytest.mark.parametrize("name", list(fc.CASES))
def test_fit_equals_the_reference_exactly(name, norm, defmin):
    case = fc.CASES[name]
    runs, qrels, trials = fc.case_data(name)
    q_ids, ids, scores, ptr, rel, trials_t = tables(name)
    got = {}
    for metric in case.metrics:
        code, k = M.parse_metric(metric)
        mean, per_q = hfuse.fit_tables(ids, scores, trials_t, ptr, rel, code, k, norm=norm, defmin=defmin)
        mean, per_q = mean.cpu().numpy(), per_q.cpu().numpy()
        want = fc.case_fit(name, norm, defmin, metric)
        assert per_q.shape == want.per_q.shape == (len(trials), case.nq)
        bad = np.argwhere(per_q != want.per_q)
        assert np.array_equal(per_q, want.per_q), (metric, len(bad), bad[:5].tolist(), per_q[tuple(bad[0])], want.per_q[tuple(bad[0])])
        assert np.array_equal(mean, np.mean(per_q, axis=1)), metric      # np.mean's pairwise summation, bit for bit
        got[metric] = per_q
    # the sibling kernel: fuse_combine_kernel writes the order fuse_fit_kernel claims to rank by
    for t in (len(trials) // 2, len(trials) - 1):
        f_ids, f_scores, counts = hfuse.fuse_tables(ids, scores, trials[t], norm=norm, defmin=defmin)
        fused = hfuse.tables_to_run(q_ids, None, f_ids, f_scores, counts)
        for metric in case.metrics:
            values = ofuse.rank_metric(fused, qrels, metric)[1]
            assert np.array_equal(np.array(values, dtype=np.float64), got[metric][t]), (metric, t)


def test_fit_wsum_on_the_shipped_shape_runs_the_whole_grid():
    runs, qrels, _ = fc.case_data("floor")
    best, trials = ofuse.fusion_fit(runs, qrels, norm="gzmuv", defmin=True, metric="mrr@100")
    got_best, got_trials = hfuse.fit_wsum(runs, qrels, norm="gzmuv", defmin=True, metric="mrr@100")
    assert len(trials) == 11 and [w for w, _ in got_trials] == [list(w) for w, _ in trials]
    diff = np.abs(np.array([s for _, s in got_trials]) - np.array([s for _, s in trials]))
    assert diff.max() <= 1e-12, diff.max()
    assert got_best == best


def _fit_call(lib, n_runs, nq, K, n_trials, metric=0, metric_k=0, ws_short=0, norm=1):
    """mq_fuse_fit_wsum_f64 on zero-filled tables that are as large as the call claims: a call that is not refused reads and
    writes inside them.  rel_ids and the stream are null (legal: no query has a relevant document)."""
    ids = torch.full((n_runs, nq, K), -1, dtype=torch.int64, device=DEV)
    scores = torch.zeros((n_runs, nq, K), dtype=torch.float64, device=DEV)
    trials = torch.zeros((max(n_trials, 1), n_runs), dtype=torch.float64, device=DEV)
    ptr = torch.zeros((nq + 1,), dtype=torch.int64, device=DEV)
    per_q = torch.full((max(n_trials, 1), nq), -7.0, dtype=torch.float64, device=DEV)
    mean = torch.full((max(n_trials, 1),), -7.0, dtype=torch.float64, device=DEV)
    ws_bytes = max(int(lib.mq_fuse_workspace_bytes(min(n_runs, fc.MAX_RUNS), nq, K)), 8 * (6 * n_runs * nq + 2 * n_runs))
    ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device=DEV)
    rc = lib.mq_fuse_fit_wsum_f64(ids.data_ptr(), scores.data_ptr(), n_runs, nq, K, trials.data_ptr(), n_trials, norm, 1,
                                  ptr.data_ptr(), None, metric, metric_k, per_q.data_ptr(), mean.data_ptr(), ws.data_ptr(),
                                  ws_bytes - ws_short, None)
    torch.cuda.synchronize()
    return rc, per_q.cpu().numpy(), mean.cpu().numpy()


def test_fit_entry_refuses_cleanly(hip_lib):
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
    refused = [(dict(n_runs=17, K=241), EUNSUPPORTED),          # 4097 entries
               (dict(n_runs=1, K=4097), EUNSUPPORTED),
               (dict(n_runs=33, K=2), EINVAL),
               (dict(n_trials=0), EINVAL),
               (dict(metric=4), EINVAL), (dict(metric=-1), EINVAL),
               (dict(metric_k=-1), EINVAL),
               (dict(norm=3), EINVAL),
               (dict(ws_short=1), EWORKSPACE)]
    for kwargs, want in refused:
        args = dict(n_runs=2, nq=3, K=4, n_trials=2)
        args.update(kwargs)
        rc, per_q, mean = _fit_call(hip_lib, **args)
        assert rc == want, (kwargs, rc)
        assert (per_q == -7.0).all() and (mean == -7.0).all(), kwargs      # nothing ran
    assert hip_lib.mq_fuse_fit_wsum_f64(None, None, 2, 3, 4, None, 2, 1, 1, None, None, 0, 0, None, None, None, 0, None) == EINVAL
    # the same call, accepted: all-empty tables score 0 everywhere, at the entry limit as well
    for kwargs in (dict(), dict(n_runs=32, K=128), dict(n_runs=1, K=4096)):
        args = dict(n_runs=2, nq=3, K=4, n_trials=2)
        args.update(kwargs)
        rc, per_q, mean = _fit_call(hip_lib, **args)
        assert rc == 0 and (per_q == 0.0).all() and (mean == 0.0).all(), kwargs
    with pytest.raises(_lib.MeerqatHipError):
        ids = torch.full((17, 1, 241), -1, dtype=torch.int64, device=DEV)
        hfuse.fit_tables(ids, ids.double(), torch.zeros((1, 17), dtype=torch.float64), torch.zeros(2, dtype=torch.int64, device=DEV),
                         torch.zeros(1, dtype=torch.int64, device=DEV), 0, 0)
