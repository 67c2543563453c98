"""GPU suite of the reader stage: the log-softmax and span-search kernels of csrc/reader.hip, the MultiPassageBERT logits
against Hugging Face (golden minted by tools/make_golden_reader.py) and the `test` CLI end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import reader_restatement as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = rr.load_golden()


def _ulp(x):
    x = np.abs(np.asarray(x, np.float32))
    return np.spacing(x).astype(np.float64)


@pytest.mark.parametrize("N, M, L, scale", [(1, 1, 7, 1.0), (3, 5, 33, 4.0), (8, 24, 256, 3.0), (16, 24, 97, 1.0),
                                            (4, 12, 200, 1e4), (2, 24, 130, 80.0), (16, 1, 256, 30.0)])
def test_log_softmax(hip_lib, N, M, L, scale):
    from viquae_amd.rc.reader import log_softmax_per_question
    rng = np.random.default_rng(N * 1000 + M * 10 + L)
    x = (rng.standard_normal((2, N, M, L)) * scale).astype(np.float32)
    if scale > 100:
        x[0, :, :, 3] += 5 * scale  # large-magnitude logits: most probabilities underflow
    dev = torch.from_numpy(x).cuda()
    sl, el, sp, ep = log_softmax_per_question(dev[0], dev[1], N, M, L)
    torch.cuda.synchronize()
    for k, (lp, p) in enumerate(((sl, sp), (el, ep))):
        x64 = x[k].reshape(N, M * L).astype(np.float64)
        ref = x64 - x64.max(1, keepdims=True)
        ref = ref - np.log(np.exp(ref).sum(1, keepdims=True))
        got = lp.cpu().numpy().reshape(N, M * L).astype(np.float64)
        assert np.all(np.abs(got - ref) <= 4e-6 * np.maximum(1.0, np.abs(ref))), np.abs(got - ref).max()
        p_ref = np.exp(got).astype(np.float32)
        p_got = p.cpu().numpy().reshape(N, M * L)
        assert np.all(np.abs(p_got.astype(np.float64) - np.exp(got)) <= 4 * _ulp(p_ref)), (k, scale)


def _spans_gpu(s, e, w, cbf):
    from viquae_amd.rc.reader import best_spans
    out = best_spans(torch.from_numpy(np.ascontiguousarray(s, np.float32)).cuda(),
                     torch.from_numpy(np.ascontiguousarray(e, np.float32)).cuda(), w, cbf)
    return torch.stack(out).cpu().numpy()


def test_spans_planted_cases(hip_lib):
    for case in GOLDEN["planted"]:
        s, e = np.array(case["start"], np.float32), np.array(case["end"], np.float32)
        w = None if case["weights"] is None else np.array(case["weights"], np.float32)
        got = _spans_gpu(s, e, w, case["cannot_be_first_token"])
        assert got.tolist() == case["reference"] == rr.best_spans(s, e, w, case["cannot_be_first_token"]).tolist(), case


def _planted_ties(rng, N, M, L):
    """probabilities with exact ties: one passage copied into another, values drawn from a few levels (many equal products),
    a passage of zeros and a passage of denormal-scale values"""
    levels = np.array([0, 2.0 ** -3, 2.0 ** -5, 0.1, 0.3], np.float32)
    s = levels[rng.integers(0, len(levels), (N, M, L))]
    e = levels[rng.integers(0, len(levels), (N, M, L))]
    if M >= 3:
        s[:, M - 1], e[:, M - 1] = s[:, 0], e[:, 0]
        s[:, 1] = 0
        s[:, 2] *= np.float32(1e-20)
        e[:, 2] *= np.float32(1e-19)
    return s, e


@pytest.mark.parametrize("N, M, L", [(1, 1, 16), (4, 3, 64), (8, 24, 256), (16, 7, 130), (3, 24, 200)])
@pytest.mark.parametrize("cbf", [True, False])
def test_spans_bit_identical_to_the_restatement(hip_lib, N, M, L, cbf):
    rng = np.random.default_rng(N * 7 + M * 3 + L)
    for kind in ("ties", "random", "tiny"):
        if kind == "ties":
            s, e = _planted_ties(rng, N, M, L)
        else:
            s, e = rng.random((N, M, L)).astype(np.float32), rng.random((N, M, L)).astype(np.float32)
            s, e = s / s.sum(), e / e.sum()
            if kind == "tiny":  # denormal products everywhere
                s, e = s * np.float32(1e-16), e * np.float32(1e-17)
        for w in (None, rr.shift_weights(rng.uniform(-2, 3, (N, M)).astype(np.float32)),
                  rng.uniform(1, 4, (N, M)).astype(np.float32), np.full((N, M), 0.5, np.float32)):
            assert np.array_equal(_spans_gpu(s, e, w, cbf), rr.best_spans(s, e, w, cbf)), (kind, w is None)


def test_span_arguments_are_checked(hip_lib):
    assert hip_lib.mq_reader_best_spans_f32(None, None, None, 1, 1, 8, 1, None, None, None, None) == -1
    assert hip_lib.mq_reader_best_spans_f32(None, None, None, 1, 2, 65536, 1, None, None, None, None) == -1
    assert hip_lib.mq_reader_log_softmax_f32(None, None, 1, 1, 8, None, None, None, None, None) == -1
    assert hip_lib.mq_reader_qa_head_f32(None, None, None, None, None, 4, 130, None) == -1


@pytest.mark.parametrize("size", ["tiny", "base2"])
@pytest.mark.parametrize("mode", ["split_bf16", "f32"])
def test_logits_against_hf(hip_lib, monkeypatch, size, mode):
    from viquae_amd.encoders import MultiPassageBERT
    monkeypatch.setenv("MQ_ENC_GEMM", mode)
    g = GOLDEN["sizes"][size]
    d = np.load(os.path.join(rr.GOLDEN, f"reader_{size}.npz"))
    vocab = len(GOLDEN["world"]["vocab"])
    state = rr.reader_state(g["config"], vocab, g["seed"])
    assert rr.state_checksum(state) == g["checksum"]
    model = MultiPassageBERT.from_state_dict(rr.hf_config(g["config"], vocab), state).cuda().eval()
    for bi in range(len(g["batches"])):
        inputs = {k: torch.from_numpy(d[f"b{bi}_{k}"].astype(np.int64)).cuda() for k in ("input_ids", "token_type_ids", "attention_mask")}
        out = model(**inputs)
        for k in ("start", "end"):
            got = out[f"{k}_logits"].cpu().numpy()
            assert got.shape == d[f"b{bi}_{k}_logits"].shape
            assert np.abs(got - d[f"b{bi}_{k}_logits"]).max() <= 1e-3, (size, mode, bi, k)


@pytest.mark.parametrize("source", ["search_key", "run_path"])
def test_cli_end_to_end(hip_lib, tmp_path, source):
    import yaml
    size = "tiny"
    g = GOLDEN["sizes"][size]
    paths = rr.write_world(str(tmp_path / "world"), GOLDEN["world"])
    ckpt = str(tmp_path / "reader")
    rr.write_checkpoint(ckpt, g["config"], len(GOLDEN["world"]["vocab"]), g["seed"])
    cfg = json.loads(json.dumps(GOLDEN["settings"]))
    cfg["trainer"] = {"default_root_dir": str(tmp_path), "accelerator": "gpu", "devices": 1}
    cfg["model"]["init_args"]["model_kwargs"]["pretrained_model_name_or_path"] = ckpt
    args = cfg["data"]["init_args"]
    args.update(kb=paths["kb"], dataset_path=paths["dataset"], tokenizer_name_or_path=paths["tokenizer"],
                run_path=paths["run"] if source == "run_path" else None)
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "viquae_amd.rc.reader", "test", "--config", str(tmp_path / "config.yaml"),
                          "--output", str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    d = np.load(os.path.join(rr.GOLDEN, f"reader_{size}.npz"))
    exceptions, compared = [], 0
    for name, key in (("predictions", "margin"), ("weighted_predictions", "weighted_margin")):
        got = json.load(open(out / f"{name}.json"))
        want = g[name]
        assert len(got) == len(want) == 16
        margin = np.concatenate([d[f"b{bi}_{key}"] for bi in range(2)], axis=1)
        for q in range(16):
            confident = margin[0, q] - margin[1, q] > 1e-2 * margin[0, q]
            if confident:
                compared += 1
                assert got[q] == want[q], (name, q)
            elif got[q] != want[q]:
                exceptions.append((name, q))
    print("near-tie questions whose answer differs from the golden:", exceptions)
    assert compared >= 16
    metrics = json.load(open(out / "metrics.json"))
    assert list(metrics) == ["exact_match", "f1", "weighted_exact_match", "weighted_f1"]
    if not exceptions:
        assert metrics == g["metrics"]
