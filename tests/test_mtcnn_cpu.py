"""Host side of the MTCNN stage (no GPU): the restatement's NMS against a brute-force definition, ``select_boxes``, ``scale_box``,
weight loading and packing, the deliberate gaps, and the committed golden of the float64 restatement."""
import os

import numpy as np
import pytest
import torch

from tests import mtcnn_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _overlap(a, b, method):
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]) + 1)
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]) + 1)
    inter = w * h
    aa, ab = (a[2] - a[0] + 1) * (a[3] - a[1] + 1), (b[2] - b[0] + 1) * (b[3] - b[1] + 1)
    return inter / min(aa, ab) if method == "Min" else inter / (aa + ab - inter)


def _brute_nms(boxes, scores, thr, method):
    """the definition: walk the boxes best first (ties: lower index); keep one iff no kept box overlaps it by more than thr"""
    order = sorted(range(len(scores)), key=lambda i: (-scores[i], i))
    keep = []
    for i in order:
        if all(_overlap(boxes[k], boxes[i], method) <= thr for k in keep):
            keep.append(i)
    return keep


@pytest.mark.parametrize("method", ["Union", "Min"])
@pytest.mark.parametrize("n", [0, 1, 2, 60])
def test_restatement_nms_is_greedy_nms(n, method):
    rng = np.random.default_rng(n)
    xy = rng.integers(0, 30, (n, 2)).astype(np.float64)
    boxes = np.concatenate([xy, xy + rng.integers(3, 25, (n, 2))], axis=1)
    scores = rng.integers(0, 8, n) / 8.0   # many equal scores
    for thr in (0.3, 0.5, 0.7):
        assert R.nms(boxes, scores, thr, method).tolist() == _brute_nms(boxes, scores, thr, method)


def test_restatement_nms_exact_threshold_and_min_mode():
    boxes = np.array([[0, 0, 9, 9], [0, 0, 9, 19], [2, 2, 5, 5]], np.float32)   # IoU(0, 1) = 100 / 200 exactly; 2 inside 0
    scores = np.array([0.9, 0.8, 0.7], np.float32)
    assert R.nms(boxes[:2], scores[:2], 0.5).tolist() == [0, 1]          # equal to the threshold: kept
    assert R.nms(boxes[:2], scores[:2], 0.49).tolist() == [0]
    assert R.nms(boxes[[0, 2]], scores[[0, 2]], 0.7).tolist() == [0, 1]   # IoU 16 / 100
    assert R.nms(boxes[[0, 2]], scores[[0, 2]], 0.7, "Min").tolist() == [0]


def _host_model():
    """an MTCNN object without a device: select_boxes and the refusals are host code"""
    from viquae_amd.image.face_detection import MTCNN
    m = MTCNN.__new__(MTCNN)
    m.keep_all, m.selection_method, m.min_face_size = False, "probability", 20
    return m


def test_select_boxes():
    m = _host_model()
    boxes = np.array([[0, 0, 10, 10], [0, 0, 30, 20], [5, 5, 9, 9]], np.float32)
    probs = np.array([0.7, 0.8, 0.95], np.float32)
    points = np.arange(30, dtype=np.float32).reshape(3, 5, 2)
    b, p, l = m.select_boxes(boxes, probs, points, np.zeros((40, 40, 3), np.uint8), method="probability")
    assert b.shape == (1, 4) and np.array_equal(b[0], boxes[2]) and p.tolist() == [probs[2]] and np.array_equal(l[0], points[2])
    b, p, l = m.select_boxes(boxes, probs, points, np.zeros((40, 40, 3), np.uint8), method="largest")
    assert np.array_equal(b[0], boxes[1]) and np.array_equal(l[0], points[1])
    imgs = [np.zeros((40, 40, 3), np.uint8)] * 2
    b, p, l = m.select_boxes([boxes, None], [probs, [None]], [points, None], imgs, method="probability")
    assert len(b) == 2 and b[1] is None and p[1] == [None] and l[1] is None and np.array_equal(b[0][0], boxes[2])


def test_the_three_not_implemented_errors(tmp_path):
    from viquae_amd.image import face_detection as fd
    m = _host_model()
    with pytest.raises(NotImplementedError):
        m.extract(None, None, None)
    with pytest.raises(NotImplementedError):
        m.forward(np.zeros((40, 40, 3), np.uint8), save_path="face.png")
    with pytest.raises(NotImplementedError):
        fd.detect_face(["a.jpg"], m, save_root_path=tmp_path)
    for method in ("center_weighted_size", "largest_over_threshold"):
        with pytest.raises(NotImplementedError):
            m.select_boxes(None, None, None, None, method=method)


def test_weight_loading_and_missing_file_message(tmp_path, monkeypatch):
    from viquae_amd.image import face_detection as fd
    state = R.seeded_state(0)
    monkeypatch.delenv("MQ_MTCNN_WEIGHTS", raising=False)
    with pytest.raises(FileNotFoundError, match="facenet_pytorch/data"):
        fd.load_state_dicts(None)
    for net in ("pnet", "rnet"):
        torch.save({k: torch.from_numpy(v) for k, v in state[net].items()}, tmp_path / f"{net}.pt")
    with pytest.raises(FileNotFoundError, match=r"onet\.pt is missing: copy pnet\.pt, rnet\.pt and onet\.pt from facenet_pytorch/data"):
        fd.load_state_dicts(tmp_path)
    torch.save({k: torch.from_numpy(v) for k, v in state["onet"].items()}, tmp_path / "onet.pt")
    monkeypatch.setenv("MQ_MTCNN_WEIGHTS", str(tmp_path))
    loaded = fd.load_state_dicts(None)
    assert all(np.array_equal(loaded[n][k], state[n][k]) for n in state for k in state[n])
    assert all(np.array_equal(a, b) for a, b in zip(fd.pack_weights(loaded).values(), fd.pack_weights(fd.load_state_dicts(state)).values()))


def test_packed_layout_matches_the_library(hip_lib):
    from viquae_amd.image import face_detection as fd
    state = R.seeded_state(1)
    packed = fd.pack_weights(state)
    assert [packed[n].size for n in fd.NETS] == [hip_lib.mq_mtcnn_weight_floats(i) for i in range(3)]
    assert hip_lib.mq_mtcnn_weight_floats(3) == 0
    # dense4's packed row (c, y, x) holds the published input feature (x * 3 + y) * 64 + c
    r = packed["rnet"]
    off = sum(state["rnet"][k].size for k in ("conv1.weight", "conv1.bias", "prelu1.weight", "conv2.weight", "conv2.bias", "prelu2.weight",
                                                "conv3.weight", "conv3.bias", "prelu3.weight"))
    d4 = r[off:off + 576 * 128].reshape(576, 128)
    c, y, x = 5, 2, 1
    assert np.array_equal(d4[(c * 3 + y) * 3 + x], state["rnet"]["dense4.weight"][:, (x * 3 + y) * 64 + c])
    bad = {n: dict(sd) for n, sd in state.items()}
    bad["pnet"]["conv2.weight"] = bad["pnet"]["conv2.weight"][:, :5]
    with pytest.raises(ValueError, match="conv2"):
        fd.pack_weights(bad)


def test_argument_validation_needs_no_gpu(hip_lib):
    assert hip_lib.mq_mtcnn_nms_workspace_bytes(10) == 360 and hip_lib.mq_mtcnn_nms_workspace_bytes(0) == 0
    assert hip_lib.mq_mtcnn_nms_f32(None, 4, None, None, 1, 0, None, None, 0.0, 0.5, 0, None, None, None, None, None, None, 0, None) == -1
    assert hip_lib.mq_mtcnn_rnet_f32(None, 3, None, None, None, None) == -1
    assert hip_lib.mq_mtcnn_rnet_f32(None, 0, None, None, None, None) == 0
    assert hip_lib.mq_mtcnn_resample_u8_f32(None, None, None, 1, None, 2, 4, None, 8, None, None) == -1


def test_scale_pyramid_and_small_images():
    from viquae_amd.image import face_detection as fd
    assert fd.scale_pyramid(20, 20, 20, 0.709) == [0.6] and fd.scale_pyramid(19, 40, 20, 0.709) == []
    assert fd.scale_pyramid(37, 53, 20, 0.709) == R.scale_pyramid(37, 53)
    s = fd.scale_pyramid(384, 512, 20, 0.709)
    assert min(384, 512) * s[-1] >= 12 > min(384, 512) * s[-1] * 0.709


def test_scale_box_reference_arithmetic(tmp_path, monkeypatch):
    from PIL import Image
    from viquae_amd.data import loading
    from viquae_amd.image import face_box
    monkeypatch.setattr(loading, "IMAGE_PATH", tmp_path)
    Image.new("RGB", (50, 40)).save(tmp_path / "a.png")
    box = [[5.0, 4.0, 30.0, 24.0], [10.0, 10.0, 20.0, 30.0]]
    lm = [[[10.0, 8.0]] * 5, [[25.0, 20.0]] * 5]
    item = face_box.scale_box({"image": "a.png", "face_box": box, "face_landmarks": lm})
    want = np.array([[0.1, 0.1, 0.6, 0.6, 0.5, 0.5, 0.25], [0.2, 0.25, 0.4, 0.75, 0.2, 0.5, 0.1]])
    assert item["face_box"].shape == (2, 7) and np.allclose(item["face_box"], want, rtol=0, atol=1e-15)
    assert np.array_equal(item["face_box"][:, 4], item["face_box"][:, 2] - item["face_box"][:, 0])
    assert np.allclose(item["face_landmarks"][0], [[0.2, 0.2]] * 5) and np.allclose(item["face_landmarks"][1], [[0.5, 0.5]] * 5)
    untouched = {"image": "missing.png", "face_box": None, "face_landmarks": None}
    assert face_box.scale_box(dict(untouched)) == untouched   # no face: the file is not even opened


def test_golden_of_the_float64_restatement():
    """tools/make_golden_mtcnn.py wrote the float64 restatement's per-stage counts and final outputs for four images of the set: an
    edit of the restatement cannot move the target silently."""
    from tests import mtcnn_cases
    s = mtcnn_cases.end_to_end_set()
    g = np.load(os.path.join(ROOT, "tests", "golden", "mtcnn_seeded.npz"))
    assert np.allclose(g["thresholds"], s["thresholds"], rtol=0, atol=1e-12)
    for j, i in enumerate(g["images"].tolist()):
        assert np.array_equal(g["counts"][j], s["f64"]["counts"][i])
        boxes, probs, points = s["f64"]["boxes"][i], s["f64"]["probs"][i], s["f64"]["points"][i]
        if boxes is None:
            assert g[f"boxes_{i}"].size == 0
            continue
        assert np.allclose(g[f"boxes_{i}"], np.concatenate([boxes, probs[:, None]], axis=1), rtol=0, atol=1e-4)
        assert np.allclose(g[f"points_{i}"], points, rtol=0, atol=1e-4)
