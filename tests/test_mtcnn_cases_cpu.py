"""The conditions under which the end-to-end MTCNN test (tests/test_mtcnn_gpu.py) means something, checked on the restatements alone
(tests/mtcnn_cases.py): enough images count, enough boxes survive every stage, faces and a face-less image both occur, and every
NMS site has something to suppress."""
import numpy as np

from tests import mtcnn_cases
from tests import mtcnn_restatement as R


def test_set_has_three_sizes_in_range():
    sizes = {im.shape[:2] for im in mtcnn_cases.end_to_end_set()["images"]}
    assert len(mtcnn_cases.end_to_end_set()["images"]) == 16 and len(sizes) >= 3
    assert all(40 <= s <= 96 for hw in sizes for s in hw)


def test_at_most_two_images_left_out():
    assert len(mtcnn_cases.end_to_end_set()["counted"]) >= 14


def test_boxes_survive_every_stage():
    counts = mtcnn_cases.end_to_end_set()["f64"]["counts"]
    for k, stage in enumerate(R.STAGES):
        assert (counts[:, k] >= 3).sum() >= 12, (stage, counts[:, k])


def test_faces_and_a_faceless_image():
    final = mtcnn_cases.end_to_end_set()["f64"]["counts"][:, -1]
    assert (final > 0).sum() >= 8 and (final == 0).sum() >= 1, final


def test_every_nms_site_suppresses():
    traces = mtcnn_cases.end_to_end_set()["f64"]["traces"]
    for site in ("nms1", "nms2", "nms3", "nms4"):
        assert any(a > b for a, b in (mtcnn_cases.stage_survivors(t)[site] for t in traces)), site


def test_thresholds_sit_between_outputs():
    """quantile thresholds are midpoints: no float64 output equals one, so `>=` and `>` agree on the set"""
    s = mtcnn_cases.end_to_end_set()
    for t in s["f64"]["traces"]:
        assert all(not np.any(lv["prob"] == s["thresholds"][0]) for lv in t["levels"])
        assert not np.any(t.get("rnet_score", np.zeros(0)) == s["thresholds"][1])
        assert not np.any(t.get("onet_score", np.zeros(0)) == s["thresholds"][2])
    assert any("onet_score" in t for t in s["f64"]["traces"])
