"""Writes tests/golden/mtcnn_seeded.npz: the float64 MTCNN restatement's thresholds, per-stage counts and final outputs for four
images of the seeded end-to-end set (tests/mtcnn_cases.py), one of them without a face.  tests/test_mtcnn_cpu.py compares the
restatement against it, so that a later edit of the restatement cannot move the GPU tests' target silently.  CPU only.

    python tools/make_golden_mtcnn.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMAGES = (1, 2, 4, 12)


def main():
    from tests import mtcnn_cases
    s = mtcnn_cases.end_to_end_set()
    out = dict(thresholds=np.asarray(s["thresholds"], np.float64), images=np.asarray(IMAGES, np.int64),
               counts=s["f64"]["counts"][list(IMAGES)])
    for i in IMAGES:
        boxes, probs, points = s["f64"]["boxes"][i], s["f64"]["probs"][i], s["f64"]["points"][i]
        out[f"boxes_{i}"] = np.zeros((0, 5), np.float32) if boxes is None else np.concatenate([boxes, probs[:, None]], axis=1)
        out[f"points_{i}"] = np.zeros((0, 5, 2), np.float32) if boxes is None else points
    path = os.path.join(ROOT, "tests", "golden", "mtcnn_seeded.npz")
    np.savez(path, **out)
    print(path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
