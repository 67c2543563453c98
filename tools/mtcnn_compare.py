#!/usr/bin/env python3
"""Pins the device MTCNN against facenet_pytorch where that package is importable (it is not where this repository is built: then
this tool says so and does nothing).  Runs `facenet_pytorch.MTCNN(keep_all=True, select_largest=False)` and
`viquae_amd.image.face_detection.MTCNN` with the same published weights on the given images and reports, per image, the two face
counts, and for equal counts the largest differences of boxes, probabilities and landmarks in input order.  What a pin must
confirm is listed in tests/mtcnn_restatement.py (scale rule, +1 conventions, flatten order, crop-skip rule, order of the final
lists, output dtypes).

    python tools/mtcnn_compare.py image1.jpg [image2.png ...] [--weights DIR]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("images", nargs="+")
    ap.add_argument("--weights", help="directory with pnet.pt, rnet.pt, onet.pt (default: facenet_pytorch's own data directory)")
    args = ap.parse_args()
    try:
        import facenet_pytorch
    except ImportError:
        print(json.dumps({"skipped": "facenet_pytorch is not importable: parity with the published implementation stays unpinned"}))
        return 0
    from PIL import Image
    from viquae_amd.image.face_detection import MTCNN
    weights = args.weights or os.path.join(os.path.dirname(facenet_pytorch.__file__), "data")
    theirs = facenet_pytorch.MTCNN(keep_all=True, select_largest=False, device="cuda")
    ours = MTCNN(keep_all=True, select_largest=False, device="cuda", weights=weights)
    report = []
    for path in args.images:
        image = Image.open(path).convert("RGB")
        tb, tp, tl = theirs.detect(image, landmarks=True)
        ob, op, ol = ours.detect(image, landmarks=True)
        row = {"image": path, "faces_facenet_pytorch": 0 if tb is None else len(tb), "faces_hip": 0 if ob is None else len(ob)}
        if tb is not None and ob is not None and len(tb) == len(ob):
            row.update(max_box_difference=float(np.abs(tb - ob).max()), max_prob_difference=float(np.abs(tp - op).max()),
                       max_landmark_difference=float(np.abs(tl - ol).max()), dtypes=[str(tb.dtype), str(ob.dtype)])
        report.append(row)
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
