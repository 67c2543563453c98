"""The seeded end-to-end set of the MTCNN tests, computed once per process from the restatements alone: 16 smooth random images of
16 sizes between 40 and 96 pixels, seeded weights, thresholds at quantiles of the float64 restatement's own outputs.

The set runs with ``factor = 0.85`` instead of the default 0.709: the second NMS site (IoU 0.7 across scales) compares unrefined
boxes of neighbouring pyramid levels, whose areas differ by ``factor**2`` -- at 0.709 their IoU cannot exceed 0.51, so that site
could never suppress anything and one of the set's conditions (tests/test_mtcnn_cases_cpu.py) could not hold."""
import functools

import numpy as np
import torch

from tests import mtcnn_restatement as R


@functools.lru_cache(maxsize=None)
def end_to_end_set():
    state = R.seeded_state(R.WEIGHT_SEED)
    images = R.seeded_images()
    thresholds = R.quantile_thresholds(images, state, R.QUANTILES, factor=R.SET_FACTOR)
    out = dict(state=state, images=images, thresholds=thresholds, factor=R.SET_FACTOR)
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        traces = []
        boxes, probs, points = R.detect(images, state, thresholds=thresholds, factor=R.SET_FACTOR, dtype=dtype, select_largest=False,
                                        traces=traces)
        out[name] = dict(boxes=boxes, probs=probs, points=points, traces=traces,
                         counts=np.array([[t["counts"][s] for s in R.STAGES] for t in traces]))
    # an image counts only if both restatements keep the same number of boxes after every stage (the others sit on a threshold)
    out["counted"] = [i for i in range(len(images)) if (out["f64"]["counts"][i] == out["f32"]["counts"][i]).all()]
    return out


def stage_survivors(trace):
    """per NMS site of one image's float64 trace: (boxes entering, boxes leaving)"""
    c = trace["counts"]
    return dict(nms1=(c["pnet"], c["nms1"]), nms2=(c["nms1"], c["nms2"]), nms3=(c["rnet"], c["nms3"]), nms4=(c["onet"], c["nms4"]))
