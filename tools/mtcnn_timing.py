#!/usr/bin/env python3
"""MTCNN face detection (viquae_amd.image.face_detection.MTCNN, csrc/mtcnn.hip) throughput on 256 synthetic 512 x 384 images -- the
size the reference's `resize` stage leaves and the batch of EXPERIMENTS.rst -- with seeded weights and FIXED thresholds (quantiles of
the float64 restatement's outputs on four of the images), so that the per-image candidate counts after each stage are part of the
record: the rate means nothing without them.

Beside it, the same three networks through torch-ROCm's own fp32 operators on the same GPU in the same run
(tests/mtcnn_restatement.py's networks with their tensors on the device): P-Net on the whole batch per scale behind
`interpolate(mode="area")`, R-Net and O-Net on as many crops as the HIP path cut, in the published chunks of 512.  That leg has NO NMS,
box arithmetic, crop cutting or host round trip in it: it is a lower bound of what the published implementation spends, so the ratio
recorded here understates the gap.

Warm-up, then five windows, min to max; per-stage device times from events between the stages; one JSON line.

    python tools/mtcnn_timing.py [--batch 256] [--steps 3] [--no-baseline]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUANTILES = (0.995, 0.5, 0.5)


def windows(fn, steps, n_windows=5):
    out = []
    for _ in range(n_windows):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) / steps)
    return out


def main():
    from tests import mtcnn_restatement as R
    from viquae_amd import _lib
    from viquae_amd.image import face_detection as fd
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--restatement-images", type=int, default=8, help="images of the whole-restatement-on-the-device leg")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    images = [R.smooth_image(rng, 384, 512) for _ in range(args.batch)]
    state = R.seeded_state(R.WEIGHT_SEED)
    thresholds = R.quantile_thresholds(images[:4], state, QUANTILES)
    model = fd.MTCNN(thresholds=list(thresholds), select_largest=False, keep_all=True, device="cuda", weights=state)
    model.trace = True
    model.detect(images)   # warm-up; also the counts
    counts = model.last_counts
    model.trace = False
    out = {"workload": f"{args.batch} synthetic 512x384 images, seeded weights", "thresholds": [round(t, 6) for t in thresholds],
           "threshold_quantiles": QUANTILES, "scales_per_image": len(fd.scale_pyramid(384, 512, 20, 0.709)),
           "candidates_per_image_after": {s: {"mean": round(float(counts[:, k].mean()), 1), "max": int(counts[:, k].max())}
                                          for k, s in enumerate(fd.STAGES)},
           "host_reads_per_batch": fd.HOST_READS_PER_BATCH, "capacity_retries_in_warm_up": model.retries}
    w = windows(lambda: model.detect(images), args.steps)
    out["hip"] = {"images_per_s_min_max": [round(args.batch / max(w), 1), round(args.batch / min(w), 1)],
                  "ms_per_batch_min_max": [round(min(w) * 1e3, 2), round(max(w) * 1e3, 2)], "windows": 5, "batches_per_window": args.steps}
    model.stage_events = []
    model.detect(images)
    torch.cuda.synchronize()
    ev = model.stage_events
    model.stage_events = None
    out["hip"]["stage_ms"] = {b[0]: round(a[1].elapsed_time(b[1]), 3) for a, b in zip(ev[:-1], ev[1:])}
    out["hip"]["stage_ms"]["note"] = "device time between the stages' marks, each stage's host read included"
    if not args.no_baseline:
        base = {}
        try:
            torch.backends.cudnn.benchmark = True
            torch.backends.cudnn.allow_tf32 = False
            torch.backends.cuda.matmul.allow_tf32 = False
            dev_state = {n: {k: torch.from_numpy(v).cuda() for k, v in sd.items()} for n, sd in state.items()}
            batch = torch.from_numpy(np.stack(images)).cuda().permute(0, 3, 1, 2).float()
            n_r, n_o = int(counts[:, 2].sum()), int(counts[:, 4].sum())
            crops_r = torch.randn((max(n_r, 1), 3, 24, 24), device="cuda")
            crops_o = torch.randn((max(n_o, 1), 3, 48, 48), device="cuda")
            scales = fd.scale_pyramid(384, 512, 20, 0.709)

            def networks():
                with torch.no_grad():
                    for s in scales:
                        R.pnet(dev_state["pnet"], R.normalise(R.imresample(batch, R.pyramid_size(384, 512, s))))
                    for i in range(0, crops_r.shape[0], 512):
                        R.rnet(dev_state["rnet"], crops_r[i:i + 512])
                    for i in range(0, crops_o.shape[0], 512):
                        R.onet(dev_state["onet"], crops_o[i:i + 512])
            networks()
            networks()
            w = windows(networks, args.steps)
            base = {"what": "P-Net per scale on the whole batch, R-Net / O-Net on the same numbers of crops in chunks of 512; no NMS, "
                            "box arithmetic, crop cutting or host reads: a lower bound of the published implementation",
                    "rnet_crops": n_r, "onet_crops": n_o,
                    "images_per_s_min_max": [round(args.batch / max(w), 1), round(args.batch / min(w), 1)],
                    "ms_per_batch_min_max": [round(min(w) * 1e3, 2), round(max(w) * 1e3, 2)]}
            # the leg as the published implementation runs it: the whole restatement with its tensors on the device -- one image at a
            # time, one launch per scale, a host round trip per scale and stage, its own numpy NMS -- on a subset of the images
            sub = images[:args.restatement_images]
            R.detect(sub[:2], state, thresholds=thresholds, select_largest=False, device="cuda")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            R.detect(sub, state, thresholds=thresholds, select_largest=False, device="cuda")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            base["restatement_on_device"] = {"what": "tests/mtcnn_restatement.py detect() with device tensors, NMS as it has it (numpy)",
                                             "images": len(sub), "images_per_s": round(len(sub) / dt, 2), "windows": 1}
            out["hip_over_restatement_on_device"] = round(out["hip"]["images_per_s_min_max"][0] / (len(sub) / dt), 1)
            out["hip_over_torch_rocm_fp32_networks_only"] = round(base["ms_per_batch_min_max"][0] / out["hip"]["ms_per_batch_min_max"][0], 3)
        except Exception as e:  # noqa: BLE001 - torch-ROCm cannot run the convolutions here: record that instead of a ratio
            base["error"] = repr(e)
        out["torch_rocm_fp32"] = base
    out["library"] = _lib.load().mq_version().decode()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
