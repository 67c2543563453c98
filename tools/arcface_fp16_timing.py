#!/usr/bin/env python3
"""ArcFace r50 forward throughput at both precisions, 656 faces per forward (the encoder's chunk): the default fp32-class path and
the opt-in fp16 path (ArcFaceR50(precision="fp16"), the reference's autocast precision).  Same random weights and pixels as
tools/bench_encoders.arcface_throughput; one JSON line.

    python tools/arcface_fp16_timing.py [--batch 656] [--steps 10]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tools.bench_encoders import random_arcface_state, time_it
    from viquae_amd.arcface import ArcFaceR50
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=656)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    state = random_arcface_state(0)
    g = torch.Generator(device="cuda").manual_seed(4)
    px = torch.rand((args.batch, 3, 112, 112), generator=g, device="cuda") * 2 - 1
    out = {"batch": args.batch}
    with torch.no_grad():
        for precision in ("fp32", "fp16"):
            model = ArcFaceR50.from_state_dict(state, precision=precision).cuda().eval()
            t = time_it(lambda: model(px), args.steps)
            out[precision] = {"faces_per_s": round(args.batch / t, 1), "ms_per_forward": round(t * 1e3, 3)}
            del model
    out["fp16_over_fp32"] = round(out["fp16"]["faces_per_s"] / out["fp32"]["faces_per_s"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
