#!/usr/bin/env python3
"""ResNet-50 (viquae_amd.resnet.TorchvisionResNet, the `imagenet-RN50` encoder) forward throughput at 224 x 224: the HIP forward at
the shipped config's batch (256) and at the encoder's chunk, beside the same network (tests/resnet_restatement.py) run by torch-ROCm's
own fp32 convolutions on the same GPU (the faster of the default and the channels_last memory format, after warm-up), the ratio of
the two at batch 256, the executed matrix-pipe rate beside what the pipe sustains on random operands (bench.py's probe), and the
two routes of the stem.  Seeded weights, random pixels; one JSON line.

    python tools/resnet_timing.py [--batch 256] [--steps 10] [--no-baseline]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOL = {"Class_name": "AdaptiveMaxPool2d", "output_size": 1}


def network_macs(layers, size=224):
    """multiply-adds per image of every convolution: (total, {stem, 1x1, 3x3, downsample})"""
    from tests.resnet_restatement import EXPANSION, WIDTHS
    split = {"stem": (size // 2) ** 2 * 64 * 147, "1x1": 0, "3x3": 0, "downsample": 0}
    hw, cin = size // 4, 64
    for s, (n, width) in enumerate(zip(layers, WIDTHS), start=1):
        for i in range(n):
            out_hw = hw // 2 if (i == 0 and s > 1) else hw
            split["1x1"] += hw * hw * cin * width + out_hw * out_hw * width * width * EXPANSION
            split["3x3"] += out_hw * out_hw * 9 * width * width
            if i == 0:
                split["downsample"] += out_hw * out_hw * cin * width * EXPANSION
            hw, cin = out_hw, width * EXPANSION
    return sum(split.values()), split


def main():
    from bench import mfma_ceiling
    from tests import resnet_restatement as R
    from tools.bench_encoders import time_it
    from viquae_amd import _lib
    from viquae_amd.arcface import ArcFaceR50
    from viquae_amd.encoders import EPI_BIAS, gemm_nt, split_bf16_tiled
    from viquae_amd.resnet import TorchvisionResNet
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-baseline", action="store_true", help="skip the torch-ROCm forward (its first call may tune for minutes)")
    args = ap.parse_args()
    state = R.seeded_state(50)
    model = TorchvisionResNet.from_state_dict(state, pool_kwargs=POOL).cuda()
    g = torch.Generator(device="cuda").manual_seed(4)
    macs, split = network_macs(R.LAYERS)
    out = {"network": "resnet50 224x224, AdaptiveMaxPool2d(1)", "gmacs_per_image": round(macs / 1e9, 3),
           "mac_share": {k: round(v / macs, 4) for k, v in split.items()}, "hip": {}}
    with torch.no_grad():
        for batch in dict.fromkeys((args.batch, model.chunk)):
            px = torch.randn((batch, 3, 224, 224), generator=g, device="cuda")
            t = time_it(lambda: model(px), args.steps)
            out["hip"][f"batch_{batch}"] = {"images_per_s": round(batch / t, 1), "ms_per_forward": round(t * 1e3, 3),
                                            "executed_bf16_tflops": round(3 * 2 * (macs - split["stem"]) * batch / t / 1e12, 1)}
        px = torch.randn((args.batch, 3, 224, 224), generator=g, device="cuda")
        # the stem: the fused vector-ALU kernel against im2col (K = 147 -> 160) + the GEMM WITHOUT the max-pool pass that route
        # would still need (a lower bound of it)
        t_fused = time_it(lambda: model._stem(px), args.steps)
        w160 = torch.cat([model.conv1_w2, model.conv1_w2.new_zeros((64, 13))], dim=1).contiguous()
        ws = split_bf16_tiled(w160)

        def stem_gemm():
            A = ArcFaceR50._im2col(px, args.batch, 224, 224, 3, True, 7, 7, 2, 3, 160, None, None, None)
            return gemm_nt(A, w160, bias=model.conv1_b, epilogue=EPI_BIAS, wsplit=ws)
        t_gemm = time_it(stem_gemm, args.steps)
        out["stem"] = {"batch": args.batch, "fused_direct_ms": round(t_fused * 1e3, 3), "im2col_gemm_without_pool_ms": round(t_gemm * 1e3, 3)}
        torch.cuda.synchronize()
        out["sustained_mfma"] = mfma_ceiling(torch.device("cuda"), torch.cuda.current_stream(),
                                             out["hip"][f"batch_{args.batch}"]["executed_bf16_tflops"])
        if not args.no_baseline:
            base = {}
            try:
                torch.backends.cudnn.benchmark = True
                torch.backends.cuda.matmul.allow_tf32 = False
                torch.backends.cudnn.allow_tf32 = False
                dev_state = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in state.items()}
                for name, fmt in (("default", torch.contiguous_format), ("channels_last", torch.channels_last)):
                    st = {k: (v.contiguous(memory_format=fmt) if v.dim() == 4 else v) for k, v in dev_state.items()}
                    x = px.contiguous(memory_format=fmt)
                    fwd = lambda: F.adaptive_max_pool2d(R.features(st, x), 1)  # noqa: E731
                    t = time_it(fwd, args.steps, warmup=3)
                    base[name] = {"images_per_s": round(args.batch / t, 1), "ms_per_forward": round(t * 1e3, 3)}
                best = max(base.values(), key=lambda r: r["images_per_s"])
                base["best_images_per_s"] = best["images_per_s"]
                out["hip_over_torch_rocm_fp32"] = round(out["hip"][f"batch_{args.batch}"]["images_per_s"] / best["images_per_s"], 3)
                # the two forwards on the same pixels (the baseline is an fp32 forward: its own rounding is in the figure)
                out["max_abs_difference_of_the_two_forwards"] = float((model(px[:8]) - F.adaptive_max_pool2d(R.features(dev_state, px[:8]), 1)).abs().max())
            except Exception as e:  # noqa: BLE001 - torch-ROCm cannot run the convolutions here: record that instead of a ratio
                base["error"] = repr(e)
            out["torch_rocm_fp32"] = base
    out["library"] = _lib.load().mq_version().decode()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
