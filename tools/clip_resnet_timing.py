#!/usr/bin/env python3
"""CLIP RN50 (viquae_amd.clip_resnet.CLIPModifiedResNet, the `clip-RN50` encoder) forward throughput at 224 x 224: the HIP forward at
the shipped config's batch (2048, walked in the encoder's chunks) and at one chunk, beside the same network
(tests/clip_resnet_restatement.py) run by torch-ROCm's own convolutions on the same GPU in the same run -- fp32 in the channels_last
memory format, and fp16 (the precision the reference itself runs this model in) -- at the chunk's batch; the ratios at that batch;
and, for the two memory-bound kernels this encoder adds (the 2 x 2 average pool on a pair and the attention pool's tokens), the
bytes they must move over their time as a fraction of the HBM peak.  Seeded weights, random pixels; one JSON line.  Each figure is
the median of `--repeats` windows of `--steps` forwards after warm-up, with the spread (min, max) beside it.

    python tools/clip_resnet_timing.py [--batch 2048] [--steps 5] [--repeats 5] [--no-baseline]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK, HBM_MEASURED = 8.0e12, 6.29e12   # bytes/s: the datasheet figure and a float4 copy on the MI355X


def network_macs(layers, size=224, width=64, output_dim=1024):
    """multiply-adds per image: (total, {stem, 1x1, 3x3, downsample, attnpool})"""
    h = size // 2
    split = {"stem": h * h * (27 * width // 2 + 9 * (width // 2) ** 2 + 9 * width * width // 2), "1x1": 0, "3x3": 0, "downsample": 0}
    hw, cin = size // 4, width
    for s, n in enumerate(layers, start=1):
        planes = width * 2 ** (s - 1)
        for i in range(n):
            out_hw = hw // 2 if (i == 0 and s > 1) else hw
            split["1x1"] += hw * hw * cin * planes + out_hw * out_hw * planes * planes * 4
            split["3x3"] += hw * hw * 9 * planes * planes           # un-strided: the pool comes after it
            if i == 0:
                split["downsample"] += out_hw * out_hw * cin * planes * 4
            hw, cin = out_hw, planes * 4
    T = hw * hw + 1
    split["attnpool"] = T * cin * 2 * cin + cin * cin + 2 * T * cin + cin * output_dim
    return sum(split.values()), split


def progress(what):
    print(what, file=sys.stderr, flush=True)


def windows(fn, steps, repeats, warmup=3):
    from tools.bench_encoders import time_it
    time_it(fn, warmup, warmup=1)
    ts = sorted(time_it(fn, steps, warmup=0) for _ in range(repeats))
    return statistics.median(ts), ts[0], ts[-1]


def rate(batch, t):
    med, lo, hi = t
    return {"images_per_s": round(batch / med, 1), "ms_per_forward": round(med * 1e3, 3),
            "images_per_s_min_max": [round(batch / hi, 1), round(batch / lo, 1)]}


def main():
    from tests import clip_resnet_restatement as R
    from viquae_amd import _lib
    from viquae_amd.clip_resnet import CLIPModifiedResNet
    from viquae_amd.encoders import SplitAct
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true", help="skip the torch-ROCm forwards (their first call may tune for minutes)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_resnet_timing.py measures on the GPU: no GPU visible")
    state = R.seeded_state(7)
    model = CLIPModifiedResNet.from_state_dict(state).cuda()
    chunk = model.chunk
    g = torch.Generator(device="cuda").manual_seed(4)
    macs, split = network_macs(R.LAYERS)
    out = {"network": "clip RN50 224x224 (ModifiedResNet (3, 4, 6, 3) + AttentionPool2d)", "gmacs_per_image": round(macs / 1e9, 3),
           "mac_share": {k: round(v / macs, 4) for k, v in split.items()}, "chunk": chunk, "steps": args.steps, "repeats": args.repeats,
           "hip": {}}
    with torch.no_grad():
        for batch in dict.fromkeys((args.batch, chunk)):
            px = torch.randn((batch, 3, 224, 224), generator=g, device="cuda")
            t = windows(lambda: model(px), args.steps if batch <= chunk else max(1, args.steps // 2), args.repeats)
            progress(f"hip forward, batch {batch}: done")
            out["hip"][f"batch_{batch}"] = dict(rate(batch, t), useful_tflops=round(2 * macs * batch / t[0] / 1e12, 1))   # 2 x the network's multiply-adds
            del px
        # the two memory-bound kernels at the chunk's batch: the bytes they must move (each pair element is 2 + 2 bytes)
        mem = {}
        for name, (H, C) in {"avgpool_stem_112x112x64": (112, 64), "avgpool_layer2_56x56x256": (56, 256), "avgpool_layer4_14x14x1024": (14, 1024)}.items():
            X = SplitAct.empty(chunk * H * H, C, "cuda")
            X.hi.zero_(), X.lo.zero_()
            t = windows(lambda: model._avgpool(X, chunk, H, H), 20, args.repeats)
            nbytes = chunk * H * H * C * 4 * 1.25
            mem[name] = {"us": round(t[0] * 1e6, 1), "gb": round(nbytes / 1e9, 3), "fraction_of_hbm_peak": round(nbytes / t[0] / HBM_PEAK, 3),
                         "fraction_of_measured_copy_rate": round(nbytes / t[0] / HBM_MEASURED, 3)}
            del X
        y = torch.randn((chunk * 49, 2048), generator=g, device="cuda")
        tok, mean = SplitAct.empty(chunk * 50, 2048, "cuda"), SplitAct.empty(chunk, 2048, "cuda")
        lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream

        def tokens():
            _lib.check(lib.mq_attnpool_tokens_f32(y.data_ptr(), chunk, 49, 2048, model.pos.data_ptr(), tok.hi.data_ptr(), tok.lo.data_ptr(),
                                                  mean.hi.data_ptr(), mean.lo.data_ptr(), stream), "mq_attnpool_tokens_f32")
        t = windows(tokens, 20, args.repeats)
        nbytes = chunk * 2048 * (49 * 4 + 51 * 4)
        mem["attnpool_tokens_49x2048"] = {"us": round(t[0] * 1e6, 1), "gb": round(nbytes / 1e9, 3),
                                          "fraction_of_hbm_peak": round(nbytes / t[0] / HBM_PEAK, 3),
                                          "fraction_of_measured_copy_rate": round(nbytes / t[0] / HBM_MEASURED, 3)}
        out["memory_bound_kernels_at_chunk"] = mem
        progress("memory-bound kernels: done")
        del y, tok, mean
        if not args.no_baseline:
            base = {}
            try:
                torch.backends.cudnn.benchmark = True
                torch.backends.cuda.matmul.allow_tf32 = False
                torch.backends.cudnn.allow_tf32 = False
                px = torch.randn((chunk, 3, 224, 224), generator=g, device="cuda")
                for name, dtype in (("fp32_channels_last", torch.float32), ("fp16_channels_last", torch.float16)):
                    st = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in state.items()}
                    st = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in st.items()}
                    st = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in st.items()}
                    x = px.to(dtype).contiguous(memory_format=torch.channels_last)
                    fwd = lambda: R.attention_pool(st, R.features(st, x))  # noqa: E731
                    base[name] = rate(chunk, windows(fwd, args.steps, args.repeats))
                    progress(f"torch-ROCm {name}: done")
                    base[name]["max_abs_difference_from_the_hip_forward_8_images"] = float((model(px[:8]) - R.attention_pool(st, R.features(st, x[:8])).float()).abs().max())
                hip = out["hip"][f"batch_{chunk}"]["images_per_s"]
                out["hip_over_torch_rocm_fp32"] = round(hip / base["fp32_channels_last"]["images_per_s"], 3)
                out["hip_over_torch_rocm_fp16"] = round(hip / base["fp16_channels_last"]["images_per_s"], 3)
            except Exception as e:  # noqa: BLE001 - torch-ROCm cannot run the network here: record that instead of a ratio
                base["error"] = repr(e)
            out["torch_rocm_at_chunk"] = base
    out["library"] = _lib.load().mq_version().decode()
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
