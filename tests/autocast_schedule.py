"""A torch-CPU statement of the rounding points of arcface_torch's fp16 autocast forward (``get_model('r50', fp16=True)``:
everything up to ``flatten`` under ``torch.cuda.amp.autocast``, ``fc`` and ``features`` on ``x.float()``), written from this table:

    conv2d (stem, 3 x 3, 1 x 1)   input and UNFOLDED weight rounded to fp16; wide accumulation   -> rounded to fp16
    BatchNorm (eval)              fp16 tensor, fp32 statistics                                   -> rounded to fp16
    PReLU                         fp16 tensor, slope rounded to fp16                             -> rounded to fp16
    residual add                  fp16 + fp16                                                    -> rounded to fp16
    bn2 -> flatten                fp16, then .float(); fc, features in fp32

``r`` rounds to fp16 (nearest even, overflow to +-inf) and returns the working dtype.  ``forward`` computes every operation in
float64 and rounds its result to ``dtype`` before fp16: float32 is correctly rounded fp32 between the roundings, as the golden
file's ``embeddings_fp16_autocast`` was made -- the same bits on every CPU, where torch's own fp32 convolutions and BatchNorms
sum and fuse differently per instruction set and one flipped fp16 rounding cascades through 50 layers; float64 puts exact
arithmetic between the same roundings (the per-kernel pins of tests/test_arcface_fp16_gpu.py)."""
import numpy as np
import torch
import torch.nn.functional as F

STAGES = ((3, 64), (4, 128), (14, 256), (3, 512))


def r(t):
    return t.to(torch.float16).to(t.dtype)


def affine(t, scale, shift):
    """an eval-mode BatchNorm given as per-channel (scale, shift) on the LAST axis (NHWC), rounded"""
    return r(t * scale + shift)


def prelu(t, slope):
    """PReLU with the slope rounded to fp16, on the last axis, rounded"""
    s = r(slope)
    return r(torch.where(t >= 0, t, t * s))


def conv_nhwc(x, w, stride, pad):
    """x [B, H, W, C] (already fp16 values), w [N, C, k, k] -> r(conv) [B, Ho, Wo, N] with r(w), wide accumulation"""
    y = F.conv2d(x.permute(0, 3, 1, 2), r(w), None, stride=stride, padding=pad)
    return r(y.permute(0, 2, 3, 1))


def ulp16(v):
    """the spacing of fp16 at |v| (2^-24 below the normal range), as float64"""
    a = np.abs(np.asarray(v, np.float64))
    a = np.where(np.isfinite(a), np.minimum(a, 65504.0), 65504.0)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def forward(state, x, dtype=torch.float32):
    """IResNet-50 eval forward at the autocast rounding points; state: checkpoint-layout dict of tensors, x: [B, 3, 112, 112];
    every operation in float64, its result rounded to ``dtype`` (then to fp16 in the backbone)"""
    st = {k: v.to(torch.float64) for k, v in state.items()}
    x = x.to(torch.float64)

    def q(t):
        return t.to(dtype).to(torch.float64)

    def norm(t, name):
        return r(q(F.batch_norm(t, st[name + ".running_mean"], st[name + ".running_var"], st[name + ".weight"], st[name + ".bias"],
                                training=False, momentum=0.0, eps=1e-5)))

    def conv(t, name, stride, padding):
        return r(q(F.conv2d(t, r(st[name + ".weight"]), None, stride=stride, padding=padding)))

    def act(t, name):
        return r(q(F.prelu(t, r(st[name + ".weight"]))))

    t = act(norm(conv(r(x), "conv1", 1, 1), "bn1"), "prelu")
    for s, (blocks, _) in enumerate(STAGES, start=1):
        for b in range(blocks):
            p = f"layer{s}.{b}"
            stride = 2 if b == 0 else 1
            u = conv(norm(t, p + ".bn1"), p + ".conv1", 1, 1)
            u = act(norm(u, p + ".bn2"), p + ".prelu")
            u = norm(conv(u, p + ".conv2", stride, 1), p + ".bn3")
            if b == 0:
                t = norm(conv(t, p + ".downsample.0", stride, 0), p + ".downsample.1")
            t = r(q(u + t))
    t = torch.flatten(norm(t, "bn2"), 1)
    t = q(F.linear(t, st["fc.weight"], st["fc.bias"]))
    return F.batch_norm(t, st["features.running_mean"], st["features.running_var"], st["features.weight"], st["features.bias"],
                        training=False, momentum=0.0, eps=1e-5).to(dtype)
