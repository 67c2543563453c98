"""torchvision's bottleneck ResNet (``resnet50`` / 101 / 152) on MI355X -- the encoder behind the ``imagenet-RN50`` column
(meerqat/image/embedding.py:68-83: the torchvision model cut before ``avgpool``, followed by ``nn.AdaptiveMaxPool2d(1)``).

The layout is :mod:`viquae_amd.arcface`'s: NHWC, every activation that only feeds convolutions is a split-bf16 (hi, lo) pair in PAIR
LAYOUT, every convolution a GEMM on the matrix pipe with three bf16 products per fp32 product (fp32-class accuracy: the reference
runs this model in fp32), the BatchNorm behind each convolution folded into its weights and bias at load, in float64.  A bottleneck
(torchvision v1.5: the stride sits on the 3 x 3) is three launches, four in a stage's first block:

    o1 = split(relu(conv1(P) + b1))                    # 1 x 1            mq_conv1x1_pair_f32
    o2 = split(relu(conv2(o1) + b2))                   # 3 x 3, stride s  mq_conv3x3_pair_f32 (a zero PReLU slope is ReLU)
    identity = downsample(P) + bd                      # 1 x 1, stride s  mq_conv1x1_pair_f32 on the same pair P, fp32 out
    y = relu(conv3(o2) + b3 + identity);  P' = split(y)   # 1 x 1: one epilogue writes the next shortcut and the next conv1's input

The shortcut stays fp32 (``y``), as in the face encoder: a pair keeps 16 significant bits, and a shortcut read back from it would be
rounded to 2^-17 relative once per block -- 16 roundings that add up along the identity path, up to 1.2e-4 of a feature of 30 = 3.7e-3
in the worst case against the 1e-3 this encoder is held to; kept in fp32 the identity path is exact and the only pair roundings are
those of the convolutions' operands, whose products are rounded at that level anyway.  It costs one more 4-byte stream per element of
the block outputs; ``y`` is not written where nothing reads it (the block in front of a downsample), and the last block writes only
``y``, which the pooled head reduces (``mq_pool_hw_f32``).  The stem (7 x 7 / 2, bn1, ReLU, max-pool 3 x 3 / 2) is one vector-ALU
kernel that writes the pooled pair and never the 112 x 112 x 64 tensor (``mq_stem_conv7x7_pool_f32``).

Weights come from a plain torchvision state dict on disk; nothing is ever fetched.  torchvision is not installed on the build machine
and neither are the ImageNet weights: parity is pinned against ``tests/resnet_restatement.py`` (the same network in
``torch.nn.functional`` calls, float64) on seeded weights, not against the published checkpoint."""
import os

import numpy as np
import torch

from . import _lib
from . import arcface as _arcface   # the module, not its names: arcface.py and this file both load while encoders.py is importing
from .encoders import HIP_CLASSES, SplitAct, _HipEncoder, _check_cuda, _stream, split_bf16_tiled

LAYERS = (3, 4, 6, 3)
POOL_MAX, POOL_MEAN = 0, 1   # MQ_POOL_MAX, MQ_POOL_MEAN (include/meerqat_hip.h)
_POOLS = {"AdaptiveMaxPool2d": POOL_MAX, "AdaptiveAvgPool2d": POOL_MEAN}


def fold_conv_bn(weight, bn):
    """A convolution's weight [Cout, Cin, k, k] and the eval-mode BatchNorm behind it, ``bn`` = (scale, shift) of
    :func:`viquae_amd.arcface._affine` -> float64 (W', b) with conv(x, W') + b == bn(conv(x, W))."""
    a, b = bn
    return np.asarray(weight, np.float64) * a[:, None, None, None], np.asarray(b, np.float64)


def _pool_mode(pool_kwargs):
    if pool_kwargs is None:
        raise TypeError("TorchvisionResNet needs pool_kwargs, e.g. {'Class_name': 'AdaptiveMaxPool2d', 'output_size': 1}")
    kw = dict(pool_kwargs)
    if "Class_name" not in kw:
        raise TypeError("pool_kwargs misses 'Class_name'")
    name, size = kw.pop("Class_name"), kw.pop("output_size", None)
    if isinstance(size, (list, tuple)):
        size = tuple(size)
    if name not in _POOLS or size not in (1, (1, 1)) or kw:
        raise NotImplementedError(f"pool_kwargs={pool_kwargs}: AdaptiveMaxPool2d / AdaptiveAvgPool2d with output_size 1 are provided")
    return _POOLS[name]


class TorchvisionResNet(_HipEncoder):
    """``model(pixel_values)`` -> fp32 [B, C, 1, 1] (C = 2048), the reference's shape; ``pixel_values`` fp32 [B, 3, H, W] on a GPU.

    H and W must be multiples of 32 (every stage then halves an even size, as at 224): such sizes are supported, 224 x 224 is the
    size the golden pins and 64 x 96 is tested on a small state; any other size raises ValueError.  Eval mode only."""

    def __init__(self, state, layers=LAYERS, pool_kwargs=None, chunk=328, groups=1, replace_stride_with_dilation=None):
        super().__init__()
        self.training = False
        self.pool_mode = _pool_mode(pool_kwargs)
        if groups != 1:
            raise NotImplementedError("grouped convolutions (ResNeXt) are not provided")
        if replace_stride_with_dilation is not None and any(replace_stride_with_dilation):
            raise NotImplementedError("dilated ResNets are not provided")
        # chunk = images per forward.  Coverage of the 256 CUs: the 14 x 14 3 x 3 convolutions (six blocks, the largest share) run
        # ceil(B * 196 / 256) workgroups of one 256 x 256 tile and the 7 x 7 ones ceil(B * 49 / 256) * 4 of 256 x 128: 328 images
        # give 252 of 256 in both (256 images: 196); the 56 x 56 stage has 3136 rows per image and covers at any batch.  Memory:
        # the forward is widest in layer1, where the block input (pair + fp32 shortcut), o1, o2 and the block output (pair + fp32)
        # are live: 3136 pixels x (256 x 8 + 64 x 4 x 2 + 256 x 8) bytes = 14.5 MB per image, 3.7 GB at 256 images, 4.7 GB at 328.
        # Buffers go back to torch's caching allocator as the walk drops them, so every later block reuses layer1's memory.
        state = {(k[7:] if k.startswith("module.") else k): v for k, v in state.items()}   # the reference's Places365 note
        state = {k: _arcface._np(v) for k, v in state.items() if not k.endswith("num_batches_tracked") and not k.startswith("fc.")}
        self.layers, self.chunk = tuple(int(n) for n in layers), int(chunk)
        if len(self.layers) != 4 or min(self.layers) < 1:
            raise ValueError(f"layers={layers}: four stage depths are expected")
        if "layer1.0.conv3.weight" not in state:
            raise NotImplementedError("BasicBlock ResNets (resnet18 / 34: no conv3 in the blocks) are not provided")
        for s, n in enumerate(self.layers, start=1):
            if f"layer{s}.{n - 1}.conv1.weight" not in state or f"layer{s}.{n}.conv1.weight" in state:
                raise ValueError(f"the state dict does not have layers={self.layers} blocks (stage {s})")
        self._geom = {}
        conv = lambda name, bn, k, stride: self._fold(state, name, bn, k, stride)  # noqa: E731

        if state["conv1.weight"].shape != (64, 3, 7, 7):
            raise ValueError(f"conv1.weight: expected [64, 3, 7, 7], got {state['conv1.weight'].shape}")
        conv("conv1", "bn1", 7, 2)
        # the stem as a direct convolution (mq_stem_conv7x7_pool_f32): weights [147, 64], row (kh * 7 + kw) * 3 + c
        self._reg("conv1.wt", self.conv1_w2.T.contiguous())
        cin = 64
        for s, n in enumerate(self.layers, start=1):
            for i in range(n):
                p = f"layer{s}.{i}"
                stride = 2 if (i == 0 and s > 1) else 1
                width = state[p + ".conv1.weight"].shape[0]
                if state[p + ".conv2.weight"].shape[1] != width:
                    raise NotImplementedError(f"{p}.conv2 is a grouped convolution (ResNeXt): not provided")
                if state[p + ".conv1.weight"].shape[1] != cin or width % 64:
                    raise ValueError(f"{p}.conv1.weight {state[p + '.conv1.weight'].shape}: expected {cin} input channels, a multiple of 64 outputs")
                conv(p + ".conv1", p + ".bn1", 1, 1)
                conv(p + ".conv2", p + ".bn2", 3, stride)
                conv(p + ".conv3", p + ".bn3", 1, 1)
                if (p + ".downsample.0.weight") in state:
                    conv(p + ".downsample.0", p + ".downsample.1", 1, stride)
                elif stride != 1 or cin != self._geom[p + ".conv3"][0]:
                    raise ValueError(f"{p}: the block changes shape but the state dict has no downsample")
                cin = self._geom[p + ".conv3"][0]
        self.num_features = cin
        self._reg("relu_slope", torch.zeros(max(g[0] for g in self._geom.values())))   # PReLU with slope 0: the 3 x 3's ReLU

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_state_dict(cls, state, **kw):
        """``state``: a torchvision ResNet state dict (``conv1``, ``bn1``, ``layerS.I.{conv1,bn1,conv2,bn2,conv3,bn3,downsample.0,
        downsample.1}``; ``fc.*`` and ``num_batches_tracked`` are ignored, a leading ``module.`` is stripped).  ``kw``: ``layers``
        ((3, 4, 6, 3) = resnet50, (3, 4, 23, 3) = resnet101, (3, 8, 36, 3) = resnet152), ``pool_kwargs``, ``chunk``."""
        return cls(state, **kw)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, **kw):
        """A state-dict FILE, e.g. ``torch.save(torchvision.models.resnet50(weights=...).state_dict(), path)`` made where torchvision
        and the weights exist.  Never downloads: a path that does not exist is a FileNotFoundError."""
        path = os.fspath(pretrained_model_name_or_path)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: no such state-dict file (TorchvisionResNet loads local weights only)")
        return cls(torch.load(path, map_location="cpu", weights_only=True), **kw)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError(f"{type(self).__name__} is an inference encoder: BatchNorms are folded, eval mode only")
        return super().train(False)

    def _fold(self, state, name, bn, k, stride, pad_out=0, pad_in=0):
        """Registers convolution ``name`` with the BatchNorm ``bn`` behind it folded in (float64): ``.w2`` fp32 [Cout, k k Cin] with
        (kh, kw, c) columns, ``.b`` fp32 [Cout], and its geometry.  ``pad_out`` / ``pad_in``: output / input channels of zeros added
        (a padded output channel is relu(0) = 0, a padded input channel multiplies it by 0)."""
        w = state[name + ".weight"]
        if w.ndim != 4 or w.shape[2] != k or w.shape[3] != k:
            raise ValueError(f"{name}.weight: expected a {k} x {k} kernel, got {w.shape}")
        w64, b64 = fold_conv_bn(w, _arcface._affine(state, bn))
        w64, b64 = np.pad(w64, ((0, pad_out), (0, pad_in), (0, 0), (0, 0))), np.pad(b64, (0, pad_out))
        cout, cin = w64.shape[:2]
        self._geom[name] = (cout, cin, k, stride)
        self._reg(name + ".w2", torch.from_numpy(w64.transpose(0, 2, 3, 1).reshape(cout, -1).astype(np.float32)))   # (kh, kw, c)
        self._reg(name + ".b", torch.from_numpy(b64.astype(np.float32)))

    # ------------------------------------------------------------------ kernels
    def _b(self, name):
        return getattr(self, name.replace(".", "_"))

    def _zeros(self, dev):
        zeros = self.__dict__.setdefault("_zero_pages", {})
        if dev not in zeros:
            zeros[dev] = torch.zeros(64, dtype=torch.uint8, device=dev)
        return zeros[dev]

    def _wsplit(self, name):
        w = self._b(name)
        cache = self.__dict__.setdefault("_split_cache", {})
        key = (name, w.device, w.data_ptr())
        if key not in cache:
            cache[key] = split_bf16_tiled(w)
        return cache[key]

    def _stem(self, x):
        """-> the pooled stem output as a pair [B * H/4 * W/4, 64]"""
        B, _, H, W = x.shape
        P = SplitAct.empty(B * (H // 4) * (W // 4), 64, x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().mq_stem_conv7x7_pool_f32(x.data_ptr(), B, H, W, self.conv1_wt.data_ptr(), self.conv1_b.data_ptr(),
                                                            P.hi.data_ptr(), P.lo.data_ptr(), _stream(x)), "mq_stem_conv7x7_pool_f32")
        return P

    def _conv1x1(self, name, xin, B, H, W, residual=None, relu=True, want_y=False, want_pair=True, tile=0):
        """1 x 1 convolution ``name`` on the pair ``xin`` [B * H * W, Cin] -> (Y fp32 or None, P pair or None), Ho, Wo; ``tile``: MQ_CONV_TILE_* (0 = AUTO)"""
        cout, cin, _, stride = self._geom[name]
        assert xin.shape == (B * H * W, cin)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        M, dev = B * Ho * Wo, xin.device
        Y = torch.empty((M, cout), dtype=torch.float32, device=dev) if want_y else None
        P = SplitAct.empty(M, cout, dev) if want_pair else None
        wh, wl = self._wsplit(name + ".w2")
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mq_conv1x1_pair_f32(xin.hi.data_ptr(), xin.lo.data_ptr(), B, H, W, cin, stride, wh.data_ptr(),
                                                       wl.data_ptr(), cout, self._b(name + ".b").data_ptr(), p(residual), int(relu), p(Y),
                                                       P.hi.data_ptr() if P is not None else None,
                                                       P.lo.data_ptr() if P is not None else None, self._zeros(dev).data_ptr(), tile,
                                                       _stream(xin.hi)), "mq_conv1x1_pair_f32")
        return (Y, P), Ho, Wo

    def _conv3x3(self, name, xin, B, H, W):
        """split(relu(conv3x3 + bias)) of the pair ``xin`` -> pair, Ho, Wo"""
        cout, cin, _, stride = self._geom[name]
        assert xin.shape == (B * H * W, cin)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        P = SplitAct.empty(B * Ho * Wo, cout, xin.device)
        wh, wl = self._wsplit(name + ".w2")
        with torch.cuda.device(xin.device):
            _lib.check(_lib.load().mq_conv3x3_pair_f32(xin.hi.data_ptr(), xin.lo.data_ptr(), B, H, W, cin, stride, wh.data_ptr(),
                                                       wl.data_ptr(), cout, self._b(name + ".b").data_ptr(), self.relu_slope.data_ptr(),
                                                       None, None, None, None, P.hi.data_ptr(), P.lo.data_ptr(),
                                                       self._zeros(xin.device).data_ptr(), _arcface.CONV_TILE_AUTO | _arcface.CONV_K_CHANNEL_MAJOR,
                                                       _stream(xin.hi)), "mq_conv3x3_pair_f32")
        return P, Ho, Wo

    def _pool(self, y, B, HW):
        out = torch.empty((B, y.shape[1]), dtype=torch.float32, device=y.device)
        with torch.cuda.device(y.device):
            _lib.check(_lib.load().mq_pool_hw_f32(y.data_ptr(), B, HW, y.shape[1], self.pool_mode, out.data_ptr(), _stream(y)),
                       "mq_pool_hw_f32")
        return out

    # ------------------------------------------------------------------ forward
    def forward(self, pixel_values):
        _check_cuda(pixel_values)
        x = pixel_values.to(torch.float32).contiguous()
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 32 or x.shape[3] % 32 or 0 in x.shape[2:]:
            raise ValueError(f"expected [B, 3, H, W] pixel values with H and W multiples of 32, got {tuple(x.shape)}")
        if x.shape[0] > self.chunk:
            out = torch.cat([self._forward(x[s:s + self.chunk]) for s in range(0, x.shape[0], self.chunk)])
        else:
            out = self._forward(x)
        return out.view(x.shape[0], self.num_features, 1, 1)

    _avgpooled = frozenset()   # blocks whose stride is an AvgPool2d(2) (openai-clip's ModifiedResNet, clip_resnet.py); none here

    def _avgpool(self, xin, B, H, W):
        raise NotImplementedError

    def bottleneck(self, p, xin, y, B, H, W, want_y=True, want_pair=True):
        """One block ``p`` on its input pair ``xin`` (and fp32 shortcut ``y``, unused when the block has a downsample) -> (y', pair',
        Ho, Wo).  openai-clip's ModifiedResNet walks the same block: its strided blocks (``_avgpooled``) keep every convolution at
        stride 1 and average-pool 2 x 2 in front of conv3 and of the shortcut's 1 x 1."""
        (_, o1), _, _ = self._conv1x1(p + ".conv1", xin, B, H, W)
        o2, Ho, Wo = self._conv3x3(p + ".conv2", o1, B, H, W)
        if p in self._avgpooled:
            o2, xin = self._avgpool(o2, B, Ho, Wo), self._avgpool(xin, B, H, W)
            H, W, Ho, Wo = H // 2, W // 2, Ho // 2, Wo // 2
        if (p + ".downsample.0") in self._geom:
            (y, _), _, _ = self._conv1x1(p + ".downsample.0", xin, B, H, W, relu=False, want_y=True, want_pair=False)
        (y, xin), _, _ = self._conv1x1(p + ".conv3", o2, B, Ho, Wo, residual=y, want_y=want_y, want_pair=want_pair)
        return y, xin, Ho, Wo

    def _stages(self, xin, B, H, W):
        """the four stages on the stem's output pair ``xin`` [B * H * W, C] -> (the last block's fp32 output, H', W')"""
        blocks = [f"layer{s}.{i}" for s, n in enumerate(self.layers, start=1) for i in range(n)]
        y = None
        for bi, p in enumerate(blocks):
            last = bi + 1 == len(blocks)
            # the fp32 output is the NEXT block's shortcut (not read when that block has a downsample) or the pooled head's input
            reads_y = last or (blocks[bi + 1] + ".downsample.0") not in self._geom
            y, xin, H, W = self.bottleneck(p, xin, y, B, H, W, want_y=reads_y, want_pair=not last)
        return y, H, W

    def _forward(self, x):
        B, H, W = x.shape[0], x.shape[2] // 4, x.shape[3] // 4
        y, H, W = self._stages(self._stem(x), B, H, W)
        return self._pool(y, B, H * W)


HIP_CLASSES["TorchvisionResNet"] = TorchvisionResNet
