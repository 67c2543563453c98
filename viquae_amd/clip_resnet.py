"""openai-clip's ``ModifiedResNet`` (``clip.load("RN50")``'s visual tower; RN101 with ``layers=(3, 4, 23, 3)``) on MI355X -- the encoder
behind the ``clip-RN50`` column (meerqat/image/embedding.py: ``"type": "clip", "name": "RN50"``; the model is written here from the
published architecture, the ``clip`` package is not needed).

It is :class:`viquae_amd.resnet.TorchvisionResNet`'s walk -- NHWC, split-bf16 (hi, lo) pair activations, every convolution a GEMM on the
matrix pipe with three bf16 products per fp32 product, BatchNorms folded in float64 at load, the shortcut kept in fp32 beside the pair
for the reasons given there -- with the four differences of the architecture:

* the stem is three 3 x 3 convolutions (3 -> w/2 at stride 2, w/2 -> w/2, w/2 -> w; BatchNorm + ReLU each) and ``AvgPool2d(2)``: the
  first on the vector ALU (``mq_clip_stem_conv3x3s2_f32``, K = 27), the other two ``mq_conv3x3_pair_f32``.  The 32-channel ``conv2``
  is loaded with 32 output channels of zeros (and ``conv3`` with the matching input columns of zeros): that kernel takes multiples of
  64 output channels, relu(0 + 0) = 0 and 0 times anything adds an exact 0 to the sums;
* a strided block keeps its convolutions at stride 1 and pools 2 x 2 between ``relu(bn2(conv2))`` and ``conv3`` and in front of the
  shortcut's 1 x 1 (``mq_avgpool2x2_pair_f32``; the hook is in :meth:`TorchvisionResNet.bottleneck`, the block is stated once);
* the head is ``AttentionPool2d``: tokens = [mean | the H W / 32^2 pixels] + positional embedding (``mq_attnpool_tokens_f32``),
  ``[k_proj; v_proj]`` as ONE GEMM over the tokens, ``q_proj`` over the mean tokens only, attention with that one query per image
  (``mq_attention_single_query_f32``), ``c_proj``;
* the checkpoint stores convolution and linear weights in fp16 (upcast exactly here) under a ``visual.`` prefix.

The reference runs this model in fp16 on a GPU (``clip.load`` keeps the fp16 weights on CUDA); this is the fp32-class path.  Weights
come from a local file; nothing is ever fetched.  Neither ``clip`` nor its weights exist where this is built: parity is pinned against
``tests/clip_resnet_restatement.py`` (the same network in ``torch.nn.functional`` calls, float64) on seeded weights, NOT against the
published checkpoint."""
import math
import os
import warnings

import torch

from . import _lib
from . import arcface as _arcface
from .encoders import EPI_BIAS, HIP_CLASSES, SplitAct, _HipEncoder, _check_cuda, _stream, gemm_nt
from .resnet import LAYERS, TorchvisionResNet

HEAD_DIM = 64   # mq_attention_single_query_f32: a lane per dimension


def visual_state(state):
    """The visual tower's tensors of a CLIP state dict, as numpy arrays under ModifiedResNet's own names: a leading ``module.`` and /
    or ``visual.`` is stripped; when any key carries ``visual.`` (a full CLIP state dict) every other key -- the text tower, the
    top-level ``positional_embedding``, ``logit_scale`` -- is dropped.  fp16 tensors stay fp16 here; every consumer widens them
    exactly (to float64 for the fold, to fp32 for the linear layers)."""
    state = {(k[7:] if k.startswith("module.") else k): v for k, v in state.items()}
    if any(k.startswith("visual.") for k in state):
        state = {k[7:]: v for k, v in state.items() if k.startswith("visual.")}
    return {k: _arcface._np(v) for k, v in state.items() if not k.endswith("num_batches_tracked")}


class CLIPModifiedResNet(TorchvisionResNet):
    """``model(pixel_values)`` -> fp32 [B, output_dim] (1024 for RN50); ``pixel_values`` fp32 [B, 3, S, S] on a GPU, S = 32 x the
    attention pool's ``spacial_dim`` (224 for the published RN50 / RN101).  Eval mode only."""

    def __init__(self, state, layers=LAYERS, heads=None, chunk=328):
        _HipEncoder.__init__(self)
        self.training = False
        # chunk = images per forward: resnet.py's figure holds.  Coverage of the 256 CUs: the dominant launches are again the 3 x 3
        # convolutions at 14 x 14 -- layer3's six (N = 256: ceil(B * 196 / 256) tiles of 256 x 256) and, here, layer4.0's un-strided
        # one (N = 512: twice as many) -- and layer4's at 7 x 7 (ceil(B * 49 / 256) * 4 tiles of 256 x 128): 328 images give 252
        # workgroups (504 = two rounds of 252 for layer4.0) of 256 in all of them; the un-strided 3 x 3s at 56 x 56 and 28 x 28
        # (layer2.0, layer3.0) and the stem's 112 x 112 ones have 3136 ... 12544 rows per image and cover at any batch.  Memory: the
        # stem's widest moment is conv2's and conv3's outputs together, 12544 pixels x 64 channels x 4 bytes x 2 = 6.4 MB per image,
        # and a strided block holds its un-pooled and pooled tensors together (layer2.0: 3136 x (256 + 128 + 128) x 4 + 784 x (256 +
        # 128 + 512) x 4 + the output 784 x 512 x 8 = 12.4 MB); both stay under layer1's 14.5 MB per image (block input and output as pair +
        # fp32 shortcut, o1, o2: resnet.py), so 328 images are 4.7 GB.  The head adds 50 x (2048 x 4 + 4096 x 4) + 49 x 2048 x 4 bytes
        # = 1.6 MB per image after the trunk's buffers went back to the allocator.
        state = visual_state(state)
        self.layers, self.chunk = tuple(int(n) for n in layers), int(chunk)
        if len(self.layers) != 4 or min(self.layers) < 1:
            raise ValueError(f"layers={layers}: four stage depths are expected")
        if "attnpool.positional_embedding" not in state:
            raise NotImplementedError("the state dict has no attnpool.*: not a CLIP ModifiedResNet (the ViT towers are CLIPModel's)")
        for s, n in enumerate(self.layers, start=1):
            if f"layer{s}.{n - 1}.conv1.weight" not in state or f"layer{s}.{n}.conv1.weight" in state:
                raise ValueError(f"the state dict does not have layers={self.layers} blocks (stage {s})")
        width = state["layer1.0.conv1.weight"].shape[0]
        if width % 64:
            raise NotImplementedError(f"width {width}: widths that are multiples of 64 are provided (RN50, RN101; not RN50x4 / x16)")
        if width != 64:
            raise NotImplementedError(f"width {width}: the stem kernel makes 32 channels (RN50, RN101; not RN50x64)")
        half = width // 2
        for name, shape in (("conv1", (half, 3, 3, 3)), ("conv2", (half, half, 3, 3)), ("conv3", (width, half, 3, 3))):
            if state[name + ".weight"].shape != shape:
                raise ValueError(f"{name}.weight: expected {list(shape)}, got {list(state[name + '.weight'].shape)}")
        self._geom = {}
        self._fold(state, "conv1", "bn1", 3, 2)
        self._reg("conv1.wt", self.conv1_w2.T.contiguous())   # mq_clip_stem_conv3x3s2_f32: [27, 32], row (kh * 3 + kw) * 3 + c
        self._fold(state, "conv2", "bn2", 3, 1, pad_out=64 - half)
        self._fold(state, "conv3", "bn3", 3, 1, pad_in=64 - half)
        cin, pooled = width, set()
        for s, n in enumerate(self.layers, start=1):
            for i in range(n):
                p = f"layer{s}.{i}"
                w = state[p + ".conv1.weight"].shape[0]
                if state[p + ".conv1.weight"].shape[1] != cin or w % 64 or state[p + ".conv2.weight"].shape[1] != w:
                    raise ValueError(f"{p}.conv1 / conv2 weights {state[p + '.conv1.weight'].shape}, {state[p + '.conv2.weight'].shape}: "
                                     f"expected {cin} input channels and a multiple of 64 outputs")
                for c, k in (("1", 1), ("2", 3), ("3", 1)):
                    self._fold(state, f"{p}.conv{c}", f"{p}.bn{c}", k, 1)   # every convolution at stride 1: the stride is a pool
                if i == 0 and s > 1:
                    pooled.add(p)
                if (p + ".downsample.0.weight") in state:
                    self._fold(state, p + ".downsample.0", p + ".downsample.1", 1, 1)
                elif p in pooled or cin != self._geom[p + ".conv3"][0]:
                    raise ValueError(f"{p}: the block changes shape but the state dict has no downsample")
                cin = self._geom[p + ".conv3"][0]
        self._avgpooled = frozenset(pooled)
        self.num_features = cin
        self._reg("relu_slope", torch.zeros(max(g[0] for g in self._geom.values())))   # PReLU with slope 0: the 3 x 3's ReLU
        # AttentionPool2d
        pos = state["attnpool.positional_embedding"]
        self.spacial_dim = math.isqrt(pos.shape[0] - 1)
        if self.spacial_dim ** 2 + 1 != pos.shape[0] or pos.shape[1] != cin:
            raise ValueError(f"attnpool.positional_embedding {list(pos.shape)}: expected [s * s + 1, {cin}]")
        self.heads = int(heads) if heads is not None else cin // HEAD_DIM
        if self.heads * HEAD_DIM != cin:
            raise NotImplementedError(f"{self.heads} heads over {cin} channels: a head size of {HEAD_DIM} is provided")
        self.input_resolution = 32 * self.spacial_dim
        lin = lambda n: (state[f"attnpool.{n}.weight"], state[f"attnpool.{n}.bias"])  # noqa: E731
        for n in ("q_proj", "k_proj", "v_proj"):
            if lin(n)[0].shape != (cin, cin):
                raise ValueError(f"attnpool.{n}.weight: expected [{cin}, {cin}], got {list(lin(n)[0].shape)}")
        self.output_dim = lin("c_proj")[0].shape[0]
        if lin("c_proj")[0].shape[1] != cin or self.output_dim % 4:
            raise ValueError(f"attnpool.c_proj.weight: expected [4 n, {cin}], got {list(lin('c_proj')[0].shape)}")
        f32 = lambda a: torch.from_numpy(a).to(torch.float32)  # noqa: E731  exact for the checkpoint's fp16
        self._reg("pos", f32(pos))
        self._reg("q.w", f32(lin("q_proj")[0]))
        self._reg("q.b", f32(lin("q_proj")[1]))
        self._reg("kv.w", torch.cat([f32(lin("k_proj")[0]), f32(lin("v_proj")[0])]))   # [k_proj; v_proj]: one GEMM, N = 2 C
        self._reg("kv.b", torch.cat([f32(lin("k_proj")[1]), f32(lin("v_proj")[1])]))
        self._reg("c.w", f32(lin("c_proj")[0]))
        self._reg("c.b", f32(lin("c_proj")[1]))

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_state_dict(cls, state, **kw):
        """``state``: ModifiedResNet's state dict (``conv1 .. conv3``, ``bn1 .. bn3``, ``layerS.I.*``, ``attnpool.*``), bare, under
        ``visual.`` (the full CLIP state dict: its other keys are ignored) and / or ``module.``.  ``kw``: ``layers`` ((3, 4, 6, 3) =
        RN50, (3, 4, 23, 3) = RN101), ``heads`` (default: channels / 64), ``chunk``."""
        return cls(state, **kw)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, **kw):
        """A local FILE: a state dict (``torch.save(clip.load("RN50")[0].state_dict(), path)``, made where ``clip`` and its weights
        exist) or the original TorchScript archive (``RN50.pt``).  Never downloads: a path that does not exist is a
        FileNotFoundError."""
        path = os.fspath(pretrained_model_name_or_path)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: no such weight file (CLIPModifiedResNet loads local weights only)")
        try:
            with warnings.catch_warnings():   # torch.load announces a TorchScript archive before it refuses it
                warnings.simplefilter("ignore", UserWarning)
                state = torch.load(path, map_location="cpu", weights_only=True)
        except Exception as plain:   # a TorchScript archive is no pickle of tensors: weights_only refuses it
            try:
                state = torch.jit.load(path, map_location="cpu").state_dict()
            except Exception:
                raise plain
        return cls(state, **kw)

    # ------------------------------------------------------------------ kernels
    def _stem(self, x):
        """-> the stem's output as a pair [B * H/4 * W/4, width]"""
        B, _, H, W = x.shape
        half = self._geom["conv1"][0]
        P = SplitAct.empty(B * (H // 2) * (W // 2), half, x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().mq_clip_stem_conv3x3s2_f32(x.data_ptr(), B, H, W, self.conv1_wt.data_ptr(), self.conv1_b.data_ptr(), half,
                                                              P.hi.data_ptr(), P.lo.data_ptr(), _stream(x)), "mq_clip_stem_conv3x3s2_f32")
        H, W = H // 2, W // 2
        P, _, _ = self._conv3x3("conv2", P, B, H, W)
        P, _, _ = self._conv3x3("conv3", P, B, H, W)
        return self._avgpool(P, B, H, W)

    def _avgpool(self, xin, B, H, W):
        """AvgPool2d(2) of the pair ``xin`` [B * H * W, C] -> pair [B * H/2 * W/2, C]"""
        C = xin.shape[1]
        assert xin.shape[0] == B * H * W
        P = SplitAct.empty(B * (H // 2) * (W // 2), C, xin.device)
        with torch.cuda.device(xin.device):
            _lib.check(_lib.load().mq_avgpool2x2_pair_f32(xin.hi.data_ptr(), xin.lo.data_ptr(), B, H, W, C, P.hi.data_ptr(), P.lo.data_ptr(),
                                                          _stream(xin.hi)), "mq_avgpool2x2_pair_f32")
        return P

    def _attnpool(self, y, B, HW):
        """AttentionPool2d on the last block's fp32 output ``y`` [B * HW, C] -> fp32 [B, output_dim]"""
        lib, C, T, dev = _lib.load(), y.shape[1], HW + 1, y.device
        tokens, mean = SplitAct.empty(B * T, C, dev), SplitAct.empty(B, C, dev)
        with torch.cuda.device(dev):
            _lib.check(lib.mq_attnpool_tokens_f32(y.data_ptr(), B, HW, C, self.pos.data_ptr(), tokens.hi.data_ptr(), tokens.lo.data_ptr(),
                                                  mean.hi.data_ptr(), mean.lo.data_ptr(), _stream(y)), "mq_attnpool_tokens_f32")
        # a GEMM row's sums do not depend on the rows beside it (one K walk per output, whatever M is): batch-invariant
        kv = gemm_nt(tokens, self.kv_w, self.kv_b, epilogue=EPI_BIAS, wsplit=self._wsplit("kv.w"))
        q = gemm_nt(mean, self.q_w, self.q_b, epilogue=EPI_BIAS, wsplit=self._wsplit("q.w"))
        o = SplitAct.empty(B, C, dev)
        with torch.cuda.device(dev):
            _lib.check(lib.mq_attention_single_query_f32(q.data_ptr(), kv.data_ptr(), B, T, self.heads, C // self.heads,
                                                         1.0 / math.sqrt(C // self.heads), o.hi.data_ptr(), o.lo.data_ptr(), _stream(y)),
                       "mq_attention_single_query_f32")
        return gemm_nt(o, self.c_w, self.c_b, epilogue=EPI_BIAS, wsplit=self._wsplit("c.w"))

    # ------------------------------------------------------------------ forward
    def forward(self, pixel_values):
        _check_cuda(pixel_values)
        x = pixel_values.to(torch.float32).contiguous()
        S = self.input_resolution
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, S, S):
            raise ValueError(f"expected [B, 3, {S}, {S}] pixel values (the attention pool's positional embedding is {self.spacial_dim} x "
                             f"{self.spacial_dim}), got {tuple(x.shape)}")
        if x.shape[0] > self.chunk:
            return torch.cat([self._forward(x[s:s + self.chunk]) for s in range(0, x.shape[0], self.chunk)])
        return self._forward(x)

    def _forward(self, x):
        B, H, W = x.shape[0], x.shape[2] // 4, x.shape[3] // 4
        y, H, W = self._stages(self._stem(x), B, H, W)
        return self._attnpool(y, B, H * W)


HIP_CLASSES["CLIPModifiedResNet"] = CLIPModifiedResNet
