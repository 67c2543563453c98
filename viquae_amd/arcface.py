"""ArcFace r50 (insightface `arcface_torch` IResNet-50) on MI355X -- the model behind ``meerqat.image.face_recognition``
(meerqat/image/face_recognition.py:55-61: ``get_model('r50', fp16=True)`` + ``backbone.pth``).

Every convolution is a GEMM on the split-bf16 matrix-pipe kernels (three bf16 MFMA products per fp32 product: fp32-class
accuracy, where the reference runs fp16 autocast); activations are NHWC, so a GEMM's output ``[B * Ho * Wo, Cout]`` IS the next
layer's input.  BatchNorms are eval-mode affines: the one BEHIND a convolution is folded into its weights and bias here, at load
(exact); the one IN FRONT of a convolution (IBasicBlock.bn1, the final bn2) and PReLU are elementwise operations on the tensor the
convolution reads.

The 48 3 x 3 convolutions of the blocks are IMPLICIT GEMMs (``mq_conv3x3_pair_f32``, csrc/conv.hip): no patch matrix is written,
the GEMM's LDS-DMA gathers the taps from the input's (hi, lo) pair, and the elementwise operations ride on the epilogue of the
convolution that PRODUCES a tensor.  An IBasicBlock is two launches:

    P1 = split(prelu(conv1(P0) + b2))                          # P0 = split(bn1(x)), written by the previous block
    x' = conv2(P1) + b3 + identity;   P0' = split(bn1'(x'))    # one epilogue: the fp32 shortcut of the next block + its input pair

(+ im2col and GEMM for the strided 1 x 1 downsample of a stage's first block).  The 3-channel stem (K = 27) is a direct fp32 convolution on
the vector ALU fused with its PReLU (``mq_stem_conv3x3_f32``: writes the first block's input pair and its downsample's operand, never
the full-resolution fp32 tensor); the head (bn2 - flatten - fc - features = one 7 x 7 "convolution", split-K) goes through
``mq_im2col_split_f32`` + the encoder GEMM.  ``_forward_im2col`` runs EVERY convolution that way (round 4's first form, kept as the
check of the implicit one).  The implicit kernel walks K as (32-channel block, tap) -- the nine taps of a block re-read the same
input lines back to back, +6 % from L2 hits alone -- and the library picks its tile; the two forwards agree within fp32 rounding
(tests/test_arcface_gpu.py; per convolution, the (tap, block) order of the explicit path gives its bits exactly).

Parity: arcface_torch is not vendored by the reference and not installable here -- ``oracle/arcface.py`` restates the PUBLISHED
definition (parity unpinned); ``tests/test_arcface_gpu.py`` holds this module to that oracle within 1e-3.

``precision="fp16"`` (opt-in) runs the trunk at the reference's own precision, ``get_model('r50', fp16=True)``: fp16 autocast up to
``flatten``, the head in fp32.  Every activation is ONE fp16 tensor (not a bf16 pair), every 3 x 3 convolution one
``v_mfma_f32_32x32x16_f16`` per 16 k instead of three bf16 products, and the rounding points are autocast's: the convolution's
output is rounded BEFORE its BatchNorm, so nothing is folded -- each convolution keeps its fp16 weights and its BatchNorm as an
affine of the epilogue (``mq_conv3x3_f16``, ``mq_stem_conv3x3_f16``, ``mq_conv1x1_f16``; ``mq_head_prep_f16`` hands bn2's fp16
output to the unchanged fp32-class head GEMM).  Both precisions walk the blocks in one ``_forward``; only the stem, the 3 x 3
launch, the downsample and the hand-off to the head differ, and a model holds the weights of its own precision only.
tests/test_arcface_fp16_gpu.py pins each kernel against a torch restatement of those rounding points (tests/autocast_schedule.py)."""
import os

import numpy as np
import torch

from . import _lib
from .encoders import EPI_BIAS, EPI_BIAS_RESIDUAL, SplitAct, _HipEncoder, _check_cuda, _stream, _tile, gemm_nt, split_bf16_tiled

EPS = 1e-5
LAYERS = (3, 4, 14, 3)
PRECISIONS = ("fp32", "fp16")
CONV_TILE_AUTO, CONV_K_CHANNEL_MAJOR = 0, 0x100   # MQ_CONV_TILE_AUTO, MQ_CONV_K_CHANNEL_MAJOR (include/meerqat_hip.h)
HEAD_SPLITS = 49   # workgroup rows of the head's split-K GEMM


def _half(a):
    """float array -> the same values rounded to fp16 (round to nearest even, as Tensor.half()), as float32"""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def _f16_bits(a):
    """float array -> its fp16 values as an int16 tensor (the bits)"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float16)).view(np.int16))


def f16_empty(rows, channels, device):
    """an fp16 activation [rows, channels] in PAIR LAYOUT (one array, rows padded to 256), as flat int16"""
    return torch.empty(((rows + 255) // 256) * 256 * channels, dtype=torch.int16, device=device)


def _affine(state, name):
    """eval-mode BatchNorm ``name`` as (scale, shift) float64 arrays: y = x * scale + shift"""
    g, b = np.asarray(state[name + ".weight"], np.float64), np.asarray(state[name + ".bias"], np.float64)
    m, v = np.asarray(state[name + ".running_mean"], np.float64), np.asarray(state[name + ".running_var"], np.float64)
    a = g / np.sqrt(v + EPS)
    return a, b - m * a


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


class _Conv:
    """One convolution's geometry: Cout, Cin, k x k, stride, padding; the GEMM's K, (kh, kw, cin), padded to kpad, a multiple of 32."""

    def __init__(self, weight, k, stride, pad):
        self.cout, self.cin = weight.shape[:2]
        self.k, self.stride, self.pad = k, stride, pad
        self.kpad = (k * k * self.cin + 31) // 32 * 32


def _folded(weight, post_bn, kpad):
    """fp32 form of a convolution: W [Cout, kpad] ((kh, kw, cin) order, zeros beyond) with the BatchNorm behind it folded in, and the
    bias [Cout]"""
    w = np.asarray(weight, np.float64)                       # [Cout, Cin, k, k]
    a, b = post_bn
    w2 = w.transpose(0, 2, 3, 1).reshape(w.shape[0], -1) * a[:, None]
    w2 = np.concatenate([w2, np.zeros((w2.shape[0], kpad - w2.shape[1]))], axis=1)
    return w2.astype(np.float32), b.astype(np.float32)


class ArcFaceR50(_HipEncoder):
    """``model(pixel_values)`` -> fp32 [B, 512]; ``pixel_values`` fp32 [B, 3, 112, 112] in [-1, 1] on a GPU."""

    image_size = 112
    num_features = 512

    def __init__(self, state, layers=LAYERS, chunk=656, precision="fp32"):
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
        self.precision = precision
        # chunk = faces per forward: the 14 x 14 stage (half the FLOPs) runs ceil(faces * 196 / 256) workgroups of one 256-row tile
        # each -- 328 faces = 252 of the 256 CUs in one round, 656 = 503 in two (256 faces: 196 of 256; measured 19.3 k -> 21.3 k
        # faces/s at 328 with the first implicit kernel; 23.8 k / 24.7 k at 328 / 656 with the final one)
        state = {k: _np(v).astype(np.float32) for k, v in state.items() if not k.endswith("num_batches_tracked")}
        self.layers, self.chunk = tuple(layers), int(chunk)
        self._convs = {}
        f16 = precision == "fp16"

        def vec(name, arr):
            self._reg(name, torch.from_numpy(np.ascontiguousarray(arr, np.float32)))

        def prelu(name):  # fp16: autocast casts the slopes
            w = state[name + ".weight"]
            vec(name, _half(w) if f16 else w)

        def conv(name, post, k, stride, pad):
            """fp32: the BatchNorm ``post`` folded into the weights and a bias (w2, b).  fp16: nothing folded -- autocast rounds the
            convolution's output before the BatchNorm reads it -- the weights rounded to fp16 (w16: tile layout for 3 x 3, row-major
            [Cout, Cin] for 1 x 1) and the BatchNorm as (scale, shift) (ps, pb)."""
            w = state[name + ".weight"]
            c = self._convs[name] = _Conv(w, k, stride, pad)
            if not f16:
                w2, b = _folded(w, _affine(state, post), c.kpad)
                self._reg(name + ".w2", torch.from_numpy(w2))
                self._reg(name + ".b", torch.from_numpy(b))
                return
            a, b = _affine(state, post)
            vec(name + ".ps", a)
            vec(name + ".pb", b)
            if name != "conv1":  # the stem's weights: conv1.wt
                w16 = _f16_bits(w.transpose(0, 2, 3, 1).reshape(c.cout, -1))   # int16 bits as they are (_reg would convert to fp32)
                self.register_buffer((name + ".w16").replace(".", "_"), (_tile(w16) if k == 3 else w16).contiguous(), persistent=False)

        conv("conv1", "bn1", 3, 1, 1)
        prelu("prelu")
        # the stem as a direct convolution (mq_stem_conv3x3_f32 / _f16): weights [27, 64], row (kh * 3 + kw) * 3 + c
        wt = _half(state["conv1.weight"].transpose(2, 3, 1, 0).reshape(27, -1)) if f16 else self.conv1_w2[:, :27].T.numpy()
        self._reg("conv1.wt", torch.from_numpy(np.ascontiguousarray(wt)))
        for s, n in enumerate(self.layers, start=1):
            for i in range(n):
                p = f"layer{s}.{i}"
                a, b = _affine(state, p + ".bn1")
                vec(p + ".pre_scale", a)
                vec(p + ".pre_shift", b)
                conv(p + ".conv1", p + ".bn2", 3, 1, 1)
                prelu(p + ".prelu")
                conv(p + ".conv2", p + ".bn3", 3, 2 if i == 0 else 1, 1)
                if i == 0:
                    conv(p + ".downsample.0", p + ".downsample.1", 1, 2, 0)
        # head: bn2 (on the im2col) - flatten in NCHW order - fc - BatchNorm1d.  The 7 x 7 x 512 patch of the NHWC activation has
        # column (h * 7 + w) * 512 + c where the checkpoint's fc has column c * 49 + h * 7 + w: permute once; fold `features` in.
        a2, b2 = _affine(state, "bn2")
        vec("head.pre_scale", a2)
        vec("head.pre_shift", b2)
        fa, fb = _affine(state, "features")
        wfc = np.asarray(state["fc.weight"], np.float64).reshape(-1, 512, 7, 7).transpose(0, 2, 3, 1).reshape(-1, 512 * 49)
        self._reg("fc.w2", torch.from_numpy((wfc * fa[:, None]).astype(np.float32)))
        self._reg("fc.b", torch.from_numpy((np.asarray(state["fc.bias"], np.float64) * fa + fb).astype(np.float32)))
        self.num_features = wfc.shape[0]

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_state_dict(cls, state, **kw):
        """``kw``: ``layers``, ``chunk``, ``precision`` ("fp32", the default, or "fp16")"""
        return cls(state, **kw)

    @classmethod
    def from_pretrained(cls, weight_path, **kw):
        """``backbone.pth`` of insightface's arcface_torch (a plain state dict), e.g. ms1mv3_arcface_r50_fp16/backbone.pth."""
        state = torch.load(os.fspath(weight_path), map_location="cpu", weights_only=True)
        return cls(state, **kw)

    # ------------------------------------------------------------------ forward
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

    def _conv(self, name, x, B, H, W, nchw=False, slope=None, scale=None, shift=None, residual=None):
        """x: fp32 [B, H, W, Cin] (or NCHW) -> ([B * Ho * Wo, Cout] fp32, Ho, Wo)"""
        c = self._convs[name]
        Ho, Wo = (H + 2 * c.pad - c.k) // c.stride + 1, (W + 2 * c.pad - c.k) // c.stride + 1
        A = self._im2col(x, B, H, W, c.cin, nchw, c.k, c.k, c.stride, c.pad, c.kpad, slope, scale, shift)
        y = gemm_nt(A, self._b(name + ".w2"), bias=self._b(name + ".b"), residual=residual,
                    epilogue=EPI_BIAS_RESIDUAL if residual is not None else EPI_BIAS, wsplit=self._wsplit(name + ".w2"))
        return y, Ho, Wo

    @staticmethod
    def _im2col(x, B, H, W, C, nchw, KH, KW, stride, pad, kpad, slope, scale, shift):
        lib = _lib.load()
        _check_cuda(x)
        Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        A = SplitAct.empty(B * Ho * Wo, kpad, x.device)
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        with torch.cuda.device(x.device):
            _lib.check(lib.mq_im2col_split_f32(x.data_ptr(), B, H, W, C, int(nchw), KH, KW, stride, pad, p(slope), p(scale), p(shift),
                                               A.hi.data_ptr(), A.lo.data_ptr(), kpad, _stream(x)), "mq_im2col_split_f32")
        return A

    def _stem(self, x, first):
        """The stem fused with its PReLU: -> (block ``first``'s conv1 input, bn1 applied; the operand of its strided 1 x 1 downsample,
        the activated pixels at even coordinates) -- the full-resolution tensor is never stored.  fp32: split pairs; fp16: fp16."""
        lib = _lib.load()
        B, H, W, dev = x.shape[0], self.image_size, self.image_size, x.device
        ptr = lambda n: self._b(n).data_ptr()  # noqa: E731
        with torch.cuda.device(dev):
            if self.precision == "fp16":
                xin, ds_in = f16_empty(B * H * W, 64, dev), f16_empty(B * (H // 2) * (W // 2), 64, dev)
                _lib.check(lib.mq_stem_conv3x3_f16(x.data_ptr(), B, H, W, ptr("conv1.wt"), ptr("conv1.ps"), ptr("conv1.pb"), ptr("prelu"),
                                                   ptr(first + ".pre_scale"), ptr(first + ".pre_shift"), xin.data_ptr(), ds_in.data_ptr(),
                                                   _stream(x)), "mq_stem_conv3x3_f16")
            else:
                xin, ds_in = SplitAct.empty(B * H * W, 64, dev), SplitAct.empty(B * (H // 2) * (W // 2), 64, dev)
                _lib.check(lib.mq_stem_conv3x3_f32(x.data_ptr(), B, H, W, ptr("conv1.wt"), ptr("conv1.b"), ptr("prelu"),
                                                   ptr(first + ".pre_scale"), ptr(first + ".pre_shift"), xin.hi.data_ptr(), xin.lo.data_ptr(),
                                                   ds_in.hi.data_ptr(), ds_in.lo.data_ptr(), _stream(x)), "mq_stem_conv3x3_f32")
        return xin, ds_in

    def _conv3x3(self, name, xin, B, H, W, slope=None, residual=None, scale=None, shift=None):
        """The 3 x 3 convolution ``name`` as an implicit GEMM on ``xin`` [B * H * W, Cin], its input AFTER the pre-operations (fp32: a
        SplitAct, mq_conv3x3_pair_f32; fp16: one fp16 tensor, mq_conv3x3_f16).  ``slope``: -> P = prelu(conv).  Otherwise: -> (Y = conv
        + residual, P = Y * scale + shift or None).  The library picks the tile; K is walked by channel block."""
        lib = _lib.load()
        c, f16 = self._convs[name], self.precision == "fp16"
        assert c.k == 3 and c.pad == 1 and (f16 or xin.shape == (B * H * W, c.cin))
        Ho, Wo = (H - 1) // c.stride + 1, (W - 1) // c.stride + 1
        M, dev = B * Ho * Wo, xin.device
        P = Y = None
        if slope is not None or scale is not None:
            P = f16_empty(M, c.cout, dev) if f16 else SplitAct.empty(M, c.cout, dev)
        if slope is None:
            Y = f16_empty(M, c.cout, dev) if f16 else torch.empty((M, c.cout), dtype=torch.float32, device=dev)
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        tile = CONV_TILE_AUTO | CONV_K_CHANNEL_MAJOR
        with torch.cuda.device(dev):
            if f16:
                _lib.check(lib.mq_conv3x3_f16(xin.data_ptr(), B, H, W, c.cin, c.stride, self._b(name + ".w16").data_ptr(), c.cout,
                                              self._b(name + ".ps").data_ptr(), self._b(name + ".pb").data_ptr(), p(slope), p(residual),
                                              p(scale), p(shift), p(Y), p(P), self._zeros(dev).data_ptr(), tile, _stream(xin)),
                           "mq_conv3x3_f16")
            else:
                wh, wl = self._wsplit(name + ".w2")
                _lib.check(lib.mq_conv3x3_pair_f32(xin.hi.data_ptr(), xin.lo.data_ptr(), B, H, W, c.cin, c.stride, wh.data_ptr(),
                                                   wl.data_ptr(), c.cout, self._b(name + ".b").data_ptr(), p(slope), p(residual), p(scale),
                                                   p(shift), p(Y), P.hi.data_ptr() if P is not None else None,
                                                   P.lo.data_ptr() if P is not None else None, self._zeros(dev).data_ptr(), tile,
                                                   _stream(xin.hi)), "mq_conv3x3_pair_f32")
        return (P if slope is not None else (Y, P)), Ho, Wo

    def _downsample(self, name, src, B, H, W, stride):
        """The 1 x 1 convolution ``name`` on ``src`` [B * H * W, Cin] at ``stride`` -> the block's shortcut [B * Ho * Wo, Cout] (fp32 /
        fp16).  Stride 1: ``src`` is the stem's operand, already at even coordinates (fp32: as the GEMM's split pair)."""
        if self.precision == "fp32":
            if stride == 2:
                return self._conv(name, src, B, H, W)[0]
            return gemm_nt(src, self._b(name + ".w2"), bias=self._b(name + ".b"), epilogue=EPI_BIAS, wsplit=self._wsplit(name + ".w2"))
        lib = _lib.load()
        c = self._convs[name]
        y = f16_empty(B * ((H - 1) // stride + 1) * ((W - 1) // stride + 1), c.cout, src.device)
        with torch.cuda.device(src.device):
            _lib.check(lib.mq_conv1x1_f16(src.data_ptr(), B, H, W, c.cin, stride, self._b(name + ".w16").data_ptr(), c.cout,
                                          self._b(name + ".ps").data_ptr(), self._b(name + ".pb").data_ptr(), y.data_ptr(), _stream(src)),
                       "mq_conv1x1_f16")
        return y

    def _head(self, y, B, H, W):
        """bn2 - flatten - fc - features: one 7 x 7 "convolution" on the last block's output ``y``.  bn2's output goes to the GEMM as a
        split pair (fp32: mq_im2col_split_f32; fp16: mq_head_prep_f16, exact).  [B, 512] outputs over K = 25,088: as one GEMM two
        workgroups would walk 784 K steps (1.65 ms of a 15-ms forward), so the K range is split over 49 workgroup rows and the fp32
        partials summed (mq_gemm_nt_bf16x3s_splitk_f32)."""
        lib = _lib.load()
        dev = y.device
        if self.precision == "fp16":
            A = SplitAct.empty(B, H * W * 512, dev)
            with torch.cuda.device(dev):
                _lib.check(lib.mq_head_prep_f16(y.data_ptr(), B, H * W, 512, self._b("head.pre_scale").data_ptr(),
                                                self._b("head.pre_shift").data_ptr(), A.hi.data_ptr(), A.lo.data_ptr(), _stream(y)),
                           "mq_head_prep_f16")
        else:
            A = self._im2col(y, B, H, W, 512, False, H, W, 1, 0, H * W * 512, None, self._b("head.pre_scale"), self._b("head.pre_shift"))
        wh, wl = self._wsplit("fc.w2")
        K, N = H * W * 512, self.fc_w2.shape[0]
        out = torch.empty((B, N), dtype=torch.float32, device=dev)
        part = torch.empty((HEAD_SPLITS, B, N), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.mq_gemm_nt_bf16x3s_splitk_f32(A.hi.data_ptr(), A.lo.data_ptr(), wh.data_ptr(), wl.data_ptr(), self.fc_b.data_ptr(),
                                                         out.data_ptr(), B, N, K, 1, HEAD_SPLITS, part.data_ptr(), _stream(y)),
                       "mq_gemm_nt_bf16x3s_splitk_f32")
        return out

    def forward(self, pixel_values):
        _check_cuda(pixel_values)
        x = pixel_values.to(torch.float32).contiguous()
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != self.image_size or x.shape[3] != self.image_size:
            raise ValueError(f"expected [B, 3, {self.image_size}, {self.image_size}] pixel values, got {tuple(x.shape)}")
        if x.shape[0] > self.chunk:
            return torch.cat([self._forward(x[s:s + self.chunk]) for s in range(0, x.shape[0], self.chunk)])
        return self._forward(x)

    def _forward(self, x):
        """The IResNet walk for both precisions: an IBasicBlock is conv1 (epilogue: PReLU) and conv2 (epilogue: the shortcut, the next
        block's bn1), with the strided 1 x 1 downsample of a stage's first block in between."""
        B, H, W = x.shape[0], self.image_size, self.image_size
        blocks = [f"layer{s}.{i}" for s, n in enumerate(self.layers, start=1) for i in range(n)]
        xin, ds_in = self._stem(x, blocks[0])
        y = None
        for bi, p in enumerate(blocks):
            nxt = blocks[bi + 1] if bi + 1 < len(blocks) else None
            o1, _, _ = self._conv3x3(p + ".conv1", xin, B, H, W, slope=self._b(p + ".prelu"))
            if ds_in is not None:   # the first block: the stem wrote the 1 x 1 stride-2 "patches"
                identity, ds_in = self._downsample(p + ".downsample.0", ds_in, B, H // 2, W // 2, 1), None
            elif (p + ".downsample.0") in self._convs:
                identity = self._downsample(p + ".downsample.0", y, B, H, W, 2)
            else:
                identity = y
            (y, xin), H, W = self._conv3x3(p + ".conv2", o1, B, H, W, residual=identity,
                                           scale=self._b(nxt + ".pre_scale") if nxt else None,
                                           shift=self._b(nxt + ".pre_shift") if nxt else None)
        return self._head(y, B, H, W)

    def _forward_im2col(self, x):
        """Round 4's first form of the fp32 forward, kept as the check of the implicit one: every convolution an explicit im2col + GEMM."""
        B, H, W = x.shape[0], self.image_size, self.image_size
        # stem: conv - BN (folded); its PReLU is applied where the result is read (the first block's im2cols)
        y, H, W = self._conv("conv1", x, B, H, W, nchw=True)
        pending = self._b("prelu")
        for s, n in enumerate(self.layers, start=1):
            for i in range(n):
                p = f"layer{s}.{i}"
                o1, _, _ = self._conv(p + ".conv1", y, B, H, W, slope=pending, scale=self._b(p + ".pre_scale"), shift=self._b(p + ".pre_shift"))
                if i == 0:
                    identity, Ho, Wo = self._conv(p + ".downsample.0", y, B, H, W, slope=pending)
                else:
                    assert pending is None
                    identity = y
                y, Ho, Wo = self._conv(p + ".conv2", o1, B, H, W, slope=self._b(p + ".prelu"), residual=identity)
                H, W, pending = Ho, Wo, None
        return self._head(y, B, H, W)
