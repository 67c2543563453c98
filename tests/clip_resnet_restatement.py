"""openai-clip's ``ModifiedResNet`` (the visual tower of ``clip.load("RN50")``), restated for the tests from the published
architecture (the ``clip`` package is not installable where this suite is built).

``forward`` is ``clip.model.ModifiedResNet`` in eval mode, written with ``torch.nn.functional`` calls on a state dict with CLIP's
names: the three-convolution stem and its ``AvgPool2d(2)``, ``Bottleneck`` blocks whose stride is an ``AvgPool2d(2)`` behind
``relu(bn2(conv2))`` and in front of the shortcut's 1 x 1, and ``AttentionPool2d`` written out (projections, scale, softmax, weighted
sum) instead of through ``nn.MultiheadAttention``.  The transform of ``clip.load`` (``Resize(n, BICUBIC)``, ``CenterCrop(n)``, RGB,
``ToTensor``, ``Normalize``) is :func:`tests.resnet_restatement.transform_restatement` with CLIP's constants (``transform``).

``seeded_state`` makes deterministic weights in the checkpoint's storage precision (convolution and linear tensors fp16, BatchNorm
tensors and the positional embedding fp32) whose activations neither die nor grow through the blocks and whose attention is neither
uniform nor one-hot.  Achieved on the golden (seed 7, layers (3, 4, 6, 3), 224 x 224, the 8 images of ``golden_images(11)``), float64:
max |output| = 5.23; the entropy of the 8 x 32 softmax rows over the 50 tokens lies in [2.04, 3.51] nats, mean 3.14 (uniform: ln 50 =
3.91; one-hot: 0; the largest single probability is 0.58); the last block's output has max 7.16 and 75 % of its elements above zero;
the fp32 run of this file differs from the float64 one by 2.8e-6."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.resnet_restatement import golden_images, normalize_u8, transform_restatement  # noqa: F401  (re-exported for the tests)

EPS = 1e-5
LAYERS = (3, 4, 6, 3)
WIDTH = 64
EXPANSION = 4
HEAD_DIM = 64
OUTPUT_DIM = 1024
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def seeded_state(seed, layers=LAYERS, input_resolution=224, width=WIDTH, output_dim=OUTPUT_DIM):
    """A numpy state dict with ModifiedResNet's key names (no ``visual.`` prefix), stored as the published checkpoint stores it:
    convolution and linear weights and biases as float16, BatchNorm tensors and ``attnpool.positional_embedding`` as float32.
    Convolutions: N(0, gain / fan_in) (He scaling; gain 1 for the downsample convolutions); BatchNorms: running statistics near (0, 1),
    gamma near 1 -- bn3 near 0.25, which keeps each block a perturbation of its shortcut -- and small betas, as
    ``resnet_restatement.seeded_state``.  Attention pool: positional embedding N(0, 0.25); q_proj and k_proj N(0, 3 / C) so that the
    scores spread by about one unit over the tokens; v_proj N(0, 1 / C); c_proj N(0, 4 / C)."""
    rng = np.random.default_rng(seed)
    state = {}

    def conv(name, cout, cin, k, gain=2.0):
        state[name + ".weight"] = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(gain / (cin * k * k))).astype(np.float16)

    def bn(name, c, gamma=1.0):
        state[name + ".weight"] = (gamma * rng.uniform(0.8, 1.2, c)).astype(np.float32)
        state[name + ".bias"] = (0.1 * rng.standard_normal(c)).astype(np.float32)
        state[name + ".running_mean"] = (0.1 * rng.standard_normal(c)).astype(np.float32)
        state[name + ".running_var"] = rng.uniform(0.8, 1.2, c).astype(np.float32)
        state[name + ".num_batches_tracked"] = np.asarray(1000, np.int64)

    def linear(name, cout, cin, gain):
        state[name + ".weight"] = (rng.standard_normal((cout, cin)) * np.sqrt(gain / cin)).astype(np.float16)
        state[name + ".bias"] = (0.1 * rng.standard_normal(cout)).astype(np.float16)

    conv("conv1", width // 2, 3, 3)
    bn("bn1", width // 2)
    conv("conv2", width // 2, width // 2, 3)
    bn("bn2", width // 2)
    conv("conv3", width, width // 2, 3)
    bn("bn3", width)
    cin = width
    for s, n in enumerate(layers, start=1):
        planes = width * 2 ** (s - 1)
        for i in range(n):
            p = f"layer{s}.{i}"
            conv(p + ".conv1", planes, cin, 1)
            bn(p + ".bn1", planes)
            conv(p + ".conv2", planes, planes, 3)
            bn(p + ".bn2", planes)
            conv(p + ".conv3", planes * EXPANSION, planes, 1)
            bn(p + ".bn3", planes * EXPANSION, gamma=0.25)
            if i == 0:   # stride > 1 or a change of width: ("-1", AvgPool2d) has no tensors, ("0", conv 1 x 1), ("1", BatchNorm)
                conv(p + ".downsample.0", planes * EXPANSION, cin, 1, gain=1.0)
                bn(p + ".downsample.1", planes * EXPANSION)
            cin = planes * EXPANSION
    spacial = input_resolution // 32
    state["attnpool.positional_embedding"] = (0.5 * rng.standard_normal((spacial * spacial + 1, cin))).astype(np.float32)
    linear("attnpool.q_proj", cin, cin, 3.0)
    linear("attnpool.k_proj", cin, cin, 3.0)
    linear("attnpool.v_proj", cin, cin, 1.0)
    linear("attnpool.c_proj", output_dim, cin, 4.0)
    return state


def _t(state, key, dtype):
    return torch.as_tensor(state[key]).to(dtype)   # numpy arrays (the seeded state) or tensors on any device


def _bn(x, state, name):
    t = lambda k: _t(state, name + k, x.dtype)  # noqa: E731
    return F.batch_norm(x, t(".running_mean"), t(".running_var"), t(".weight"), t(".bias"), training=False, eps=EPS)


def _conv(x, state, name, stride=1, padding=0):
    return F.conv2d(x, _t(state, name + ".weight", x.dtype), stride=stride, padding=padding)


def _linear(x, state, name):
    return F.linear(x, _t(state, name + ".weight", x.dtype), _t(state, name + ".bias", x.dtype))


def features(state, x, layers=LAYERS):
    """stem and the four stages -> [B, C, H / 32, W / 32]"""
    x = F.relu(_bn(_conv(x, state, "conv1", 2, 1), state, "bn1"))
    x = F.relu(_bn(_conv(x, state, "conv2", 1, 1), state, "bn2"))
    x = F.relu(_bn(_conv(x, state, "conv3", 1, 1), state, "bn3"))
    x = F.avg_pool2d(x, 2)
    for s, n in enumerate(layers, start=1):
        for i in range(n):
            p = f"layer{s}.{i}"
            stride = 2 if (i == 0 and s > 1) else 1
            out = F.relu(_bn(_conv(x, state, p + ".conv1"), state, p + ".bn1"))
            out = F.relu(_bn(_conv(out, state, p + ".conv2", 1, 1), state, p + ".bn2"))
            if stride > 1:
                out = F.avg_pool2d(out, stride)
            out = _bn(_conv(out, state, p + ".conv3"), state, p + ".bn3")
            if (p + ".downsample.0.weight") in state:
                if stride > 1:
                    x = F.avg_pool2d(x, stride)
                x = _bn(_conv(x, state, p + ".downsample.0"), state, p + ".downsample.1")
            x = F.relu(out + x)
    return x


def attention_pool(state, f, return_attention=False):
    """AttentionPool2d on the feature map ``f`` [B, C, h, w] -> [B, output_dim] (and the softmax [B, heads, h w + 1])"""
    B, C = f.shape[:2]
    heads = C // HEAD_DIM
    x = f.flatten(2).permute(0, 2, 1)                                        # [B, HW, C]
    x = torch.cat([x.mean(dim=1, keepdim=True), x], dim=1)                  # [B, HW + 1, C]
    x = x + _t(state, "attnpool.positional_embedding", x.dtype)[None]
    T = x.shape[1]
    q = _linear(x[:, :1], state, "attnpool.q_proj").view(B, 1, heads, HEAD_DIM).transpose(1, 2)    # [B, heads, 1, 64]
    k = _linear(x, state, "attnpool.k_proj").view(B, T, heads, HEAD_DIM).transpose(1, 2)           # [B, heads, T, 64]
    v = _linear(x, state, "attnpool.v_proj").view(B, T, heads, HEAD_DIM).transpose(1, 2)
    scores = (q * HEAD_DIM ** -0.5) @ k.transpose(2, 3)                      # [B, heads, 1, T]: the query is scaled, as in F.multi_head_attention_forward
    p = torch.softmax(scores, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(B, C)
    out = _linear(o, state, "attnpool.c_proj")
    return (out, p[:, :, 0]) if return_attention else out


def forward(state, x, layers=LAYERS, dtype=torch.float64, return_attention=False):
    """``x``: [B, 3, S, S] array or tensor -> the image features [B, output_dim] in ``dtype``, on the CPU"""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    with torch.no_grad():
        return attention_pool(state, features(state, x, layers), return_attention)


def transform(image, size=224):
    """``clip.load``'s ``_transform(size)`` on a PIL image -> float32 [3, size, size]"""
    return transform_restatement(image, size=size, crop_size=size, mean=MEAN, std=STD, interpolation="bicubic")
