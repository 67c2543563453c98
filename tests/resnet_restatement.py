"""torchvision's bottleneck ResNet and the reference's torchvision transform, restated for the tests (torchvision itself is not
installable where this suite is built).

``forward`` is ``torchvision.models.resnet.ResNet`` with ``Bottleneck`` blocks (v1.5: the stride on the 3 x 3) in eval mode, cut before
``avgpool`` and followed by ``nn.AdaptiveMaxPool2d(1)`` / ``nn.AdaptiveAvgPool2d(1)`` -- the ``ImageEncoder`` of
meerqat/image/embedding.py:68-83 -- written with ``torch.nn.functional`` calls on a state dict with torchvision's names.
``transform_restatement`` is ``Compose([Resize, CenterCrop, ToTensor, Normalize])`` on a PIL image (meerqat/image/embedding.py:86-94)
from Pillow's ``Image.resize``, slicing and numpy.  ``seeded_state`` makes deterministic weights whose activations neither die nor
grow through the blocks, so that an absolute tolerance on the pooled features means something."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
LAYERS = (3, 4, 6, 3)
WIDTHS = (64, 128, 256, 512)
EXPANSION = 4
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def seeded_state(seed, layers=LAYERS):
    """A float32 numpy state dict with torchvision's key names.  Convolutions: N(0, gain / fan_in) (He scaling; the downsample
    convolutions, which read the same post-ReLU tensor as conv1 and carry the signal into the next stage, get gain 1 so that the
    stages keep their scale).  BatchNorms: running statistics near (0, 1), gamma near 1 -- except bn3, whose gamma near 0.25 keeps
    each block a perturbation of its shortcut, as zero-init-residual training does -- and small betas."""
    rng = np.random.default_rng(seed)
    state = {}

    def conv(name, cout, cin, k, gain=2.0):
        state[name + ".weight"] = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(gain / (cin * k * k))).astype(np.float32)

    def bn(name, c, gamma=1.0):
        state[name + ".weight"] = (gamma * rng.uniform(0.8, 1.2, c)).astype(np.float32)
        state[name + ".bias"] = (0.1 * rng.standard_normal(c)).astype(np.float32)
        state[name + ".running_mean"] = (0.1 * rng.standard_normal(c)).astype(np.float32)
        state[name + ".running_var"] = rng.uniform(0.8, 1.2, c).astype(np.float32)
        state[name + ".num_batches_tracked"] = np.asarray(1000, np.int64)

    conv("conv1", 64, 3, 7)
    bn("bn1", 64)
    cin = 64
    for s, (n, width) in enumerate(zip(layers, WIDTHS), start=1):
        for i in range(n):
            p = f"layer{s}.{i}"
            conv(p + ".conv1", width, cin, 1)
            bn(p + ".bn1", width)
            conv(p + ".conv2", width, width, 3)
            bn(p + ".bn2", width)
            conv(p + ".conv3", width * EXPANSION, width, 1)
            bn(p + ".bn3", width * EXPANSION, gamma=0.25)
            if i == 0:
                conv(p + ".downsample.0", width * EXPANSION, cin, 1, gain=1.0)
                bn(p + ".downsample.1", width * EXPANSION)
            cin = width * EXPANSION
    state["fc.weight"] = (rng.standard_normal((10, cin)) / np.sqrt(cin)).astype(np.float32)   # present in every torchvision state dict
    state["fc.bias"] = np.zeros(10, np.float32)
    return state


def _bn(x, state, name):
    t = lambda k: torch.as_tensor(state[name + k]).to(x.dtype)  # noqa: E731
    return F.batch_norm(x, t(".running_mean"), t(".running_var"), t(".weight"), t(".bias"), training=False, eps=EPS)


def _conv(x, state, name, stride=1, padding=0):
    return F.conv2d(x, torch.as_tensor(state[name + ".weight"]).to(x.dtype), stride=stride, padding=padding)


def features(state, x, layers=LAYERS):
    """the encoder: every child of the torchvision model up to and including layer4 -> [B, C, H / 32, W / 32]"""
    x = F.relu(_bn(_conv(x, state, "conv1", 2, 3), state, "bn1"))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    for s, n in enumerate(layers, start=1):
        for i in range(n):
            p = f"layer{s}.{i}"
            stride = 2 if (i == 0 and s > 1) else 1
            out = F.relu(_bn(_conv(x, state, p + ".conv1"), state, p + ".bn1"))
            out = F.relu(_bn(_conv(out, state, p + ".conv2", stride, 1), state, p + ".bn2"))
            out = _bn(_conv(out, state, p + ".conv3"), state, p + ".bn3")
            if (p + ".downsample.0.weight") in state:
                x = _bn(_conv(x, state, p + ".downsample.0", stride), state, p + ".downsample.1")
            x = F.relu(out + x)
    return x


def forward(state, x, layers=LAYERS, pool="AdaptiveMaxPool2d", dtype=torch.float64):
    """``x``: [B, 3, H, W] array or tensor -> the pooled features [B, C, 1, 1] in ``dtype``, on the CPU"""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    with torch.no_grad():
        f = features(state, x, layers)
        return F.adaptive_max_pool2d(f, 1) if pool == "AdaptiveMaxPool2d" else F.adaptive_avg_pool2d(f, 1)


def resize_output_size(h, w, size):
    """torchvision ``Resize``: an int is the shortest edge, the long edge int(size * long / short); a pair is (h, w)"""
    if isinstance(size, (list, tuple)):
        if len(size) == 2:
            return int(size[0]), int(size[1])
        size = size[0]
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = int(size), int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def crop_origin(size, crop):
    """torchvision ``CenterCrop``: int(round((size - crop) / 2.0)), Python's round (half to even)"""
    return int(round((size - crop) / 2.0))


def transform_restatement(image, size=224, crop_size=224, mean=MEAN, std=STD, interpolation="bilinear"):
    """PIL image -> float32 [3, crop, crop]: Resize -> CenterCrop -> ToTensor -> Normalize, in their arithmetic"""
    from PIL import Image
    image = image.convert("RGB")   # what load_image hands to the transform
    oh, ow = resize_output_size(image.height, image.width, size)
    resample = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, 2: Image.BILINEAR, 3: Image.BICUBIC}[interpolation]
    if (oh, ow) != (image.height, image.width):
        image = image.resize((ow, oh), resample)
    ch, cw = (crop_size, crop_size) if isinstance(crop_size, int) else crop_size
    if oh < ch or ow < cw:
        raise NotImplementedError("torchvision pads images smaller than the crop window")
    top, left = crop_origin(oh, ch), crop_origin(ow, cw)
    a = np.asarray(image)[top:top + ch, left:left + cw]
    x = a.astype(np.float32).transpose(2, 0, 1) / np.float32(255)                     # ToTensor: fp32 division
    m, s = np.asarray(mean, np.float32)[:, None, None], np.asarray(std, np.float32)[:, None, None]
    return (x - m) / s                                                                 # Normalize: fp32 sub, fp32 div


def golden_images(seed, n=8, size=224):
    """n uint8 [size, size, 3] images of random blocks, block edge 4 ... 56 pixels (all spatial frequencies the network sees; and
    they compress)"""
    rng = np.random.default_rng(seed)
    edges = (4, 7, 8, 14, 16, 28, 32, 56)
    out = []
    for i in range(n):
        e = edges[i % len(edges)]
        blocks = rng.integers(0, 256, (size // e, size // e, 3), dtype=np.uint8)
        out.append(np.repeat(np.repeat(blocks, e, axis=0), e, axis=1))
    return np.stack(out)


def normalize_u8(images_u8, mean=MEAN, std=STD):
    """uint8 [B, H, W, 3] -> the fp32 [B, 3, H, W] pixel values ToTensor + Normalize make of them"""
    x = images_u8.astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255)
    return (x - np.asarray(mean, np.float32)[None, :, None, None]) / np.asarray(std, np.float32)[None, :, None, None]
