"""MTCNN face detection (``facenet_pytorch.models.mtcnn`` + ``utils/detect_face.py``) restated in torch-CPU and numpy for the
tests: facenet_pytorch, torchvision and cv2 are not installable where this suite is built, so THIS module is the checker of
csrc/mtcnn.hip and parity with the published package on the published checkpoints is UNPINNED.

Every point below is restated from memory of the published code and must be confirmed by a future pin (tools/mtcnn_compare.py):

* scale rule: ``m = 12 / min_face_size``; scales ``m * factor**k`` while ``min(h, w) * m * factor**k >= 12`` (the running products
  are formed by repeated multiplication, as published);
* pyramid / crop resampling: ``interpolate(size=(int(h * s + 1), int(w * s + 1)), mode="area")`` = adaptive average pooling over
  ``[floor(i * in / out), ceil((i + 1) * in / out))``, then ``(x - 127.5) * 0.0078125``;
* P-Net / R-Net / O-Net layers, ceil-mode pools, two-channel softmax, state-dict key names; the flatten order in front of the dense
  layers is ``x.permute(0, 3, 2, 1)`` of ``[N, C, H, W]``, i.e. flat index ``(w * H + h) * C + c``;
* box generation: stride 2, cell 12, ``floor((2 * idx + 1) / s)`` and ``floor((2 * idx + 12) / s)``, threshold ``prob >= t0``;
  the division is done in float32 in BOTH dtypes of this restatement (the published tensors are float32 and these are integer
  decisions: a float64 quotient would floor differently at the many exactly-integer quotients such as 3 / 0.6);
* the ``+1`` conventions: all four NMS sites measure areas and intersections with ``+1`` (as specified for this build; the three sites
  that the published code hands to ``torchvision.ops.batched_nms`` may in fact measure without -- to be confirmed); first-stage
  regression uses ``x2 - x1`` (no ``+1``), ``bbreg`` after R-Net / O-Net uses ``x2 - x1 + 1``; landmarks use ``x2 - x1 + 1`` and
  ``- 1``; crops are the 1-based slices ``[y - 1:ey, x - 1:ex]``;
* NMS: greedy by descending score, a box is suppressed when its overlap with a kept box is ``> threshold``; IoU 0.5 within
  (image, scale), 0.7 within the image, 0.7 after R-Net, 0.7 "Min" (intersection over the smaller area) after O-Net.  Equal scores:
  the lower candidate index first (candidate index: scale-major, row-major cell order; after R-Net / O-Net the position in the
  stage's input list) -- this project's fixed order, the published sort documents none;
* R-Net / O-Net thresholds are strict (``score > t``);
* ``rerec`` squares the box around its centre, ``pad`` truncates towards zero and clips to ``[1, w] x [1, h]``;
* crop-skip rule: a box with ``ey <= y - 1`` or ``ex <= x - 1`` after ``pad`` gets no crop.  The published code then misaligns its
  lists; here such a box is dropped (it can never pass a threshold);
* ordering of the final lists: per image, the order the last NMS leaves (descending score);
* output dtypes: float32 boxes ``[n, 5]`` (x1, y1, x2, y2, prob) and points ``[n, 5, 2]``.

The published code runs a same-sized batch jointly; nothing couples the images, so ``detect_face`` here loops over them.
``seeded_state`` makes deterministic weights whose activations neither die nor saturate; with them every probability sits near
0.5, so tests take their thresholds from quantiles of the float64 outputs (``quantile_thresholds``)."""
import numpy as np
import torch
import torch.nn.functional as F

STAGES = ("pnet", "nms1", "nms2", "rnet", "nms3", "onet", "nms4")


# ---------------------------------------------------------------- weights
def seeded_state(seed):
    """{"pnet": sd, "rnet": sd, "onet": sd}: float32 numpy state dicts under facenet_pytorch's key names."""
    rng = np.random.default_rng(seed)

    def conv(sd, name, cout, cin, k, gain=1.9):
        sd[name + ".weight"] = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(gain / (cin * k * k))).astype(np.float32)
        sd[name + ".bias"] = (0.05 * rng.standard_normal(cout)).astype(np.float32)

    def dense(sd, name, cout, cin, gain=1.9, bias=0.0):
        sd[name + ".weight"] = (rng.standard_normal((cout, cin)) * np.sqrt(gain / cin)).astype(np.float32)
        sd[name + ".bias"] = (bias + 0.05 * rng.standard_normal(cout)).astype(np.float32)

    def prelu(sd, name, c):
        sd[name + ".weight"] = rng.uniform(0.1, 0.4, c).astype(np.float32)

    p = {}
    conv(p, "conv1", 10, 3, 3), prelu(p, "prelu1", 10)
    conv(p, "conv2", 16, 10, 3), prelu(p, "prelu2", 16)
    conv(p, "conv3", 32, 16, 3), prelu(p, "prelu3", 32)
    conv(p, "conv4_1", 2, 32, 1, gain=1.0), conv(p, "conv4_2", 4, 32, 1, gain=0.02)
    r = {}
    conv(r, "conv1", 28, 3, 3), prelu(r, "prelu1", 28)
    conv(r, "conv2", 48, 28, 3), prelu(r, "prelu2", 48)
    conv(r, "conv3", 64, 48, 2), prelu(r, "prelu3", 64)
    dense(r, "dense4", 128, 576), prelu(r, "prelu4", 128)
    dense(r, "dense5_1", 2, 128, gain=1.0), dense(r, "dense5_2", 4, 128, gain=0.02)
    o = {}
    conv(o, "conv1", 32, 3, 3), prelu(o, "prelu1", 32)
    conv(o, "conv2", 64, 32, 3), prelu(o, "prelu2", 64)
    conv(o, "conv3", 64, 64, 3), prelu(o, "prelu3", 64)
    conv(o, "conv4", 128, 64, 2), prelu(o, "prelu4", 128)
    dense(o, "dense5", 256, 1152), prelu(o, "prelu5", 256)
    dense(o, "dense6_1", 2, 256, gain=1.0), dense(o, "dense6_2", 4, 256, gain=0.02)
    dense(o, "dense6_3", 10, 256, gain=0.02, bias=0.5)
    return {"pnet": p, "rnet": r, "onet": o}


def _t(sd, key, like):
    v = sd[key]
    v = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
    return v.to(dtype=like.dtype, device=like.device)


def _conv(x, sd, name):
    return F.conv2d(x, _t(sd, name + ".weight", x), _t(sd, name + ".bias", x))


def _dense(x, sd, name):
    return F.linear(x, _t(sd, name + ".weight", x), _t(sd, name + ".bias", x))


def _prelu(x, sd, name):
    return F.prelu(x, _t(sd, name + ".weight", x))


# ---------------------------------------------------------------- networks
def pnet(sd, x):
    """[N, 3, H, W] -> (reg [N, 4, h, w], prob [N, 2, h, w])"""
    x = _prelu(_conv(x, sd, "conv1"), sd, "prelu1")
    x = F.max_pool2d(x, 2, 2, ceil_mode=True)
    x = _prelu(_conv(x, sd, "conv2"), sd, "prelu2")
    x = _prelu(_conv(x, sd, "conv3"), sd, "prelu3")
    return _conv(x, sd, "conv4_2"), F.softmax(_conv(x, sd, "conv4_1"), dim=1)


def rnet(sd, x):
    """[N, 3, 24, 24] -> (reg [N, 4], prob [N, 2])"""
    x = _prelu(_conv(x, sd, "conv1"), sd, "prelu1")
    x = F.max_pool2d(x, 3, 2, ceil_mode=True)
    x = _prelu(_conv(x, sd, "conv2"), sd, "prelu2")
    x = F.max_pool2d(x, 3, 2, ceil_mode=True)
    x = _prelu(_conv(x, sd, "conv3"), sd, "prelu3")
    x = x.permute(0, 3, 2, 1).contiguous()
    x = _prelu(_dense(x.view(x.shape[0], -1), sd, "dense4"), sd, "prelu4")
    return _dense(x, sd, "dense5_2"), F.softmax(_dense(x, sd, "dense5_1"), dim=1)


def onet(sd, x):
    """[N, 3, 48, 48] -> (reg [N, 4], points [N, 10], prob [N, 2])"""
    x = _prelu(_conv(x, sd, "conv1"), sd, "prelu1")
    x = F.max_pool2d(x, 3, 2, ceil_mode=True)
    x = _prelu(_conv(x, sd, "conv2"), sd, "prelu2")
    x = F.max_pool2d(x, 3, 2, ceil_mode=True)
    x = _prelu(_conv(x, sd, "conv3"), sd, "prelu3")
    x = F.max_pool2d(x, 2, 2, ceil_mode=True)
    x = _prelu(_conv(x, sd, "conv4"), sd, "prelu4")
    x = x.permute(0, 3, 2, 1).contiguous()
    x = _prelu(_dense(x.view(x.shape[0], -1), sd, "dense5"), sd, "prelu5")
    return _dense(x, sd, "dense6_2"), _dense(x, sd, "dense6_3"), F.softmax(_dense(x, sd, "dense6_1"), dim=1)


# ---------------------------------------------------------------- geometry
def scale_pyramid(h, w, min_face_size=20, factor=0.709):
    m = 12.0 / min_face_size
    minl = min(h, w) * m
    scale_i, scales = m, []
    while minl >= 12:
        scales.append(scale_i)
        scale_i = scale_i * factor
        minl = minl * factor
    return scales


def pyramid_size(h, w, s):
    return int(h * s + 1), int(w * s + 1)


def imresample(img, size):
    """[N, C, H, W] float tensor -> [N, C, *size], ``interpolate(mode="area")``"""
    return F.interpolate(img, size=size, mode="area")


def normalise(x):
    return (x - 127.5) * 0.0078125


def box_corners(idx, s):
    """integer cell indices -> (floor((2 idx + 1) / s), floor((2 idx + 12) / s)) in float32 arithmetic"""
    bb = np.asarray(idx).astype(np.float32)
    s = np.float32(s)
    return np.floor((np.float32(2) * bb + np.float32(1)) / s), np.floor((np.float32(2) * bb + np.float32(12)) / s)


def generate_bounding_box(reg, prob, s, thresh):
    """reg [4, h, w], prob [h, w] (numpy) -> boxes [n, 9] (x1, y1, x2, y2, score, reg 0..3), cell index [n] (row-major)"""
    ys, xs = np.nonzero(prob >= thresh)
    qx1, qx2 = box_corners(xs, s)
    qy1, qy2 = box_corners(ys, s)
    cols = [qx1, qy1, qx2, qy2, prob[ys, xs]] + [reg[c, ys, xs] for c in range(4)]
    boxes = np.stack([np.asarray(c, prob.dtype) for c in cols], axis=1) if len(ys) else np.zeros((0, 9), prob.dtype)
    return boxes, ys * prob.shape[1] + xs


def nms(boxes, scores, threshold, method="Union", keys=None):
    """Greedy NMS, ``+1`` areas.  -> indices of the kept boxes, by descending score (equal scores: ascending key / index)."""
    n = len(scores)
    if n == 0:
        return np.zeros(0, np.int64)
    keys = np.arange(n) if keys is None else np.asarray(keys)
    order = np.lexsort((keys, -np.asarray(scores)))
    x1, y1, x2, y2 = (boxes[:, c] for c in range(4))
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    alive = np.ones(n, bool)
    keep = []
    for pos, i in enumerate(order):
        if not alive[i]:
            continue
        keep.append(i)
        rest = order[pos + 1:]
        w = np.maximum(0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + 1)
        h = np.maximum(0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + 1)
        inter = w * h
        o = inter / np.minimum(area[i], area[rest]) if method == "Min" else inter / (area[i] + area[rest] - inter)
        alive[rest[o > threshold]] = False
    return np.asarray(keep, np.int64)


def bbreg(boxes, reg, plus_one=True):
    one = 1 if plus_one else 0
    w = boxes[:, 2] - boxes[:, 0] + one
    h = boxes[:, 3] - boxes[:, 1] + one
    out = boxes.copy()
    out[:, 0] = boxes[:, 0] + reg[:, 0] * w
    out[:, 1] = boxes[:, 1] + reg[:, 1] * h
    out[:, 2] = boxes[:, 2] + reg[:, 2] * w
    out[:, 3] = boxes[:, 3] + reg[:, 3] * h
    return out


def rerec(boxes):
    h = boxes[:, 3] - boxes[:, 1]
    w = boxes[:, 2] - boxes[:, 0]
    side = np.maximum(w, h)
    out = boxes.copy()
    out[:, 0] = boxes[:, 0] + w * 0.5 - side * 0.5
    out[:, 1] = boxes[:, 1] + h * 0.5 - side * 0.5
    out[:, 2] = out[:, 0] + side
    out[:, 3] = out[:, 1] + side
    return out


def pad(boxes, w, h):
    """-> int32 (y, ey, x, ex), 1-based inclusive"""
    b = np.trunc(boxes[:, :4]).astype(np.int32)
    x, y, ex, ey = b[:, 0].copy(), b[:, 1].copy(), b[:, 2].copy(), b[:, 3].copy()
    x[x < 1] = 1
    y[y < 1] = 1
    ex[ex > w] = w
    ey[ey > h] = h
    return y, ey, x, ex


def crop_valid(y, ey, x, ex):
    return (ey > y - 1) & (ex > x - 1)


def crops(img, y, ey, x, ex, size, dtype, device="cpu"):
    """img uint8 [H, W, 3] -> normalised [n, 3, size, size] tensor (zeros for skipped boxes) and the valid mask"""
    valid = crop_valid(y, ey, x, ex)
    chw = torch.as_tensor(np.ascontiguousarray(img)).to(device).permute(2, 0, 1).to(dtype)
    out = torch.zeros((len(y), 3, size, size), dtype=dtype, device=device)
    for k in np.nonzero(valid)[0]:
        out[k] = normalise(imresample(chw[None, :, y[k] - 1:ey[k], x[k] - 1:ex[k]], (size, size)))[0]
    return out, valid


# ---------------------------------------------------------------- the three stages on one image
def first_stage(img, state, min_face_size, t0, factor, dtype, trace=None, device="cpu"):
    """-> boxes [n, 9] after the two P-Net NMS sites (regression not applied yet).  trace: per-stage data for the tests."""
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    h, w = img.shape[:2]
    chw = torch.as_tensor(np.ascontiguousarray(img)).to(device).permute(2, 0, 1)[None].to(dtype)
    boxes, keys, levels, base = [], [], [], 0
    n_cand = 0
    for s in scale_pyramid(h, w, min_face_size, factor):
        x = normalise(imresample(chw, pyramid_size(h, w, s)))
        with torch.no_grad():
            reg, prob = pnet(state["pnet"], x)
        reg, prob = reg[0].cpu().numpy(), prob[0, 1].cpu().numpy()
        levels.append(dict(scale=s, input=x[0].cpu().numpy(), reg=reg, prob=prob))
        b, cell = generate_bounding_box(reg, prob, s, t0)
        n_cand += len(b)
        pick = nms(b[:, :4], b[:, 4], 0.5, keys=cell)
        boxes.append(b[pick])
        keys.append(base + cell[pick])
        base += prob.size
    boxes = np.concatenate(boxes) if boxes else np.zeros((0, 9), np_dtype)
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    n1 = len(boxes)
    pick = nms(boxes[:, :4], boxes[:, 4], 0.7, keys=keys)
    boxes = boxes[pick]
    if trace is not None:
        trace.update(levels=levels, counts=dict(pnet=n_cand, nms1=n1, nms2=len(boxes)), stage1=boxes.copy())
    return boxes


def detect_face_one(img, state, min_face_size=20, thresholds=(0.6, 0.7, 0.7), factor=0.709, dtype=torch.float32, trace=None,
                    device="cpu"):
    """One uint8 [H, W, 3] image -> (boxes [n, 5], points [n, 5, 2]) as float32, in the order the last NMS leaves."""
    trace = {} if trace is None else trace
    h, w = img.shape[:2]
    boxes = first_stage(img, state, min_face_size, thresholds[0], factor, dtype, trace, device)
    counts = trace["counts"]
    counts.update(rnet=0, nms3=0, onet=0, nms4=0)
    points = np.zeros((0, 5, 2), boxes.dtype)
    if len(boxes):
        boxes = np.concatenate([bbreg(boxes[:, :4], boxes[:, 5:9], plus_one=False), boxes[:, 4:5]], axis=1)
        boxes = rerec(boxes)
        y, ey, x, ex = pad(boxes, w, h)
        im, valid = crops(img, y, ey, x, ex, 24, dtype, device)
        with torch.no_grad():
            reg, prob = rnet(state["rnet"], im)
        reg, score = reg.cpu().numpy(), prob[:, 1].cpu().numpy()
        trace.update(rnet_in=im.cpu().numpy(), rnet_boxes=boxes.copy(), rnet_pad=np.stack([y, ey, x, ex], 1), rnet_reg=reg, rnet_score=score)
        ipass = np.nonzero((score > thresholds[1]) & valid)[0]
        counts["rnet"] = len(ipass)
        pick = nms(boxes[ipass, :4], score[ipass], 0.7, keys=ipass)
        sel = ipass[pick]
        counts["nms3"] = len(sel)
        boxes = np.concatenate([bbreg(boxes[sel, :4], reg[sel]), score[sel, None]], axis=1)
        boxes = rerec(boxes)
    if len(boxes):
        y, ey, x, ex = pad(boxes, w, h)
        im, valid = crops(img, y, ey, x, ex, 48, dtype, device)
        with torch.no_grad():
            reg, pts, prob = onet(state["onet"], im)
        reg, pts, score = reg.cpu().numpy(), pts.cpu().numpy(), prob[:, 1].cpu().numpy()
        trace.update(onet_in=im.cpu().numpy(), onet_boxes=boxes.copy(), onet_pad=np.stack([y, ey, x, ex], 1), onet_reg=reg, onet_pts=pts,
                     onet_score=score)
        ipass = np.nonzero((score > thresholds[2]) & valid)[0]
        counts["onet"] = len(ipass)
        b = boxes[ipass, :4]
        w_i = b[:, 2] - b[:, 0] + 1
        h_i = b[:, 3] - b[:, 1] + 1
        px = w_i[:, None] * pts[ipass, :5] + b[:, 0:1] - 1
        py = h_i[:, None] * pts[ipass, 5:] + b[:, 1:2] - 1
        points = np.stack([px, py], axis=2)
        boxes = np.concatenate([bbreg(b, reg[ipass]), score[ipass, None]], axis=1)
        pick = nms(boxes[:, :4], boxes[:, 4], 0.7, "Min", keys=ipass)
        boxes, points = boxes[pick], points[pick]
        counts["nms4"] = len(boxes)
    return boxes[:, :5].astype(np.float32), points.astype(np.float32)


def detect(images, state, min_face_size=20, thresholds=(0.6, 0.7, 0.7), factor=0.709, dtype=torch.float32, select_largest=True,
           traces=None, device="cpu"):
    """``MTCNN.detect(list, landmarks=True)``: per image (boxes [n, 4], probs [n], points [n, 5, 2]) or (None, [None], None)."""
    out_b, out_p, out_l = [], [], []
    for i, img in enumerate(images):
        img = np.asarray(img, np.uint8)
        trace = {}
        if min(img.shape[:2]) < 1 or not scale_pyramid(*img.shape[:2], min_face_size, factor):
            box, point = np.zeros((0, 5), np.float32), np.zeros((0, 5, 2), np.float32)
            trace["counts"] = dict.fromkeys(STAGES, 0)
        else:
            box, point = detect_face_one(img, state, min_face_size, thresholds, factor, dtype, trace, device)
        if traces is not None:
            traces.append(trace)
        if len(box) == 0:
            out_b.append(None), out_p.append([None]), out_l.append(None)
            continue
        if select_largest:
            order = np.argsort((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1]))[::-1]
            box, point = box[order], point[order]
        out_b.append(box[:, :4]), out_p.append(box[:, 4]), out_l.append(point)
    return out_b, out_p, out_l


# ---------------------------------------------------------------- the seeded end-to-end set
SET_SEED, WEIGHT_SEED = 11, 5
SET_SIZES = ((40, 40), (48, 64), (64, 48), (72, 96), (96, 80), (56, 56), (88, 60), (61, 77), (80, 80), (52, 70), (70, 52), (96, 96),
             (90, 66), (66, 90), (75, 58), (58, 83))
SET_FACTOR = 0.85
QUANTILES = (0.85, 0.30, 0.50)   # share of P-Net cells / R-Net crops / O-Net crops of the set that do NOT pass


def smooth_image(rng, h, w):
    """A smooth random field (low-resolution noise, bilinearly enlarged) with a little pixel noise: uint8 [h, w, 3]"""
    from PIL import Image
    gh, gw = max(2, h // 8), max(2, w // 8)
    low = rng.uniform(0, 255, (gh, gw, 3)).astype(np.uint8)
    img = np.asarray(Image.fromarray(low).resize((w, h), Image.BILINEAR), np.float64)
    return np.clip(img + rng.normal(0, 4, img.shape), 0, 255).astype(np.uint8)


def seeded_images(seed=SET_SEED, n=16):
    rng = np.random.default_rng(seed)
    return [smooth_image(rng, *SET_SIZES[i % len(SET_SIZES)]) for i in range(n)]


def quantile_thresholds(images, state, quantiles=QUANTILES, min_face_size=20, factor=0.709):
    """Thresholds at which the given share of the float64 restatement's own outputs does not pass, stage by stage (each stage
    measured behind the thresholds of the stages before it).  Midpoints between neighbouring outputs: no output sits on one."""
    def mid(values, q):
        v = np.sort(np.concatenate(values))
        k = min(max(int(q * len(v)), 1), len(v) - 1)
        return float((v[k - 1] + v[k]) / 2)
    probs = []
    for img in images:
        tr = {}
        first_stage(img, state, min_face_size, 2.0, factor, torch.float64, tr)
        probs += [lv["prob"].ravel() for lv in tr["levels"]]
    t0 = mid(probs, quantiles[0])
    scores = []
    for img in images:
        tr = {}
        detect_face_one(img, state, min_face_size, (t0, 2.0, 2.0), factor, torch.float64, tr)
        scores.append(tr.get("rnet_score", np.zeros(0)))
    t1 = mid(scores, quantiles[1])
    scores = []
    for img in images:
        tr = {}
        detect_face_one(img, state, min_face_size, (t0, t1, 2.0), factor, torch.float64, tr)
        scores.append(tr.get("onet_score", np.zeros(0)))
    return t0, t1, mid(scores, quantiles[2])
