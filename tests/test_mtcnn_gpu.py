"""csrc/mtcnn.hip on the device against tests/mtcnn_restatement.py, stage by stage through the C ABI (each stage gets the float64
restatement's inputs for that stage, so one stage's arithmetic error cannot become a different box list further down), then end to
end through ``MTCNN.detect`` and the dataset job.

Tolerance rule: the float32 torch-CPU restatement's own maximum distance to the float64 one on the same inputs is measured; the HIP
result may be at most 4 times that away from the float64 result (a different summation order over at most 1152 terms, the
hardware's exp).  Every test prints the two distances.  Integer and decision stages (box generation, NMS, rerec, pad, crop
coordinates) are compared bit for bit on identical inputs."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import mtcnn_cases
from tests import mtcnn_restatement as R

pytestmark = pytest.mark.gpu
NINF = float("-inf")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def packed_weights(seed=R.WEIGHT_SEED):
    from viquae_amd.image.face_detection import pack_weights
    return {k: dev(v) for k, v in pack_weights(R.seeded_state(seed)).items()}


def check_rule(name, hip, f32, f64):
    """the tolerance rule; prints the measured distances"""
    hip, f32, f64 = np.asarray(hip, np.float64), np.asarray(f32, np.float64), np.asarray(f64, np.float64)
    d32 = float(np.abs(f32 - f64).max()) if f64.size else 0.0
    dhip = float(np.abs(hip - f64).max()) if f64.size else 0.0
    print(f"{name}: float32 restatement {d32:.3e}, HIP {dhip:.3e} from the float64 restatement (bound {4 * d32:.3e})")
    assert dhip <= 4 * d32, (name, dhip, d32)


def pack_images(images):
    offsets, hw, total = np.zeros(len(images), np.int64), np.zeros((len(images), 2), np.int32), 0
    for i, a in enumerate(images):
        offsets[i], hw[i] = total, a.shape[:2]
        total += a.size
    packed = np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in images])
    return dev(packed), dev(offsets), dev(hw.reshape(-1))


def resample(lib, images, jobs):
    """jobs: rows of (image, x0, y0, w, h, out_w, out_h); -> list of [3, out_h, out_w] arrays"""
    from viquae_amd import _lib
    img_d, off_d, hw_d = pack_images(images)
    rows, off = [], 0
    for j in jobs:
        rows.append(tuple(j) + (off,))
        off += 3 * j[5] * j[6]
    out = torch.full((off + 64,), 777.0, dtype=torch.float32, device="cuda")   # 64 guard words behind the buffer
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
    rows_d = dev(np.asarray(rows, np.int64))   # named: a device argument must outlive the launch
    _lib.check(lib.mq_mtcnn_resample_u8_f32(ptr(img_d), ptr(off_d), ptr(hw_d), len(images), ptr(rows_d), len(rows),
                                            max(j[5] * j[6] for j in jobs), ptr(out), off, ptr(overflow), stream()))
    out = out.cpu().numpy()
    assert overflow.item() == 0 and (out[off:] == 777.0).all()
    return [out[r[7]:r[7] + 3 * r[5] * r[6]].reshape(3, r[6], r[5]) for r in rows]


def restated_resample(image, x0, y0, w, h, ow, oh, dtype):
    """the rectangle cut with zeros outside the image, "area" resampled and normalised"""
    H, W = image.shape[:2]
    cut = np.zeros((h, w, 3), np.uint8)
    ys, xs = np.arange(y0, y0 + h), np.arange(x0, x0 + w)
    iy, ix = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    cut[np.ix_(iy, ix)] = image[np.ix_(ys[iy], xs[ix])]
    t = torch.as_tensor(cut).permute(2, 0, 1)[None].to(dtype)
    return R.normalise(R.imresample(t, (oh, ow)))[0].numpy()


# ------------------------------------------------------------------------------------------------ 1. resampling
def test_pyramid_resampling(hip_lib):
    rng = np.random.default_rng(0)
    images = [R.smooth_image(rng, h, w) for h, w in ((20, 20), (37, 53), (64, 48))]
    jobs = []
    for b, im in enumerate(images):
        h, w = im.shape[:2]
        scales = R.scale_pyramid(h, w)
        assert len(scales) >= 1 and (b or len(scales) == 1)   # 20 x 20: one scale, P-Net output 1 x 1
        jobs += [(b, 0, 0, w, h, R.pyramid_size(h, w, s)[1], R.pyramid_size(h, w, s)[0]) for s in scales]
    got = resample(hip_lib, images, jobs)
    f32 = [restated_resample(images[j[0]], *j[1:], torch.float32) for j in jobs]
    f64 = [restated_resample(images[j[0]], *j[1:], torch.float64) for j in jobs]
    assert all(g.shape == w.shape for g, w in zip(got, f64))
    cat = lambda xs: np.concatenate([x.reshape(-1) for x in xs])  # noqa: E731
    check_rule("pyramid", cat(got), cat(f32), cat(f64))


def test_resampling_reads_zero_outside_the_image(hip_lib):
    """rectangles hanging over the four borders and a one-pixel rectangle, straight through the resampling entry"""
    image = R.smooth_image(np.random.default_rng(8), 37, 53)
    jobs = [(0, -5, 3, 30, 25, 24, 24), (0, 10, -7, 21, 30, 24, 24), (0, 40, 20, 30, 13, 48, 48), (0, 7, 25, 33, 20, 48, 48),
            (0, 17, 9, 1, 1, 24, 24), (0, -3, -3, 59, 43, 13, 11)]
    got = resample(hip_lib, [image], jobs)
    cat = lambda xs: np.concatenate([x.reshape(-1) for x in xs])  # noqa: E731
    check_rule("rectangles over the borders", cat(got), cat([restated_resample(image, *j[1:], torch.float32) for j in jobs]),
               cat([restated_resample(image, *j[1:], torch.float64) for j in jobs]))


def _refine(lib, boxes9, image_hw, flags, crop):
    """one segment of records against one image -> (rec, pad, valid, jobs)"""
    from viquae_amd import _lib
    n = len(boxes9)
    rec_in = dev(np.asarray(boxes9, np.float32))
    seg, dst, hw = dev(np.zeros(1, np.int64)), dev(np.array([0, n], np.int64)), dev(np.asarray(image_hw, np.int32))
    rec, img, pad = torch.empty((n, 9), device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((n, 4), dtype=torch.int32, device="cuda")
    jobs, valid = torch.empty((n, 8), dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.mq_mtcnn_refine_f32(ptr(rec_in), ptr(seg), ptr(dst), 1, n, ptr(hw), flags, crop, n, ptr(rec), ptr(img), ptr(pad),
                                       ptr(jobs), ptr(valid), ptr(overflow), stream()))
    assert overflow.item() == 0 and (img == 0).all()
    return rec.cpu().numpy(), pad.cpu().numpy(), valid.cpu().numpy().astype(bool), jobs.cpu().numpy()


@pytest.mark.parametrize("size", [24, 48])
def test_crop_resampling_over_the_borders(hip_lib, size):
    """crops hanging over each border, a one-pixel crop, and boxes that leave nothing (crop-skip rule): pad and the crop
    coordinates bit for bit, the pixels by the tolerance rule"""
    image = R.smooth_image(np.random.default_rng(1), 37, 53)
    boxes = np.array([[-6.5, 10.2, 14.9, 31.6], [20.3, -9.8, 41.2, 11.1], [40.1, 8.0, 60.7, 28.6], [15.5, 25.4, 33.3, 43.2],
                      [12.2, 9.9, 12.9, 9.99], [-20.0, -20.0, 80.0, 70.0], [60.0, 5.0, 70.0, 15.0], [5.0, -30.0, 15.0, -2.0]], np.float32)
    rec = np.concatenate([boxes, np.full((len(boxes), 1), 0.5, np.float32), np.zeros((len(boxes), 4), np.float32)], axis=1)
    out, pad, valid, jobs = _refine(hip_lib, rec, image.shape[:2], 0, size)
    assert np.array_equal(out[:, :4], boxes)   # zero regression, no rerec: untouched
    y, ey, x, ex = R.pad(boxes, 53, 37)
    assert np.array_equal(pad, np.stack([y, ey, x, ex], axis=1)) and np.array_equal(valid, R.crop_valid(y, ey, x, ex))
    assert valid.tolist() == [True] * 6 + [False, False] and (ey[4] - y[4] + 1, ex[4] - x[4] + 1) == (1, 1)
    got = resample(hip_lib, [image], [tuple(int(v) for v in j[:7]) for j in jobs])
    f64, _ = R.crops(image, y, ey, x, ex, size, torch.float64)
    f32, _ = R.crops(image, y, ey, x, ex, size, torch.float32)
    check_rule(f"crops {size}", np.stack(got), f32.numpy(), f64.numpy())


def test_box_refinement_bit_for_bit(hip_lib):
    """regression (both +1 conventions), rerec, trunc and pad against the float32 restatement on identical inputs"""
    rng = np.random.default_rng(2)
    n = 700
    xy = rng.uniform(-10, 90, (n, 2))
    boxes = np.concatenate([xy, xy + rng.uniform(1, 60, (n, 2))], axis=1).astype(np.float32)
    reg = rng.normal(0, 0.2, (n, 4)).astype(np.float32)
    rec = np.concatenate([boxes, rng.uniform(0, 1, (n, 1)).astype(np.float32), reg], axis=1)
    for flags, plus_one, square in ((2, False, True), (3, True, True), (1, True, False)):
        out, pad, valid, _ = _refine(hip_lib, rec, (80, 100), flags, 24)
        want = R.bbreg(boxes, reg, plus_one=plus_one)
        want = R.rerec(want) if square else want
        assert want.dtype == np.float32 and np.array_equal(out[:, :4], want) and np.array_equal(out[:, 4], rec[:, 4])
        y, ey, x, ex = R.pad(want, 100, 80)
        assert np.array_equal(pad, np.stack([y, ey, x, ex], axis=1)) and np.array_equal(valid, R.crop_valid(y, ey, x, ex))


# ------------------------------------------------------------------------------------------------ 2. P-Net
def _pnet(lib, inputs, scales, threshold, cap, n_images=1, images_of=None, want_maps=True, guard=0):
    """inputs: list of [3, h, w] float32 levels -> dict(maps per level, rec / idx / sub lists, count, overflow, raw buffers)"""
    from viquae_amd import _lib
    levels, in_off, map_off, cells, max_tiles = [], 0, 0, {}, 1
    for k, x in enumerate(inputs):
        h, w = x.shape[1:]
        ho, wo = (h - 3) // 2 + 1 - 4, (w - 3) // 2 + 1 - 4
        b = images_of[k] if images_of else 0
        levels.append((in_off, h, w, b, k, cells.get(b, 0), map_off, 0))
        cells[b] = cells.get(b, 0) + ho * wo
        in_off, map_off = in_off + x.size, map_off + 5 * ho * wo
        max_tiles = max(max_tiles, -(-ho // 16) * -(-wo // 16))
    flat = dev(np.concatenate([x.reshape(-1) for x in inputs]).astype(np.float32))
    maps = torch.full((map_off,), np.nan, dtype=torch.float32, device="cuda") if want_maps else None
    total = n_images * cap
    rec = torch.full(((total + guard) * 9,), 777.0, dtype=torch.float32, device="cuda")
    idx = torch.full((total + guard,), -777, dtype=torch.int32, device="cuda")
    sub = torch.full((total + guard,), -777, dtype=torch.int32, device="cuda")
    count, overflow = torch.empty(n_images, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    levels_d, scales_d = dev(np.asarray(levels, np.int64)), dev(np.asarray(scales, np.float32))   # named: they outlive the launch
    _lib.check(lib.mq_mtcnn_pnet_f32(ptr(flat), flat.numel(), ptr(levels_d), ptr(scales_d), len(levels), max_tiles,
                                     ptr(packed_weights()["pnet"]), threshold, n_images, cap, ptr(rec), ptr(idx), ptr(sub), ptr(count),
                                     ptr(overflow), ptr(maps), map_off if want_maps else 0, stream()))
    out = dict(rec=rec.cpu().numpy().reshape(-1, 9), idx=idx.cpu().numpy(), sub=sub.cpu().numpy(), count=count.cpu().numpy(),
               overflow=int(overflow.item()), levels=levels)
    if want_maps:
        m = maps.cpu().numpy()
        out["maps"] = [m[lv[6]:lv[6] + 5 * ((lv[1] - 3) // 2 - 3) * ((lv[2] - 3) // 2 - 3)].reshape(5, (lv[1] - 3) // 2 - 3, (lv[2] - 3) // 2 - 3)
                       for lv in levels]
    return out


PNET_SHAPES = [(12, 12), (13, 13), (14, 31), (50, 45)]   # 13: a partial ceil-mode pool window; 50 x 45: 20 x 18 cells, > one 16 x 16 tile


@functools.lru_cache(maxsize=None)
def pnet_case():
    rng = np.random.default_rng(3)
    inputs = [rng.uniform(-1, 1, (3, h, w)).astype(np.float32) for h, w in PNET_SHAPES]
    state = R.seeded_state(R.WEIGHT_SEED)
    ref = {}
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        ref[name] = []
        for x in inputs:
            with torch.no_grad():
                reg, prob = R.pnet(state["pnet"], torch.as_tensor(x)[None].to(dtype))
            ref[name].append(np.concatenate([prob[0, 1:2].numpy(), reg[0].numpy()]))
    return inputs, ref


def test_pnet_maps(hip_lib):
    inputs, ref = pnet_case()
    got = _pnet(hip_lib, inputs, [0.6] * len(inputs), 2.0, 4)
    assert got["overflow"] == 0 and got["count"].tolist() == [0]
    for k, shape in enumerate(PNET_SHAPES):
        assert got["maps"][k].shape == ref["f64"][k].shape, shape
        check_rule(f"P-Net prob {shape}", got["maps"][k][0], ref["f32"][k][0], ref["f64"][k][0])
        check_rule(f"P-Net reg {shape}", got["maps"][k][1:], ref["f32"][k][1:], ref["f64"][k][1:])
    assert ref["f64"][0].shape == (5, 1, 1) and ref["f64"][1].shape == (5, 2, 2)


# ------------------------------------------------------------------------------------------------ 3. box generation, NMS
def test_box_generation_bit_for_bit(hip_lib):
    """the passing cells of the device's own maps (identical inputs): which cells, their corners, scores, regressions and indices"""
    inputs, ref = pnet_case()
    scales = [0.6, 0.6 * 0.709, 0.3, 0.2137]
    thr = float(np.median(np.concatenate([m[0].ravel() for m in ref["f64"]])))
    got = _pnet(hip_lib, inputs, scales, thr, 1024)
    n, base, want = int(got["count"][0]), 0, []
    for k, s in enumerate(scales):
        prob, reg = got["maps"][k][0], got["maps"][k][1:]
        boxes, cell = R.generate_bounding_box(reg, prob, np.float32(s), np.float32(thr))
        want += [(base + c, k) + tuple(b) for b, c in zip(boxes.tolist(), cell.tolist())]
        base += prob.size
    order = np.argsort(got["idx"][:n])
    have = [(int(got["idx"][i]), int(got["sub"][i])) + tuple(got["rec"][i].tolist()) for i in order]
    assert 10 < n < 1024 and got["overflow"] == 0 and have == want


def _nms(lib, rec, segments, key=None, sub=None, score_gt=NINF, thr=0.5, mode=0, seg_cap=0):
    """segments: list of (start, count) -> per segment the kept source positions (and checks the gathered outputs)"""
    from viquae_amd import _lib
    n_total = len(rec)
    rec_d = dev(np.asarray(rec, np.float32).reshape(n_total, 9)) if n_total else None
    out_rec = torch.full((n_total, 9), 777.0, device="cuda") if n_total else None
    out_key, out_sub, out_src = (torch.full((max(n_total, 1),), -777, dtype=torch.int32, device="cuda") for _ in range(3))
    out_count = torch.full((len(segments),), -1, dtype=torch.int32, device="cuda")
    ws_bytes = lib.mq_mtcnn_nms_workspace_bytes(n_total)
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device="cuda")
    start_d, count_d = dev(np.array([s for s, _ in segments], np.int64)), dev(np.array([c for _, c in segments], np.int32))
    key_d = dev(np.asarray(key, np.int32)) if key is not None else None   # named: device arguments outlive the launch
    sub_d = dev(np.asarray(sub, np.int32)) if sub is not None else None
    _lib.check(lib.mq_mtcnn_nms_f32(ptr(rec_d), n_total, ptr(start_d), ptr(count_d), len(segments), seg_cap, ptr(key_d), ptr(sub_d),
                                    float(score_gt), float(thr), mode, ptr(out_rec),
                                    ptr(out_key), ptr(out_sub), ptr(out_src), ptr(out_count), ptr(ws), ws_bytes, stream()))
    counts, src = out_count.cpu().numpy(), out_src.cpu().numpy()
    kept = [src[s:s + c].tolist() for (s, _), c in zip(segments, counts)]
    if n_total:
        o = out_rec.cpu().numpy()
        for (s, _), k in zip(segments, kept):
            assert np.array_equal(o[s:s + len(k)], np.asarray(rec, np.float32).reshape(n_total, 9)[[s + i for i in k]])
            if key is not None:
                assert out_key.cpu().numpy()[s:s + len(k)].tolist() == [int(key[s + i]) for i in k]
    return kept


def _random_records(rng, n, span=60):
    xy = rng.integers(0, span, (n, 2)).astype(np.float32)
    boxes = np.concatenate([xy, xy + rng.integers(4, 30, (n, 2))], axis=1)
    scores = (rng.integers(0, 32, n) / 32).astype(np.float32)   # many equal scores
    return np.concatenate([boxes, scores[:, None], rng.normal(0, 1, (n, 4))], axis=1).astype(np.float32)


def test_nms_four_sites_bit_for_bit(hip_lib):
    """groups of 0, 1, 2 and several hundred boxes with many equal scores, at the four sites' settings"""
    rng = np.random.default_rng(4)
    sizes = [0, 1, 2, 700, 333]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    rec = np.concatenate([_random_records(rng, n) for n in sizes])
    rec[starts[2] + 1] = rec[starts[2]]   # the group of two: identical boxes and scores, the lower key wins
    rec[starts[1]:starts[3], 4] = 0.5       # the groups of one and two pass the R-Net / O-Net sites' score threshold
    key = np.concatenate([rng.permutation(n) for n in sizes])   # keys are not the positions
    sub = rng.integers(0, 3, len(rec))
    sub[starts[2] + 1] = sub[starts[2]]
    segments = list(zip(starts[:-1].tolist(), sizes))
    for name, kw, rkw in (("site 1", dict(key=key, sub=sub, thr=0.5), dict(threshold=0.5)),
                          ("site 2", dict(key=key, thr=0.7), dict(threshold=0.7)),
                          ("site 3", dict(score_gt=0.4, thr=0.7), dict(threshold=0.7)),
                          ("site 4", dict(score_gt=0.4, thr=0.7, mode=1), dict(threshold=0.7, method="Min"))):
        kept = _nms(hip_lib, rec, segments, **kw)
        for (s, n), k in zip(segments, kept):
            r, kk = rec[s:s + n], (key[s:s + n] if "key" in kw else np.arange(n))
            groups = sub[s:s + n] if "sub" in kw else np.zeros(n, int)
            ok = np.nonzero(r[:, 4] > np.float32(kw.get("score_gt", NINF)))[0]
            want = []
            for g in np.unique(groups[ok]):   # the reference runs each (image, scale) group on its own
                m = ok[groups[ok] == g]
                want += m[R.nms(r[m, :4], r[m, 4], np.float32(rkw["threshold"]), rkw.get("method", "Union"), keys=kk[m])].tolist()
            want.sort(key=lambda i: (-r[i, 4], kk[i]))
            assert k == want, (name, n)
        assert len(kept[3]) < sizes[3] and kept[0] == [] and kept[1] == [0]
        assert kept[2] == ([int(np.argmin(key[starts[2]:starts[2] + 2]))] if "key" in kw else [0])


def test_nms_exact_threshold_and_min_mode(hip_lib):
    z = [0.0] * 4
    rec = np.array([[0, 0, 9, 9, 0.9] + z, [0, 0, 9, 19, 0.8] + z,      # IoU 100 / 200 = 0.5 exactly: not > 0.5, kept
                    [0, 0, 9, 9, 0.9] + z, [0, 0, 6, 9, 0.8] + z,       # IoU 70 / 100 = float32(0.7) exactly: kept at 0.7
                    [0, 0, 9, 9, 0.9] + z, [2, 2, 5, 5, 0.8] + z], np.float32)   # one inside the other: IoU 0.16, "Min" 1.0
    segments = [(0, 2), (2, 2), (4, 2)]
    assert _nms(hip_lib, rec, segments, thr=0.5) == [[0, 1], [0], [0, 1]]
    assert _nms(hip_lib, rec, segments, thr=0.7) == [[0, 1], [0, 1], [0, 1]]
    assert _nms(hip_lib, rec, segments, thr=np.nextafter(np.float32(0.7), np.float32(0))) == [[0, 1], [0], [0, 1]]
    assert _nms(hip_lib, rec, segments, thr=0.7, mode=1) == [[0], [0], [0]]
    for thr, mode in ((0.5, "Union"), (0.7, "Union"), (0.7, "Min")):
        for s, n in segments:
            got = _nms(hip_lib, rec, segments, thr=thr, mode=int(mode == "Min"))[s // 2]
            assert got == R.nms(rec[s:s + n, :4], rec[s:s + n, 4], np.float32(thr), mode).tolist()


# ------------------------------------------------------------------------------------------------ 4. R-Net, O-Net
N_CROPS = 513


@functools.lru_cache(maxsize=None)
def net_case(net):
    size = 24 if net == "rnet" else 48
    rng = np.random.default_rng(5 if net == "rnet" else 6)
    low = rng.uniform(-1, 1, (N_CROPS, 3, size // 4, size // 4))
    x = (np.kron(low, np.ones((4, 4))) + rng.normal(0, 0.05, (N_CROPS, 3, size, size))).astype(np.float32)
    state, ref = R.seeded_state(R.WEIGHT_SEED), {}
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        with torch.no_grad():
            out = getattr(R, net)(state[net], torch.as_tensor(x).to(dtype))
        ref[name] = [o.numpy() for o in out]
    return x, ref


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 513])
def test_rnet(hip_lib, n):
    from viquae_amd import _lib
    x, ref = net_case("rnet")
    rec = torch.full((n + 1, 9), 777.0, device="cuda")
    valid = np.ones(n, np.int32)
    valid[n // 2] = 0 if n > 2 else 1
    x_d, valid_d = dev(x[:n]), dev(valid)
    _lib.check(hip_lib.mq_mtcnn_rnet_f32(ptr(x_d), n, ptr(packed_weights()["rnet"]), ptr(valid_d), ptr(rec), stream()))
    got = rec.cpu().numpy()
    keep = valid.astype(bool)
    assert (got[n] == 777.0).all() and (got[:n, :4] == 777.0).all() and np.isneginf(got[:n][~keep, 4]).all()
    check_rule(f"R-Net score, {n} crops", got[:n][keep, 4], ref["f32"][1][:n][keep, 1], ref["f64"][1][:n][keep, 1])
    check_rule(f"R-Net reg, {n} crops", got[:n][keep, 5:], ref["f32"][0][:n][keep], ref["f64"][0][:n][keep])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 513])
def test_onet(hip_lib, n):
    from viquae_amd import _lib
    x, ref = net_case("onet")
    rec = torch.full((n + 1, 9), 777.0, device="cuda")
    pts = torch.full((n + 1, 10), 777.0, device="cuda")
    x_d = dev(x[:n])
    _lib.check(hip_lib.mq_mtcnn_onet_f32(ptr(x_d), n, ptr(packed_weights()["onet"]), None, ptr(rec), ptr(pts), 0, stream()))
    got, gp = rec.cpu().numpy(), pts.cpu().numpy()
    assert (got[n] == 777.0).all() and (gp[n] == 777.0).all()
    check_rule(f"O-Net score, {n} crops", got[:n, 4], ref["f32"][2][:n, 1], ref["f64"][2][:n, 1])
    check_rule(f"O-Net reg, {n} crops", got[:n, 5:], ref["f32"][0][:n], ref["f64"][0][:n])
    check_rule(f"O-Net points, {n} crops", gp[:n], ref["f32"][1][:n], ref["f64"][1][:n])


def test_onet_landmarks_and_last_regression(hip_lib):
    """MQ_MTCNN_ONET_POST on the raw outputs of the same launch (identical inputs): bit for bit against the float32 restatement"""
    from viquae_amd import _lib
    x, _ = net_case("onet")
    n = 40
    rng = np.random.default_rng(7)
    xy = rng.uniform(0, 60, (n, 2))
    boxes = np.concatenate([xy, xy + rng.uniform(8, 50, (n, 2))], axis=1).astype(np.float32)
    out = []
    for flags in (0, 1):
        rec = dev(np.concatenate([boxes, np.zeros((n, 5), np.float32)], axis=1))
        pts = torch.empty((n, 10), device="cuda")
        x_d = dev(x[:n])
        _lib.check(hip_lib.mq_mtcnn_onet_f32(ptr(x_d), n, ptr(packed_weights()["onet"]), None, ptr(rec), ptr(pts), flags, stream()))
        out.append((rec.cpu().numpy(), pts.cpu().numpy()))
    (raw, raw_pts), (post, post_pts) = out
    w_i, h_i = boxes[:, 2] - boxes[:, 0] + 1, boxes[:, 3] - boxes[:, 1] + 1
    assert np.array_equal(post_pts[:, :5], w_i[:, None] * raw_pts[:, :5] + boxes[:, 0:1] - 1)
    assert np.array_equal(post_pts[:, 5:], h_i[:, None] * raw_pts[:, 5:] + boxes[:, 1:2] - 1)
    assert np.array_equal(post[:, :4], R.bbreg(boxes, raw[:, 5:9])) and np.array_equal(post[:, 4:], raw[:, 4:])


# ------------------------------------------------------------------------------------------------ 5. capacity
def test_candidate_capacity_overflow_and_retry(hip_lib):
    inputs, ref = pnet_case()
    thr = float(np.median(np.concatenate([m[0].ravel() for m in ref["f64"]])))
    scales = [0.6] * len(inputs)
    full = _pnet(hip_lib, inputs, scales, thr, 1024, want_maps=False)
    n = int(full["count"][0])
    cap = n // 3
    small = _pnet(hip_lib, inputs, scales, thr, cap, want_maps=False, guard=64)
    assert small["overflow"] == 1 and int(small["count"][0]) == n > cap > 0      # the counter says how much is needed
    assert (small["rec"][cap:] == 777.0).all() and (small["idx"][cap:] == -777).all() and (small["sub"][cap:] == -777).all()
    assert (small["idx"][:cap] >= 0).all()
    retry = _pnet(hip_lib, inputs, scales, thr, n, want_maps=False, guard=64)
    assert retry["overflow"] == 0 and int(retry["count"][0]) == n and (retry["rec"][n:] == 777.0).all()
    by_idx = lambda r: r["rec"][:n][np.argsort(r["idx"][:n])]  # noqa: E731
    assert np.array_equal(np.sort(retry["idx"][:n]), np.sort(full["idx"][:n])) and np.array_equal(by_idx(retry), by_idx(full))


# ------------------------------------------------------------------------------------------------ 6. / 7. MTCNN.detect
@functools.lru_cache(maxsize=None)
def set_model():
    from viquae_amd.image.face_detection import MTCNN
    s = mtcnn_cases.end_to_end_set()
    model = MTCNN(thresholds=list(s["thresholds"]), factor=s["factor"], select_largest=False, keep_all=True, device="cuda",
                  weights=s["state"])
    model.trace = True
    return model


def test_detect_end_to_end(hip_lib):
    s, model = mtcnn_cases.end_to_end_set(), set_model()
    boxes, probs, points = model.detect(s["images"], landmarks=True)
    counts = model.last_counts.copy()
    assert len(boxes) == 16 and len(s["counted"]) >= 14
    d32 = dhip = p32 = phip = 0.0
    for i in s["counted"]:
        assert counts[i].tolist() == s["f64"]["counts"][i].tolist(), (i, counts[i], s["f64"]["counts"][i])
        b64, b32 = s["f64"]["boxes"][i], s["f32"]["boxes"][i]
        if b64 is None:
            assert boxes[i] is None and probs[i] == [None] and points[i] is None
            continue
        assert boxes[i].shape == b64.shape and boxes[i].dtype == np.float32 and points[i].shape == (len(b64), 5, 2)
        side = np.maximum(b64[:, 2] - b64[:, 0], b64[:, 3] - b64[:, 1]).astype(np.float64)[:, None]
        d32 = max(d32, float((np.abs(b32.astype(np.float64) - b64) / side).max()))
        dhip = max(dhip, float((np.abs(boxes[i].astype(np.float64) - b64) / side).max()))
        d32 = max(d32, float((np.abs(s["f32"]["points"][i].astype(np.float64) - s["f64"]["points"][i]) / side[:, :, None]).max()))
        dhip = max(dhip, float((np.abs(points[i].astype(np.float64) - s["f64"]["points"][i]) / side[:, :, None]).max()))
        p32 = max(p32, float(np.abs(s["f32"]["probs"][i].astype(np.float64) - s["f64"]["probs"][i]).max()))
        phip = max(phip, float(np.abs(probs[i].astype(np.float64) - s["f64"]["probs"][i]).max()))
    print(f"end to end, boxes and landmarks / box side: float32 restatement {d32:.3e}, HIP {dhip:.3e} (bound {4 * d32:.3e}); "
          f"probabilities: float32 restatement {p32:.3e}, HIP {phip:.3e} (bound {4 * p32:.3e})")
    assert dhip <= 4 * d32 and phip <= 4 * p32


def test_batch_composition(hip_lib):
    """each of four images alone and inside the mixed batch of 16: bit-identical outputs"""
    s, model = mtcnn_cases.end_to_end_set(), set_model()
    boxes, probs, points = model.detect(s["images"], landmarks=True)
    for i in (1, 2, 4, 12):
        b, p, l = model.detect(s["images"][i], landmarks=True)
        if boxes[i] is None:
            assert b is None and p == [None] and l is None
            continue
        assert np.array_equal(b, boxes[i]) and np.array_equal(p, probs[i]) and np.array_equal(l, points[i])


def test_detect_small_capacity_retries(hip_lib):
    """a first capacity below the candidate count: the stage is repeated with the counted size, the result is the same"""
    from viquae_amd.image.face_detection import MTCNN
    s, model = mtcnn_cases.end_to_end_set(), set_model()
    small = MTCNN(thresholds=list(s["thresholds"]), factor=s["factor"], select_largest=False, keep_all=True, device="cuda",
                  weights=s["state"], candidate_capacity=8)
    a, b = model.detect(s["images"][:6], landmarks=True), small.detect(s["images"][:6], landmarks=True)
    assert small.retries == 1
    for x, y in zip(a, b):
        assert all((u is None and v is None) or np.array_equal(np.asarray(u, object), np.asarray(v, object)) for u, v in zip(x, y))


def test_small_and_empty_inputs(hip_lib):
    model = set_model()
    b, p, l = model.detect(np.zeros((10, 30, 3), np.uint8), landmarks=True)   # smaller than min_face_size: empty pyramid
    assert b is None and p == [None] and l is None
    b, p = model.detect([np.zeros((10, 30, 3), np.uint8), np.zeros((19, 19, 3), np.uint8)])
    assert len(b) == 2 and b[0] is None and b[1] is None and p[0] == [None]


# ------------------------------------------------------------------------------------------------ 8. the job
def test_dataset_job_and_face_stage(hip_lib, tmp_path, monkeypatch):
    from datasets import Dataset
    from PIL import Image
    from oracle import arcface as oa
    from viquae_amd.arcface import ArcFaceR50
    from viquae_amd.data import loading
    from viquae_amd.image import face_detection as fd
    from viquae_amd.image import face_recognition as fr
    s, model = mtcnn_cases.end_to_end_set(), set_model()
    monkeypatch.setattr(loading, "IMAGE_PATH", tmp_path)
    Image.fromarray(s["images"][4]).save(tmp_path / "faces.png")
    Image.fromarray(s["images"][12]).save(tmp_path / "faces.jpg", quality=92)
    Image.fromarray(s["images"][2]).save(tmp_path / "no_face.png")           # ends without a face in the restatement
    Image.fromarray(s["images"][1][:15, :30]).save(tmp_path / "small.png")   # smaller than min_face_size
    (tmp_path / "broken.jpg").write_bytes(b"not an image")
    names = ["faces.png", "broken.jpg", "small.png", "no_face.png", "faces.jpg"]
    with pytest.warns(UserWarning):
        out = fd.dataset_detect_faces(Dataset.from_dict({"image": names}), model=model, batch_size=3)
    assert {"face_prob", "face_box", "face_landmarks"} <= set(out.column_names)
    for k in (1, 2):   # unreadable, too small: None everywhere
        assert out[k]["face_prob"] is None and out[k]["face_box"] is None and out[k]["face_landmarks"] is None
    assert out[3]["face_box"] is None and out[3]["face_landmarks"] is None and out[3]["face_prob"] == [None]
    b, p, l = model.detect(s["images"][4], landmarks=True)
    assert np.array_equal(np.asarray(out[0]["face_box"], np.float32), b) and np.array_equal(np.asarray(out[0]["face_prob"], np.float32), p)
    assert np.array_equal(np.asarray(out[0]["face_landmarks"], np.float32), l) and l.shape[1:] == (5, 2)
    jpg = np.asarray(Image.open(tmp_path / "faces.jpg").convert("RGB"))
    b, p, l = model.detect(jpg, landmarks=True)
    assert (b is None and out[4]["face_box"] is None) or np.array_equal(np.asarray(out[4]["face_box"], np.float32), b)
    # the face stage takes the written column as it is
    arc = ArcFaceR50.from_state_dict(oa.seeded_state(0)).cuda()
    batch = fr.compute_face_embedding({"image": names, "face_landmarks": out["face_landmarks"]}, arc, fr.get_pil_preprocessor(),
                                      fr.SimilarityTransform(), max_n_faces=2)
    emb = batch["face_embedding"]
    assert emb[1] is None and emb[2] is None and emb[3] is None
    assert emb[0].shape == (min(2, len(out[0]["face_box"])), 512) and np.isfinite(emb[0]).all()
