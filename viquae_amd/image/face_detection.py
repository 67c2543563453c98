"""Usage: python -m viquae_amd.image.face_detection <dataset> [<model_config> --save=<root_path> --image_key=<image_key>
--disable_caching --batch_size=<n>]

Mirror of ``meerqat.image.face_detection`` (meerqat/image/face_detection.py): MTCNN face detection writing ``face_prob``,
``face_box`` and ``face_landmarks`` into a dataset, ahead of :mod:`viquae_amd.image.face_recognition`.

Same names and call shapes as the reference:

* ``MTCNN(image_size, margin, min_face_size, thresholds, factor, post_process, select_largest, selection_method, keep_all, device)``
  with ``detect``, ``select_boxes`` and the reference's ``forward`` override                                   :26-84
* ``detect_face(file_names, model, save_root_path=None)``                                                         :87-139
* ``dataset_detect_face`` / ``dataset_detect_faces``                                                              :142-152
* the command line with the reference's default model config                                                      :155-186

What differs underneath: the reference runs ``facenet_pytorch`` (three small CNNs through generic convolutions, one host round
trip per pyramid scale, images grouped by size); here the whole batch -- mixed sizes welcome, no image's result depends on its
neighbours -- runs through csrc/mtcnn.hip: one resampling launch for every scale of every image, a fused P-Net that only emits the
cells that pass, NMS / box refinement / crops / R-Net / O-Net as one launch per stage.  The host reads four per-stage count vectors
and the final lists per batch (:data:`HOST_READS_PER_BATCH`; one more per capacity retry).

Not built (``NotImplementedError``): ``extract`` and saving crops (``save_path``, ``save_root_path`` / ``--save``) -- the face stage
aligns from landmarks and never reads the crops -- and the ``center_weighted_size`` / ``largest_over_threshold`` selection methods.

Weights: three local state dicts ``pnet.pt``, ``rnet.pt``, ``onet.pt`` under facenet_pytorch's key names (the files of its
``facenet_pytorch/data`` directory), from ``weights=<directory>`` or ``MQ_MTCNN_WEIGHTS``; or ``weights=<dict of the three state
dicts>``.  Nothing is downloaded.  facenet_pytorch is not installable here: parity on the published checkpoints is unpinned
(tests/mtcnn_restatement.py restates the published algorithm; tools/mtcnn_compare.py)."""
import os
from pathlib import Path

import numpy as np

from ..data import loading

NETS = ("pnet", "rnet", "onet")
# (key, shape) in packing order; "dense" rows are re-ordered (see pack_weights)
_LAYOUT = {
    "pnet": [("conv1", (10, 3, 3, 3), True), ("conv2", (16, 10, 3, 3), True), ("conv3", (32, 16, 3, 3), True),
             ("conv4_1", (2, 32, 1, 1), False), ("conv4_2", (4, 32, 1, 1), False)],
    "rnet": [("conv1", (28, 3, 3, 3), True), ("conv2", (48, 28, 3, 3), True), ("conv3", (64, 48, 2, 2), True),
             ("dense4", (128, 576), True), ("dense5_1", (2, 128), False), ("dense5_2", (4, 128), False)],
    "onet": [("conv1", (32, 3, 3, 3), True), ("conv2", (64, 32, 3, 3), True), ("conv3", (64, 64, 3, 3), True),
             ("conv4", (128, 64, 2, 2), True), ("dense5", (256, 1152), True), ("dense6_1", (2, 256), False),
             ("dense6_2", (4, 256), False), ("dense6_3", (10, 256), False)],
}
_FLATTENED = {"dense4": (64, 3, 3), "dense5": (128, 3, 3)}  # (C, H, W) of the map in front of the dense layer
# blocking device-to-host reads of one batch: P-Net counts (+ both overflow flags), counts after the two P-Net NMS sites, after the
# R-Net NMS, after the O-Net NMS (+ the buffer flag), the final lists; one more per capacity retry, two more with trace=True
HOST_READS_PER_BATCH = 5
STAGES = ("pnet", "nms1", "nms2", "rnet", "nms3", "onet", "nms4")


def load_state_dicts(weights=None):
    """-> {"pnet": sd, "rnet": sd, "onet": sd} of numpy arrays from a dict (returned as numpy) or a directory holding the three
    ``.pt`` files (``weights`` or ``MQ_MTCNN_WEIGHTS``)."""
    if isinstance(weights, dict):
        return {net: {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v) for k, v in weights[net].items()}
                for net in NETS}
    directory = weights if weights is not None else os.environ.get("MQ_MTCNN_WEIGHTS")
    if directory is None:
        raise FileNotFoundError("MTCNN weights: pass weights=<directory or dict> or set MQ_MTCNN_WEIGHTS to a directory holding "
                                "pnet.pt, rnet.pt and onet.pt; copy the three files from facenet_pytorch/data/ of an installed "
                                "facenet_pytorch package (nothing is downloaded)")
    import torch
    out = {}
    for net in NETS:
        path = Path(directory) / f"{net}.pt"
        if not path.exists():
            raise FileNotFoundError(f"{path} is missing: copy pnet.pt, rnet.pt and onet.pt from facenet_pytorch/data/ of an installed "
                                    f"facenet_pytorch package into {directory} (nothing is downloaded)")
        out[net] = {k: v.numpy() for k, v in torch.load(path, map_location="cpu", weights_only=True).items()}
    return out


def pack_weights(state):
    """One float32 vector per network in the layout of include/meerqat_hip.h: per layer weight, bias, PReLU slope.  The dense layers
    behind a flatten are stored [in][out] with ``in`` in (c, y, x) order: the published forward flattens ``x.permute(0, 3, 2, 1)``,
    i.e. input feature ``(x * H + y) * C + c`` -- that permutation is applied here, once."""
    packed = {}
    for net in NETS:
        sd, parts = state[net], []
        for i, (name, shape, has_prelu) in enumerate(_LAYOUT[net]):
            w = np.asarray(sd[name + ".weight"], np.float32)
            if tuple(w.shape) != shape:
                raise ValueError(f"{net}.{name}.weight has shape {tuple(w.shape)}, expected {shape}")
            if name in _FLATTENED:
                C, H, W = _FLATTENED[name]
                c, y, x = np.meshgrid(np.arange(C), np.arange(H), np.arange(W), indexing="ij")
                w = np.ascontiguousarray(w[:, ((x * H + y) * C + c).reshape(-1)].T)
            parts.append(w.reshape(-1))
            parts.append(np.asarray(sd[name + ".bias"], np.float32).reshape(-1))
            if has_prelu:
                prelu = "prelu" + "".join(ch for ch in name if ch.isdigit())  # conv1 -> prelu1, dense4 -> prelu4
                parts.append(np.asarray(sd[prelu + ".weight"], np.float32).reshape(-1))
                if parts[-1].size != shape[0]:
                    raise ValueError(f"{net}.{prelu}.weight has {parts[-1].size} slopes, expected {shape[0]}")
        packed[net] = np.concatenate(parts)
    return packed


def scale_pyramid(h, w, min_face_size, factor):
    """The published scale rule: m = 12 / min_face_size, multiplied by factor while min(h, w) * scale >= 12."""
    m = 12.0 / min_face_size
    minl = min(h, w) * m
    scale_i, scales = m, []
    while minl >= 12:
        scales.append(scale_i)
        scale_i = scale_i * factor
        minl = minl * factor
    return scales


def _to_arrays(img):
    """-> (list of uint8 [H, W, 3] arrays, whether the input was a batch)"""
    if isinstance(img, (list, tuple)):
        return [np.asarray(i, np.uint8) for i in img], True
    if isinstance(img, np.ndarray) and img.ndim == 4:
        return [np.asarray(i, np.uint8) for i in img], True
    return [np.asarray(img, np.uint8)], False


def _object_array(items):
    out = np.empty(len(items), dtype=object)
    for i, item in enumerate(items):
        out[i] = item
    return out


class MTCNN:
    """``facenet_pytorch.MTCNN`` by signature, the detector on the device.  ``weights``: see :func:`load_state_dicts`.
    ``candidate_capacity``: first size of the per-image candidate lists (grown and the stage repeated when P-Net overflows it)."""

    def __init__(self, image_size=160, margin=0, min_face_size=20, thresholds=[0.6, 0.7, 0.7], factor=0.709, post_process=True,
                 select_largest=True, selection_method=None, keep_all=False, device=None, weights=None, candidate_capacity=4096):
        import torch
        from .. import _lib
        self.image_size, self.margin, self.min_face_size = image_size, margin, min_face_size
        self.thresholds, self.factor, self.post_process = list(thresholds), factor, post_process
        self.select_largest, self.keep_all = select_largest, keep_all
        self.selection_method = selection_method or ("largest" if select_largest else "probability")
        self.candidate_capacity = int(candidate_capacity)
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise _lib.MeerqatHipError("viquae_amd face detection runs on MI355X only (no CPU fallback)")
        lib = _lib.load()
        packed = pack_weights(load_state_dicts(weights))
        for i, net in enumerate(NETS):
            if packed[net].size != lib.mq_mtcnn_weight_floats(i):
                raise ValueError(f"{net}: {packed[net].size} packed weights, the library expects {lib.mq_mtcnn_weight_floats(i)}")
        self._w = {net: torch.from_numpy(packed[net]).to(self.device) for net in NETS}
        self.last_counts = None   # [n_images][stage] of the last batch (STAGES order; "rnet" / "onet" only with trace=True, which
        #                           costs two more host reads per batch: tests and tools only)
        self.retries = 0
        self.trace = False
        self.stage_events = None  # a list: _detect_arrays appends (stage name, CUDA event) marks (tools/mtcnn_timing.py)

    # ------------------------------------------------------------------ the device path
    def _detect_arrays(self, arrays):
        """list of uint8 [H, W, 3] arrays (any sizes) -> per image (boxes [n, 5] float32, points [n, 5, 2] float32), in the order
        the last NMS leaves."""
        import torch
        from .. import _lib
        lib, dev = _lib.load(), self.device
        B = len(arrays)
        empty = (np.zeros((0, 5), np.float32), np.zeros((0, 5, 2), np.float32))
        counts = np.zeros((B, len(STAGES)), np.int64)
        self.last_counts = counts
        if B == 0:
            return []
        offsets, hw, total = np.zeros(B, np.int64), np.zeros((B, 2), np.int32), 0
        for i, a in enumerate(arrays):
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("expected RGB images [H, W, 3]")
            offsets[i], hw[i] = total, a.shape[:2]
            total += a.size
        packed = np.empty(max(total, 1), np.uint8)
        for a, o in zip(arrays, offsets):
            packed[o:o + a.size] = np.ascontiguousarray(a).reshape(-1)
        # the pyramid: every level of every image
        jobs, levels, scales, in_off, max_tiles, max_pixels, max_cells = [], [], [], 0, 1, 1, 1
        for b, (h, w) in enumerate(hw.tolist()):
            cell_base = 0
            for k, s in enumerate(scale_pyramid(h, w, self.min_face_size, self.factor) if min(h, w) >= 1 else []):
                hs, ws = int(h * s + 1), int(w * s + 1)
                ho, wo = (hs - 3) // 2 + 1 - 4, (ws - 3) // 2 + 1 - 4
                jobs.append((b, 0, 0, w, h, ws, hs, in_off))
                levels.append((in_off, hs, ws, b, k, cell_base, 0, 0))
                scales.append(s)
                in_off += 3 * hs * ws
                cell_base += ho * wo
                max_tiles = max(max_tiles, -(-ho // 16) * -(-wo // 16))
                max_pixels = max(max_pixels, hs * ws)
            max_cells = max(max_cells, cell_base)
        if not levels:
            return [empty] * B
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            img_d, off_d, hw_d = t(packed), t(offsets), t(hw.reshape(-1))
            overflow = torch.zeros(1, dtype=torch.int32, device=dev)       # P-Net's candidate lists: cleared by every P-Net call
            buffer_over = torch.zeros(1, dtype=torch.int32, device=dev)    # pyramid and crop buffers: never cleared

            def resample(jobs_d, n_jobs, pixels, out):
                _lib.check(lib.mq_mtcnn_resample_u8_f32(ptr(img_d), ptr(off_d), ptr(hw_d), B, ptr(jobs_d), n_jobs, pixels, ptr(out),
                                                        out.numel(), ptr(buffer_over), stream), "mq_mtcnn_resample_u8_f32")

            def nms(rec, seg_start, seg_count, key, sub, score_gt, thr, mode, want_key=False, want_src=False, seg_cap=0):
                n_total = rec.shape[0]
                out_rec, out_count = torch.empty_like(rec), i32(B)
                out_key = i32(n_total) if want_key else None
                out_src = i32(n_total) if want_src else None
                ws_bytes = lib.mq_mtcnn_nms_workspace_bytes(n_total)
                ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
                _lib.check(lib.mq_mtcnn_nms_f32(ptr(rec), n_total, ptr(seg_start), ptr(seg_count), B, seg_cap, ptr(key), ptr(sub), score_gt, thr,
                                                mode, ptr(out_rec), ptr(out_key), None, ptr(out_src), ptr(out_count), ptr(ws), ws_bytes,
                                                stream), "mq_mtcnn_nms_f32")
                return out_rec, out_key, out_src, out_count

            def refine(in_rec, seg_start, count_host, flags, crop):
                """-> (rec, valid, crops, dst prefix on the device, dst prefix on the host)"""
                dst = np.zeros(B + 1, np.int64)
                np.cumsum(count_host, out=dst[1:])
                M = int(dst[-1])
                dst_d = t(dst)
                rec, img, pad, job, valid = f32(M, 9), i32(M), i32(M, 4), torch.empty((M, 8), dtype=torch.int64, device=dev), i32(M)
                crops = f32(M, 3, crop, crop)
                _lib.check(lib.mq_mtcnn_refine_f32(ptr(in_rec), ptr(seg_start), ptr(dst_d), B, M, ptr(hw_d), flags, crop, M, ptr(rec),
                                                   ptr(img), ptr(pad), ptr(job), ptr(valid), ptr(buffer_over), stream), "mq_mtcnn_refine_f32")
                resample(job, M, crop * crop, crops)
                return rec, img, valid, crops, dst_d, dst

            def mark(name):
                if self.stage_events is not None:
                    event = torch.cuda.Event(enable_timing=True)
                    event.record(torch.cuda.current_stream(dev))
                    self.stage_events.append((name, event))

            mark("start")
            pyramid = f32(in_off)
            resample(t(np.asarray(jobs, np.int64)), len(jobs), max_pixels, pyramid)
            mark("pyramid")
            levels_d, scales_d = t(np.asarray(levels, np.int64)), t(np.asarray(scales, np.float32))
            cap = max(1, min(self.candidate_capacity, max_cells))
            while True:
                rec0, idx0, sub0, count0 = f32(B * cap, 9), i32(B * cap), i32(B * cap), i32(B)
                _lib.check(lib.mq_mtcnn_pnet_f32(ptr(pyramid), in_off, ptr(levels_d), ptr(scales_d), len(levels), max_tiles,
                                                 ptr(self._w["pnet"]), float(self.thresholds[0]), B, cap, ptr(rec0), ptr(idx0), ptr(sub0),
                                                 ptr(count0), ptr(overflow), None, 0, stream), "mq_mtcnn_pnet_f32")
                head = torch.cat([count0, overflow, buffer_over]).cpu().numpy()                      # host read 1
                if head[-1]:  # the pyramid buffer is sized from the same level table: a broken invariant, not a retry
                    raise _lib.MeerqatHipError("MTCNN: the pyramid buffer overflowed")
                if not head[-2]:
                    break
                cap, self.retries = int(head[:-2].max()), self.retries + 1                           # the counters say how much
            counts[:, 0] = head[:-2]
            mark("pnet")
            seg0 = t(np.arange(B, dtype=np.int64) * cap)
            ninf = float("-inf")
            rec1, key1, _, count1 = nms(rec0, seg0, count0, idx0, sub0, ninf, 0.5, 0, want_key=True, seg_cap=cap)
            rec2, _, _, count2 = nms(rec1, seg0, count1, key1, None, ninf, 0.7, 0, seg_cap=cap)
            c12 = torch.stack([count1, count2]).cpu().numpy()                                        # host read 2
            mark("nms1+nms2")
            counts[:, 1], counts[:, 2] = c12[0], c12[1]
            if c12[1].sum() == 0:
                return [empty] * B
            recr, imgr, validr, crops, dstr_d, dstr = refine(rec2, seg0, c12[1], 2, 24)
            _lib.check(lib.mq_mtcnn_rnet_f32(ptr(crops), recr.shape[0], ptr(self._w["rnet"]), ptr(validr), ptr(recr), stream),
                       "mq_mtcnn_rnet_f32")
            mark("refine+crops24+rnet")
            if self.trace:
                counts[:, 3] = torch.bincount(imgr[recr[:, 4] > float(self.thresholds[1])].long(), minlength=B).cpu().numpy()
            rec3, _, _, count3 = nms(recr, dstr_d, count2, None, None, float(self.thresholds[1]), 0.7, 0)
            c3 = count3.cpu().numpy()                                                                # host read 3
            mark("nms3")
            counts[:, 4] = c3
            if c3.sum() == 0:
                return [empty] * B
            reco, imgo, valido, crops, dsto_d, dsto = refine(rec3, dstr_d, c3, 3, 48)
            pts = f32(reco.shape[0], 10)
            _lib.check(lib.mq_mtcnn_onet_f32(ptr(crops), reco.shape[0], ptr(self._w["onet"]), ptr(valido), ptr(reco), ptr(pts), 1, stream),
                       "mq_mtcnn_onet_f32")
            mark("refine+crops48+onet")
            if self.trace:
                counts[:, 5] = torch.bincount(imgo[reco[:, 4] > float(self.thresholds[2])].long(), minlength=B).cpu().numpy()
            rec4, _, src4, count4 = nms(reco, dsto_d, count3, None, None, float(self.thresholds[2]), 0.7, 1, want_src=True)
            tail = torch.cat([count4, buffer_over]).cpu().numpy()                                    # host read 4
            mark("nms4")
            c4 = tail[:-1]
            counts[:, 6] = c4
            if tail[-1]:  # a crop buffer sized from the counts above cannot overflow: a broken invariant, not a retry
                raise _lib.MeerqatHipError("MTCNN: a crop buffer overflowed")
            # host read 5, the final lists in one copy: kept records, every crop's landmarks, the kept records' crop positions
            final = torch.cat([rec4, pts, src4.to(torch.float32).unsqueeze(1)], dim=1).cpu().numpy()
            rec4_h, pts_h, src4_h = final[:, :9], final[:, 9:19], final[:, 19].astype(np.int64)
        out = []
        for b in range(B):
            s0, n = int(dsto[b]), int(c4[b])
            if n == 0:
                out.append(empty)
                continue
            p = pts_h[s0 + src4_h[s0:s0 + n]]
            out.append((rec4_h[s0:s0 + n, :5].copy(), np.stack([p[:, :5], p[:, 5:]], axis=2)))
        return out

    # ------------------------------------------------------------------ the published surface
    def detect(self, img, landmarks=False):
        """PIL image, uint8 [H, W, 3] array or a list of them (any sizes) -> (boxes, probs[, points]): per image an [n, 4] float32
        array (x1, y1, x2, y2), [n] probabilities and [n, 5, 2] landmarks; (None, [None], None) for an image without faces.  A
        list gives object arrays of these, a single image the entries themselves."""
        arrays, batch_mode = _to_arrays(img)
        boxes, probs, points = [], [], []
        for box, point in self._detect_arrays(arrays):
            if len(box) == 0:
                boxes.append(None), probs.append([None]), points.append(None)
                continue
            if self.select_largest:
                order = np.argsort((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1]))[::-1]
                box, point = box[order], point[order]
            boxes.append(box[:, :4]), probs.append(box[:, 4]), points.append(point)
        boxes, probs, points = _object_array(boxes), _object_array(probs), _object_array(points)
        if not batch_mode:
            boxes, probs, points = boxes[0], probs[0], points[0]
        return (boxes, probs, points) if landmarks else (boxes, probs)

    def select_boxes(self, all_boxes, all_probs, all_points, imgs, method="probability", threshold=0.9, center_weight=2.0):
        """The published selection of one face per image, on the host: ``"probability"`` or ``"largest"``."""
        if method not in ("probability", "largest"):
            raise NotImplementedError(f"select_boxes(method={method!r}) is not built: 'probability' and 'largest' are")
        batch_mode = isinstance(imgs, (list, tuple)) or (isinstance(imgs, np.ndarray) and imgs.ndim == 4)
        if not batch_mode:
            all_boxes, all_probs, all_points = [all_boxes], [all_probs], [all_points]
        sel_boxes, sel_probs, sel_points = [], [], []
        for boxes, points, probs in zip(all_boxes, all_points, all_probs):
            if boxes is None:
                sel_boxes.append(None), sel_probs.append([None]), sel_points.append(None)
                continue
            boxes, probs, points = np.array(boxes), np.array(probs), np.array(points)
            if method == "largest":
                order = np.argsort((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))[::-1]
            else:
                order = np.argsort(probs)[::-1]
            sel_boxes.append(boxes[order][[0]]), sel_probs.append(probs[order][[0]]), sel_points.append(points[order][[0]])
        if batch_mode:
            return _object_array(sel_boxes), _object_array(sel_probs), _object_array(sel_points)
        return sel_boxes[0], sel_probs[0], sel_points[0]

    def extract(self, img, batch_boxes, save_path):
        raise NotImplementedError("face crops are not built: the face stage (viquae_amd.image.face_recognition) aligns from landmarks")

    def forward(self, img, save_path=None, return_prob=False, return_box=False, return_landmarks=False):
        """The reference's override (:28-84): detect, select unless ``keep_all``, return the asked lists.  The first output, the
        face crops, is always None here and a ``save_path`` is refused (see :meth:`extract`)."""
        if save_path is not None:
            raise NotImplementedError("saving face crops is not built: the face stage aligns from landmarks")
        batch_boxes, batch_probs, batch_points = self.detect(img, landmarks=True)
        if not self.keep_all:
            batch_boxes, batch_probs, batch_points = self.select_boxes(batch_boxes, batch_probs, batch_points, img,
                                                                       method=self.selection_method)
        outputs = (None, )
        if return_prob:
            outputs += (batch_probs, )
        if return_box:
            outputs += (batch_boxes, )
        if return_landmarks:
            outputs += (batch_points, )
        return outputs[0] if len(outputs) == 1 else outputs

    __call__ = forward


def detect_face(file_names, model, save_root_path=None):
    """:87-139.  Unreadable images and images smaller than ``model.min_face_size`` keep None in all three lists.  The reference
    groups the images by size for its batched model; here the readable ones go through one mixed batch (same results)."""
    if save_root_path is not None:
        raise NotImplementedError("saving face crops (--save / save_root_path) is not built: the face stage aligns from landmarks")
    images = loading.load_image_batch(file_names)
    kept, indices = [], []
    for i, image in enumerate(images):
        if image is None or min(image.size) < model.min_face_size:
            continue
        kept.append(image)
        indices.append(i)
    prob_batch = [None for _ in range(len(file_names))]
    box_batch, landmarks_batch = prob_batch.copy(), prob_batch.copy()
    if not kept:
        return prob_batch, box_batch, landmarks_batch
    boxes, probs, landmarks = model.detect(kept, landmarks=True)
    if not model.keep_all:
        boxes, probs, landmarks = model.select_boxes(boxes, probs, landmarks, kept, method=model.selection_method)
    for prob, box, landmark, i in zip(probs, boxes, landmarks, indices):
        prob_batch[i] = prob.tolist() if isinstance(prob, np.ndarray) else prob
        box_batch[i] = box.tolist() if box is not None and isinstance(box, np.ndarray) else box
        landmarks_batch[i] = landmark.tolist() if landmark is not None and isinstance(landmark, np.ndarray) else landmark
    return prob_batch, box_batch, landmarks_batch


def dataset_detect_face(item, image_key="image", **kwargs):
    prob, box, landmarks = detect_face(item[image_key], **kwargs)
    item["face_prob"] = prob
    item["face_box"] = box
    item["face_landmarks"] = landmarks
    return item


def dataset_detect_faces(dataset, batch_size=64, **kwargs):
    """:150-152 (a random fingerprint: the model is never pickled for a hash)."""
    from datasets.fingerprint import generate_random_fingerprint
    return dataset.map(dataset_detect_face, batched=True, fn_kwargs=kwargs, batch_size=batch_size,
                       new_fingerprint=generate_random_fingerprint())


if __name__ == "__main__":
    import argparse
    import json
    ap = argparse.ArgumentParser(description="MTCNN face detection over a dataset (python -m meerqat.image.face_detection <dataset> "
                                             "[<model_config>] [--image_key=] [--disable_caching] [--batch_size=])")
    ap.add_argument("dataset")
    ap.add_argument("model_config", nargs="?")
    ap.add_argument("--save")
    ap.add_argument("--image_key", default="image")
    ap.add_argument("--disable_caching", action="store_true")
    ap.add_argument("--batch_size", type=int, default=64)
    a = ap.parse_args()
    if a.save is not None:
        raise NotImplementedError("--save (face crops) is not built: the face stage aligns from landmarks")
    import datasets
    from ..utils import device
    from .embedding import _save
    if a.disable_caching:
        datasets.disable_caching()
    # the reference's default config (:164-170)
    model_config = dict(image_size=112, post_process=False, select_largest=False, keep_all=True, device=device)
    if a.model_config is not None:
        with open(a.model_config, "r") as file:
            model_config.update(json.load(file))
    dataset = datasets.load_from_disk(a.dataset)
    dataset = dataset_detect_faces(dataset, model=MTCNN(**model_config), image_key=a.image_key, save_root_path=None,
                                   batch_size=a.batch_size)
    _save(dataset, a.dataset, a.dataset)
