"""Usage: python -m viquae_amd.image.face_box <dataset> [--image_key=<image_key> --disable_caching]

Mirror of ``meerqat.image.face_box`` (meerqat/image/face_box.py:16-54): scales the ``face_box`` and ``face_landmarks`` columns that
:mod:`viquae_amd.image.face_detection` writes by the image's width and height, and appends width, height and area to every box (the
UNITER format).  Host only; the image's size is read from the file's header, the pixels are never decoded."""
import numpy as np

from ..data import loading


def image_size(file_name):
    """(width, height) from the header of ``IMAGE_PATH / file_name``"""
    from PIL import Image
    with Image.open(loading.IMAGE_PATH / file_name) as image:
        return image.size


def scale_box(item, image_key="image"):
    box = item["face_box"]
    if box is None:
        return item
    w, h = image_size(item[image_key])
    # (n_faces, 4): coordinates are stored as (x1, y1, x2, y2)
    box = np.array(box)
    box[:, 0] /= w
    box[:, 2] /= w
    box[:, 1] /= h
    box[:, 3] /= h
    new_w = box[:, 2] - box[:, 0]
    new_h = box[:, 3] - box[:, 1]
    new_area = new_w * new_h
    item["face_box"] = np.concatenate((box, new_w.reshape(-1, 1), new_h.reshape(-1, 1), new_area.reshape(-1, 1)), axis=1)
    landmarks = item.get("face_landmarks")
    if landmarks is not None:
        landmarks = np.array(landmarks)
        landmarks[:, :, 0] /= w
        landmarks[:, :, 1] /= h
        item["face_landmarks"] = landmarks
    return item


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="scale face boxes and landmarks by the image size (python -m meerqat.image.face_box)")
    ap.add_argument("dataset")
    ap.add_argument("--image_key", default="image")
    ap.add_argument("--disable_caching", action="store_true")
    a = ap.parse_args()
    import datasets
    from .embedding import _save
    if a.disable_caching:
        datasets.disable_caching()
    dataset = datasets.load_from_disk(a.dataset)
    _save(dataset.map(scale_box, fn_kwargs=dict(image_key=a.image_key)), a.dataset, a.dataset)
