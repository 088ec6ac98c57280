"""The dataset format: a directory of

* ``meta.json``: ``{"classes": C, "mean": [r, g, b], "std": [r, g, b]}`` (0..255 scale);
* per split (``train``, ``val``): ``{split}_images.npy`` uint8 [M, Hs, Ws, 3] and ``{split}_labels.npy`` integer [M].

The arrays are opened with ``np.load(mmap_mode="r")``; labels are checked once, here, against ``classes``.
``k8s_amd.tools.make_dataset`` writes the format.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, List

import numpy as np

SPLITS = ("train", "val")


class DataError(ValueError):
    """A dataset or data configuration problem: permanent, one sentence."""


@dataclass
class Split:
    images: np.ndarray  # uint8 [M, Hs, Ws, 3] (memory map)
    labels: np.ndarray  # int64 [M] (in memory, checked)

    @property
    def nbytes(self) -> int:
        return int(np.prod(self.images.shape))


@dataclass
class Dataset:
    path: str
    classes: int
    mean: List[float]
    std: List[float]
    splits: Dict[str, Split]

    def split(self, name: str) -> Split:
        if name not in self.splits:
            raise DataError("dataset %s has no %s split (%s_images.npy / %s_labels.npy)" % (self.path, name, name,
                                                                                            name))
        return self.splits[name]


def open_dataset(path: str, need=("train",)) -> Dataset:
    """Open ``path``; every split present is mapped and its labels checked, the splits in ``need`` must exist."""
    meta_path = os.path.join(path, "meta.json")
    if not os.path.isfile(meta_path):
        raise DataError("dataset %s has no meta.json" % path)
    try:
        with open(meta_path) as f:
            meta = json.load(f)
        classes = int(meta["classes"])
        mean, std = [float(v) for v in meta["mean"]], [float(v) for v in meta["std"]]
    except (ValueError, KeyError, TypeError) as e:
        raise DataError("dataset %s: meta.json must hold classes, mean and std (%s)" % (path, e)) from e
    if classes < 1 or len(mean) != 3 or len(std) != 3 or min(std) <= 0:
        raise DataError("dataset %s: meta.json needs classes >= 1 and three positive std / three mean values" % path)
    splits = {}
    for name in SPLITS:
        fi, fl = (os.path.join(path, "%s_%s.npy" % (name, k)) for k in ("images", "labels"))
        if not (os.path.isfile(fi) and os.path.isfile(fl)):
            continue
        images = np.load(fi, mmap_mode="r")
        labels = np.load(fl, mmap_mode="r")
        if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3 or images.shape[0] < 1:
            raise DataError("dataset %s: %s_images.npy must be uint8 [M, Hs, Ws, 3]" % (path, name))
        if labels.ndim != 1 or labels.shape[0] != images.shape[0] or not np.issubdtype(labels.dtype, np.integer):
            raise DataError("dataset %s: %s_labels.npy must be an integer [M] matching the images" % (path, name))
        labels = np.array(labels, dtype=np.int64)  # in memory, writable
        if labels.min() < 0 or labels.max() >= classes:
            raise DataError("dataset %s: a %s label lies outside the %d classes of meta.json" % (path, name, classes))
        splits[name] = Split(images, labels)
    ds = Dataset(path, classes, mean, std, splits)
    for name in need:
        ds.split(name)
    return ds


def write_dataset(path: str, classes: int, mean, std, splits: Dict[str, tuple]) -> None:
    """``splits``: name -> (uint8 images [M, Hs, Ws, 3], integer labels [M])."""
    os.makedirs(path, exist_ok=True)
    for name, (images, labels) in splits.items():
        images = np.ascontiguousarray(images, dtype=np.uint8)
        assert images.ndim == 4 and images.shape[3] == 3 and len(labels) == len(images)
        np.save(os.path.join(path, "%s_images.npy" % name), images)
        np.save(os.path.join(path, "%s_labels.npy" % name), np.asarray(labels, dtype=np.int64))
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump({"classes": int(classes), "mean": [float(v) for v in mean], "std": [float(v) for v in std]}, f)
