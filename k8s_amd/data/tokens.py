"""The token dataset format (``dataset.py`` is the image format): a directory of

* ``meta.json``: ``{"kind": "tokens", "vocab": V, "pad": id, "cls": id, "sep": id, "mask": id}`` -- a meta without
  ``kind`` is an image dataset; a causal LM needs only ``kind`` and ``vocab``;
* per split (``train``, ``val``): ``{split}_tokens.npy`` 1-D uint16 (``V <= 65536``) or int32 [T];
  ``{split}_segments.npy`` int64 [G + 1], strictly ascending token offsets from 0 to T (a segment is the unit the
  writer chose: a sentence, or several); ``{split}_docs.npy`` int64 [D + 1], strictly ascending segment indices from
  0 to G. Segments and documents are what BERT's sentence pairs need (``D >= 2``); a causal LM reads the token
  stream alone.

The arrays are opened with ``np.load(mmap_mode="r")`` and checked once, here. ``k8s_amd.tools.make_dataset
--toy-tokens`` writes the format.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from k8s_amd.data.dataset import SPLITS, DataError

SPECIAL = ("pad", "cls", "sep", "mask")
_CHUNK = 1 << 24  # tokens per step of the max over the map


def dataset_kind(path: str) -> str:
    """"tokens" or "images": what ``path``'s meta.json says it holds (no ``kind``: images)."""
    meta_path = os.path.join(path, "meta.json")
    if not os.path.isfile(meta_path):
        raise DataError("dataset %s has no meta.json" % path)
    try:
        with open(meta_path) as f:
            meta = json.load(f)
        kind = meta.get("kind", "images")
    except (ValueError, AttributeError) as e:
        raise DataError("dataset %s: meta.json is not a JSON object (%s)" % (path, e)) from e
    if kind not in ("tokens", "images"):
        raise DataError("dataset %s: meta.json has the unknown kind %r" % (path, kind))
    return kind


@dataclass
class TokenSplit:
    tokens: np.ndarray                 # uint16 or int32 [T] (memory map)
    segments: Optional[np.ndarray]     # int64 [G + 1] (in memory, checked) or None
    docs: Optional[np.ndarray]         # int64 [D + 1] (in memory, checked) or None

    @property
    def T(self) -> int:
        return int(self.tokens.shape[0])

    @property
    def G(self) -> int:
        return 0 if self.segments is None else len(self.segments) - 1

    @property
    def D(self) -> int:
        return 0 if self.docs is None else len(self.docs) - 1

    @property
    def nbytes(self) -> int:
        return int(self.tokens.nbytes)


@dataclass
class TokenDataset:
    path: str
    vocab: int
    special: Optional[tuple]  # (pad, cls, sep, mask), None when the meta names none (causal LM data)
    splits: Dict[str, TokenSplit]

    def split(self, name: str) -> TokenSplit:
        if name not in self.splits:
            raise DataError("dataset %s has no %s split (%s_tokens.npy)" % (self.path, name, name))
        return self.splits[name]


def _offsets(path: str, name: str, what: str, last: int, last_name: str) -> np.ndarray:
    arr = np.load(path, mmap_mode="r")
    if arr.dtype != np.int64 or arr.ndim != 1 or arr.shape[0] < 2:
        raise DataError("dataset %s: %s_%s.npy must be int64 [n + 1] with n >= 1" % (os.path.dirname(path), name, what))
    arr = np.array(arr)
    if arr[0] != 0 or arr[-1] != last or not bool(np.all(np.diff(arr) > 0)):
        raise DataError("dataset %s: %s_%s.npy must ascend strictly from 0 to %s = %d"
                        % (os.path.dirname(path), name, what, last_name, last))
    return arr


def open_token_dataset(path: str, need=("train",), pairs: bool = False) -> TokenDataset:
    """Open ``path``; every split present is mapped and checked, the splits in ``need`` must exist. ``pairs``: the
    reader builds sentence pairs (BERT), so the special ids, segments and at least two documents are required."""
    if dataset_kind(path) != "tokens":
        raise DataError("dataset %s holds images, not tokens (its meta.json has no \"kind\": \"tokens\")" % path)
    with open(os.path.join(path, "meta.json")) as f:
        meta = json.load(f)
    try:
        vocab = int(meta["vocab"])
        special = tuple(int(meta[k]) for k in SPECIAL) if any(k in meta for k in SPECIAL) or pairs else None
    except (ValueError, KeyError, TypeError) as e:
        raise DataError("dataset %s: meta.json must hold vocab%s (%s)"
                        % (path, " and the pad, cls, sep and mask ids" if pairs else "", e)) from e
    if not 2 <= vocab <= 2 ** 31 - 1:
        raise DataError("dataset %s: vocab must be in [2, 2^31 - 1], got %d" % (path, vocab))
    if special is not None and (len(set(special)) != 4 or min(special) < 0 or max(special) >= vocab):
        raise DataError("dataset %s: the pad, cls, sep and mask ids %s must be distinct and below vocab = %d"
                        % (path, special, vocab))
    splits = {}
    for name in SPLITS:
        ft, fs, fd = (os.path.join(path, "%s_%s.npy" % (name, k)) for k in ("tokens", "segments", "docs"))
        if not os.path.isfile(ft):
            continue
        tokens = np.load(ft, mmap_mode="r")
        if tokens.dtype not in (np.uint16, np.int32) or tokens.ndim != 1 or tokens.shape[0] < 2:
            raise DataError("dataset %s: %s_tokens.npy must be a 1-D uint16 or int32 array" % (path, name))
        if tokens.dtype == np.uint16 and vocab > 65536:
            raise DataError("dataset %s: uint16 tokens cannot hold vocab = %d (> 65536)" % (path, vocab))
        T = int(tokens.shape[0])
        lo, hi = 0, 0
        for at in range(0, T, _CHUNK):  # bounded reads of the map
            part = tokens[at:at + _CHUNK]
            lo, hi = min(lo, int(part.min())), max(hi, int(part.max()))
        if lo < 0 or hi >= vocab:
            raise DataError("dataset %s: a %s token lies outside the vocab = %d of meta.json" % (path, name, vocab))
        segments = docs = None
        if os.path.isfile(fs):
            segments = _offsets(fs, name, "segments", T, "T")
            if os.path.isfile(fd):
                docs = _offsets(fd, name, "docs", len(segments) - 1, "G")
        if pairs and (segments is None or docs is None or len(docs) - 1 < 2):
            raise DataError("dataset %s: sentence pairs need %s_segments.npy and %s_docs.npy with at least two "
                            "documents" % (path, name, name))
        splits[name] = TokenSplit(tokens, segments, docs)
    ds = TokenDataset(path, vocab, special, splits)
    for name in need:
        ds.split(name)
    return ds


def write_token_dataset(path: str, vocab: int, splits: Dict[str, tuple], special: Optional[dict] = None) -> None:
    """``splits``: name -> (tokens [T], segments [G + 1] or None, docs [D + 1] or None); tokens are stored as uint16
    when ``vocab <= 65536``, else int32. ``special``: {"pad", "cls", "sep", "mask"} or None."""
    os.makedirs(path, exist_ok=True)
    dtype = np.uint16 if vocab <= 65536 else np.int32
    for name, (tokens, segments, docs) in splits.items():
        np.save(os.path.join(path, "%s_tokens.npy" % name), np.ascontiguousarray(tokens, dtype=dtype))
        if segments is not None:
            np.save(os.path.join(path, "%s_segments.npy" % name), np.asarray(segments, dtype=np.int64))
        if docs is not None:
            np.save(os.path.join(path, "%s_docs.npy" % name), np.asarray(docs, dtype=np.int64))
    meta = {"kind": "tokens", "vocab": int(vocab)}
    meta.update({k: int(special[k]) for k in SPECIAL} if special else {})
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump(meta, f)
