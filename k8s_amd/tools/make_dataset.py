"""Write a dataset directory in the trainer's format (``k8s_amd.data.dataset``). Nothing is downloaded.

    python -m k8s_amd.tools.make_dataset --out DIR --toy [--seed 0] [--train 2048] [--val 256] [--classes 10]
                                                   [--size 40]
    python -m k8s_amd.tools.make_dataset --out DIR --cifar10-batches DIR_WITH_PICKLES
    python -m k8s_amd.tools.make_dataset --out DIR --toy-tokens [--seed 0] [--train-docs 512] [--val-docs 64]
                                                   [--vocab 512] [--segments-per-doc 2 6]
                                                   [--tokens-per-segment 4 12]

``--toy``: a learnable set that is a pure function of its seed. Class k is a fixed random 5x5x3 uint8 prototype
(numpy Philox key 7, the same for every seed) upscaled to ``--size`` (x8 to 40x40 by default, nearest cell at other
sizes); Gaussian noise of sigma 48 is added and the result clipped to uint8; labels are uniform. meta: mean 127.5, std 64.

``--toy-tokens``: a learnable token set (``k8s_amd.data.tokens``) that is a pure function of its seed, for the BERT
and Llama models. Specials pad 0, cls 1, sep 2, mask 3; 8 topics, topic k owning the ids 8 + 63 k .. 8 + 63 k + 62. A
document draws one topic, 2 to 6 segments (``--segments-per-doc LO HI``) and 4 to 12 tokens per segment
(``--tokens-per-segment LO HI``; the defaults leave the files unchanged); a segment's first token is uniform in the
topic's slice and each later one is ``base + (5 * prev_off + 1) mod 63`` with probability 0.9, else uniform in the
slice.

``--cifar10-batches``: the CIFAR-10 "python version" pickles (``data_batch_1..5`` -> train, ``test_batch`` -> val; keys
``data`` [10000, 3072] CHW uint8 and ``labels``) converted to NHWC, with CIFAR-10's per-channel mean and std.
"""
from __future__ import annotations

import argparse
import os
import pickle
import sys

import numpy as np

from k8s_amd.data.dataset import write_dataset
from k8s_amd.data.tokens import write_token_dataset

TOY_PROTO_KEY, TOY_SIGMA = 7, 48.0
CIFAR10_MEAN, CIFAR10_STD = [125.3, 123.0, 113.9], [63.0, 62.1, 66.7]


def toy_prototypes(classes: int) -> np.ndarray:
    """uint8 [classes, 5, 5, 3]: the first ``classes`` prototypes of the one fixed stream."""
    g = np.random.Generator(np.random.Philox(key=TOY_PROTO_KEY))
    return g.integers(0, 256, size=(classes, 5, 5, 3), dtype=np.uint8)


def toy_split(seed: int, which: int, n: int, classes: int, size: int = 40):
    """(uint8 images [n, size, size, 3], int64 labels [n]) of split number ``which`` for ``seed``."""
    if size < 5:
        raise ValueError("--size must be at least 5 (the prototypes are 5x5)")
    g = np.random.Generator(np.random.Philox(np.random.SeedSequence([0x70F, int(seed), int(which)])))
    labels = g.integers(0, classes, size=n, dtype=np.int64)
    cell = np.arange(size) * 5 // size  # nearest prototype cell: x8 blocks at the default 40
    up = toy_prototypes(classes)[:, cell][:, :, cell]
    images = np.empty((n, size, size, 3), dtype=np.uint8)
    for at in range(0, n, 256):  # bounded temporaries at large sizes
        lab = labels[at:at + 256]
        noise = g.normal(0.0, TOY_SIGMA, size=(len(lab), size, size, 3))
        images[at:at + 256] = np.clip(np.rint(up[lab].astype(np.float64) + noise), 0, 255).astype(np.uint8)
    return images, labels


def make_toy(out: str, seed: int = 0, train: int = 2048, val: int = 256, classes: int = 10, size: int = 40) -> None:
    write_dataset(out, classes, [127.5] * 3, [64.0] * 3,
                  {"train": toy_split(seed, 0, train, classes, size), "val": toy_split(seed, 1, val, classes, size)})


TOY_TOPICS, TOY_SLICE, TOY_FIRST_ID = 8, 63, 8
TOY_SPECIAL = {"pad": 0, "cls": 1, "sep": 2, "mask": 3}


def toy_token_split(seed: int, which: int, documents: int, segments_per_doc=(2, 6), tokens_per_segment=(4, 12)):
    """(tokens int64 [T], segments int64 [G + 1], docs int64 [D + 1]) of split number ``which`` for ``seed``; a
    document holds ``segments_per_doc`` = (lo, hi) segments of ``tokens_per_segment`` = (lo, hi) tokens, both ends
    included."""
    seg_lo, seg_hi = int(segments_per_doc[0]), int(segments_per_doc[1])
    tok_lo, tok_hi = int(tokens_per_segment[0]), int(tokens_per_segment[1])
    g = np.random.Generator(np.random.Philox(np.random.SeedSequence([0x70F7, int(seed), int(which)])))
    tokens, segments, docs = [], [0], [0]
    for _ in range(documents):
        base = TOY_FIRST_ID + TOY_SLICE * int(g.integers(0, TOY_TOPICS))
        for _ in range(int(g.integers(seg_lo, seg_hi + 1))):
            n = int(g.integers(tok_lo, tok_hi + 1))
            follow, fresh = g.random(n) < 0.9, g.integers(0, TOY_SLICE, size=n)
            off = int(fresh[0])
            tokens.append(base + off)
            for i in range(1, n):
                off = (5 * off + 1) % TOY_SLICE if follow[i] else int(fresh[i])
                tokens.append(base + off)
            segments.append(len(tokens))
        docs.append(len(segments) - 1)
    return np.asarray(tokens, dtype=np.int64), np.asarray(segments, dtype=np.int64), np.asarray(docs, dtype=np.int64)


def make_toy_tokens(out: str, seed: int = 0, train_docs: int = 512, val_docs: int = 64, vocab: int = 512,
                    segments_per_doc=(2, 6), tokens_per_segment=(4, 12)) -> None:
    if vocab < TOY_FIRST_ID + TOY_TOPICS * TOY_SLICE:
        raise ValueError("--vocab must be at least %d (8 specials and reserved ids, 8 topics of 63 ids)"
                         % (TOY_FIRST_ID + TOY_TOPICS * TOY_SLICE))
    if train_docs < 2 or val_docs < 2:
        raise ValueError("--train-docs and --val-docs must be at least 2 (sentence pairs need another document)")
    if not 1 <= int(segments_per_doc[0]) <= int(segments_per_doc[1]):
        raise ValueError("--segments-per-doc LO HI must satisfy 1 <= LO <= HI")
    if not 1 <= int(tokens_per_segment[0]) <= int(tokens_per_segment[1]):
        raise ValueError("--tokens-per-segment LO HI must satisfy 1 <= LO <= HI")
    split = lambda which, documents: toy_token_split(seed, which, documents, segments_per_doc,  # noqa: E731
                                                     tokens_per_segment)
    write_token_dataset(out, vocab, {"train": split(0, train_docs), "val": split(1, val_docs)}, TOY_SPECIAL)


def read_cifar_batch(path: str):
    with open(path, "rb") as f:
        d = pickle.load(f, encoding="bytes")
    get = lambda k: d[k] if k in d else d[k.encode()]  # noqa: E731 -- the original pickles have bytes keys
    data = np.asarray(get("data"), dtype=np.uint8)
    if data.ndim != 2 or data.shape[1] != 3072:
        raise ValueError("%s: data must be [n, 3072]" % path)
    return data.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1), np.asarray(get("labels"), dtype=np.int64)


def make_cifar10(out: str, src: str) -> None:
    train = [os.path.join(src, "data_batch_%d" % i) for i in range(1, 6)]
    train = [p for p in train if os.path.isfile(p)]
    test = os.path.join(src, "test_batch")
    if not train or not os.path.isfile(test):
        raise FileNotFoundError("%s must hold data_batch_1..5 and test_batch" % src)
    parts = [read_cifar_batch(p) for p in train]
    splits = {"train": (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])),
              "val": read_cifar_batch(test)}
    write_dataset(out, 10, CIFAR10_MEAN, CIFAR10_STD, splits)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m k8s_amd.tools.make_dataset", description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--toy", action="store_true")
    src.add_argument("--cifar10-batches", default=None, metavar="DIR")
    src.add_argument("--toy-tokens", action="store_true", help="a learnable token set for the BERT and Llama models")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--train", type=int, default=2048)
    ap.add_argument("--val", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--size", type=int, default=40)
    ap.add_argument("--train-docs", type=int, default=512)
    ap.add_argument("--val-docs", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=512)
    ap.add_argument("--segments-per-doc", type=int, nargs=2, default=[2, 6], metavar=("LO", "HI"),
                    help="--toy-tokens: segments per document, both ends included (documents of HI * 8 tokens on "
                         "average at LO = HI)")
    ap.add_argument("--tokens-per-segment", type=int, nargs=2, default=[4, 12], metavar=("LO", "HI"),
                    help="--toy-tokens: tokens per segment, both ends included (8 56: BERT pairs that fill about "
                         "half of --seq 128)")
    a = ap.parse_args(argv)
    try:
        if a.toy_tokens:
            make_toy_tokens(a.out, a.seed, a.train_docs, a.val_docs, a.vocab, tuple(a.segments_per_doc),
                            tuple(a.tokens_per_segment))
        elif a.toy:
            make_toy(a.out, a.seed, a.train, a.val, a.classes, a.size)
        else:
            make_cifar10(a.out, a.cifar10_batches)
    except (ValueError, OSError) as e:
        print("error: %s" % e, file=sys.stderr)
        return 1
    print(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
