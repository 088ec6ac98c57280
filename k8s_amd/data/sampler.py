"""Which samples make batch ``t`` of rank ``r``, and how each is augmented: pure functions of their arguments.

Nothing here depends on what was drawn before: batch ``t`` is the same asked first, after others, or after a resume.

* ``E = M // (batch * world)`` steps per epoch; the last partial batch is dropped; ``E == 0`` is an error.
* Epoch ``t // E`` uses one permutation of ``M`` from a generator keyed by ``(seed, epoch)``, shared by all ranks;
  rank ``r`` takes its ``batch``-long block of the global batch at position ``t % E``.
* Each sample gets one row ``(src index, y0, x0, h, w, flip)`` of an int32 table [N, 6], drawn from a generator keyed
  by ``(seed, t, r)``. All arithmetic is float64 on the host: no device arithmetic ever decides an integer.
"""
from __future__ import annotations

import math

import numpy as np

from k8s_amd.data.dataset import DataError

AUGMENTS = ("crop", "rrc", "none")
_PERM, _ROWS = 0x70E2, 0x7AB1  # generator domains: the epoch permutation, the table rows


def _gen(*key) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(np.random.SeedSequence([int(k) & 0xFFFFFFFFFFFFFFFF for k in key])))


def steps_per_epoch(M: int, batch: int, world: int) -> int:
    E = M // (batch * world)
    if E == 0:
        raise DataError("the training split's %d images do not fill one global batch of %d x %d" % (M, batch, world))
    return E


def batch_indices(seed: int, t: int, r: int, world: int, batch: int, M: int) -> np.ndarray:
    """Source indices (int64 [batch]) of batch ``t`` of rank ``r``."""
    E = steps_per_epoch(M, batch, world)
    perm = _gen(_PERM, seed, t // E).permutation(M)
    at = ((t % E) * world + r) * batch
    return perm[at:at + batch].astype(np.int64)


def centre_box(Hs: int, Ws: int, h: int, w: int):
    return (Hs - h) // 2, (Ws - w) // 2, h, w


def rrc_boxes(g: np.random.Generator, n: int, Hs: int, Ws: int, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3),
              attempts: int = 10) -> np.ndarray:
    """torchvision's RandomResizedCrop rule for ``n`` samples, int64 [n, 4] rows (y0, x0, h, w), always inside the
    source: area scale uniform in ``scale``, log-uniform aspect in ``ratio``, ``attempts`` tries, then the centred
    fallback (the whole source, trimmed to the nearest allowed aspect)."""
    area = float(Hs * Ws)
    target = area * g.uniform(scale[0], scale[1], size=(n, attempts))
    aspect = np.exp(g.uniform(math.log(ratio[0]), math.log(ratio[1]), size=(n, attempts)))
    w = np.rint(np.sqrt(target * aspect)).astype(np.int64)
    h = np.rint(np.sqrt(target / aspect)).astype(np.int64)
    ok = (w > 0) & (w <= Ws) & (h > 0) & (h <= Hs)
    first = ok.argmax(axis=1)
    rows = np.arange(n)
    h, w, found = h[rows, first], w[rows, first], ok.any(axis=1)
    u = g.uniform(size=(n, 2))
    y0 = np.floor(u[:, 0] * (Hs - h + 1)).astype(np.int64)
    x0 = np.floor(u[:, 1] * (Ws - w + 1)).astype(np.int64)
    in_ratio = Ws / Hs
    if in_ratio < ratio[0]:
        fw, fh = Ws, int(round(Ws / ratio[0]))
    elif in_ratio > ratio[1]:
        fh, fw = Hs, int(round(Hs * ratio[1]))
    else:
        fh, fw = Hs, Ws
    fh, fw = min(fh, Hs), min(fw, Ws)
    fy, fx, _, _ = centre_box(Hs, Ws, fh, fw)
    out = np.stack([np.where(found, np.minimum(y0, Hs - h), fy), np.where(found, np.minimum(x0, Ws - w), fx),
                    np.where(found, h, fh), np.where(found, w, fw)], axis=1)
    return out


def check_geometry(augment: str, Hs: int, Ws: int, S: int, pad: int) -> None:
    if augment not in AUGMENTS:
        raise DataError("--augment must be one of %s, not %r" % (", ".join(AUGMENTS), augment))
    if S < 2 or S % 2:
        raise DataError("--image must be even (the stem reads a 2x2 space-to-depth image), got %d" % S)
    if pad < 0 or (augment == "crop" and (Hs - S + 2 * pad < 0 or Ws - S + 2 * pad < 0)):
        raise DataError("--image %d does not fit the %d x %d source padded by --crop-pad %d" % (S, Hs, Ws, pad))


def train_table(indices, seed: int, t: int, r: int, Hs: int, Ws: int, S: int, augment: str = "crop",
                pad: int = 4) -> np.ndarray:
    """int32 [N, 6] rows (src index, y0, x0, h, w, flip) of training batch ``t`` of rank ``r``."""
    n = len(indices)
    g = _gen(_ROWS, seed, t, r)
    tab = np.empty((n, 6), dtype=np.int32)
    tab[:, 0] = indices
    if augment == "crop":  # every position of the source zero-padded by `pad`
        tab[:, 1] = g.integers(-pad, Hs - S + pad + 1, size=n)
        tab[:, 2] = g.integers(-pad, Ws - S + pad + 1, size=n)
        tab[:, 3] = tab[:, 4] = S
        tab[:, 5] = g.integers(0, 2, size=n)
    elif augment == "rrc":
        tab[:, 1:5] = rrc_boxes(g, n, Hs, Ws)
        tab[:, 5] = g.integers(0, 2, size=n)
    else:
        tab[:, 1:5] = centre_box(Hs, Ws, S, S)
        tab[:, 5] = 0
    return tab


def eval_table(indices, Hs: int, Ws: int, S: int, augment: str = "crop") -> np.ndarray:
    """Evaluation rows: centred, no flip -- ``S x S`` for crop / none, the square of side round(0.875 min(Hs, Ws))
    resized to ``S`` for rrc."""
    tab = np.zeros((len(indices), 6), dtype=np.int32)
    tab[:, 0] = indices
    side = int(round(0.875 * min(Hs, Ws))) if augment == "rrc" else S
    tab[:, 1:5] = centre_box(Hs, Ws, side, side)
    return tab
