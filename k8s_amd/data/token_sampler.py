"""Which tokens make batch ``t`` of rank ``r`` of a token dataset: pure functions of their arguments (host, integers
and float64 only). Nothing depends on what was drawn before.

* Epoch and permutation are ``sampler.batch_indices``'s: ``E = items // (batch * world)`` steps per epoch, one
  permutation per ``(seed, epoch)`` shared by all ranks, the last partial batch dropped.
* Every sample carries its ordinal ``ord = (t * world + r) * batch + n``, its position in the global stream. The
  next-sentence draw (here) and the masks (the kernel) are keyed by ``ord``: the same global batch gets the same
  pairs and masks whatever the world size, and a new epoch draws new ones (dynamic masking).

BERT: the items are the ``G`` segments. A sample's A is its anchor segment ``s``; a generator keyed ``(seed, ord)``
(one Philox block per sample, ``pair_draws``, so a batch is drawn in one vectorised pass) draws ``u``: B is segment
``s + 1`` (``nsp = 0``) if ``u < 1/2`` and ``s + 1`` lies in the same document, otherwise a uniformly drawn segment of
a uniformly drawn other document (``nsp = 1``). The pair is truncated to ``la + lb <= S - 3`` by dropping the last
token of the longer segment, A on ties; ``L = la + lb + 3`` and ``n = min(P, max(1, (3 L + 10) // 20), la + lb)`` --
round(0.15 L) half-up, capped as ``max_predictions_per_seq`` caps it. Table row, int64: ``(a0, la, b0, lb, n, ord)``.

Llama: the items are the ``(T - 1) // S`` windows; row ``n`` is ``start = item * S``.

Evaluation: item ``(i * world + r) * batch + n`` of the split, in order; ``ord`` is the item index and the draws
use ``stream = 1``, so a held-out batch is the same every time. Rows past the end reuse item 0 and are marked not
real: the loader gives them label -100.
"""
from __future__ import annotations

import functools

import numpy as np

from k8s_amd.data import sampler
from k8s_amd.data.dataset import DataError

_PAIR = 0x70C5  # generator domain of the next-sentence draws


def truncate_pair(la: int, lb: int, budget: int):
    """(la, lb) after dropping the last token of the longer segment, A on ties, until ``la + lb <= budget``."""
    excess = la + lb - budget
    if excess <= 0:
        return la, lb
    d = abs(la - lb)
    if excess <= d:
        return (la - excess, lb) if la >= lb else (la, lb - excess)
    m, rest = min(la, lb), excess - d  # equal lengths m; then A, B, A, ... drop in turn
    return m - (rest + 1) // 2, m - rest // 2


def n_predictions(L: int, P: int, candidates: int) -> int:
    return min(P, max(1, (3 * L + 10) // 20), candidates)


def check_seq(S: int, P: int) -> None:
    if S < 5:
        raise DataError("--seq must be at least 5 ([CLS] A [SEP] B [SEP] with one token per segment), got %d" % S)
    if not 1 <= P <= S:
        raise DataError("the model's max_predictions = %d must lie in [1, --seq = %d]" % (P, S))


def truncate_pairs(la: np.ndarray, lb: np.ndarray, budget: int):
    """``truncate_pair`` on int64 arrays."""
    excess = np.maximum(la + lb - budget, 0)
    d = np.abs(la - lb)
    first = np.minimum(excess, d)  # taken from the longer segment alone
    rest = excess - first          # then A, B, A, ... in turn
    a_longer = la >= lb
    return (la - np.where(a_longer, first, 0) - (rest + 1) // 2, lb - np.where(a_longer, 0, first) - rest // 2)


def pair_draws(seed: int, stream: int, ords: np.ndarray) -> np.ndarray:
    """The generator keyed ``(seed, ord)``: three 32-bit words per sample (int64 [N, 3]) from one Philox4x32-10 block,
    counter ``(ord lo, ord hi, stream, _PAIR)`` -- a counter no kernel site uses -- and key ``(seed lo, seed hi)``."""
    import torch

    from k8s_amd.ops.reference import philox4x32

    o = torch.from_numpy(np.ascontiguousarray(ords, dtype=np.int64))
    z = torch.zeros_like(o)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32((o & 0xFFFFFFFF, (o >> 32) & 0xFFFFFFFF, z + int(stream), z + _PAIR),
                   (z + (seed & 0xFFFFFFFF), z + (seed >> 32)))
    return torch.stack(w[:3], dim=1).numpy()


def pair_rows(segments: np.ndarray, docs: np.ndarray, anchors, ords, seed: int, S: int, P: int, stream: int = 0):
    """(table int64 [N, 6], nsp int64 [N], kv_lens int64 [N]) of the samples anchored at segments ``anchors`` with
    ordinals ``ords``. With the sample's draws ``w0, w1, w2`` (32-bit): ``u = w0 / 2^32``; the other document is
    number ``(w1 * (D - 1)) >> 32`` of those that are not A's, and B its segment number ``(w2 * count) >> 32``."""
    s = np.asarray(anchors, dtype=np.int64)
    ords = np.asarray(ords, dtype=np.int64)
    D = len(docs) - 1
    w = pair_draws(seed, stream, ords)
    da = np.searchsorted(docs, s, side="right") - 1
    follow = (w[:, 0] < (1 << 31)) & (s + 1 < docs[da + 1])
    d = (w[:, 1] * (D - 1)) >> 32
    d = d + (d >= da)
    count = docs[d + 1] - docs[d]
    b = np.where(follow, s + 1, docs[d] + ((w[:, 2] * count) >> 32))
    a0, b0 = segments[s], segments[b]
    la, lb = truncate_pairs(segments[s + 1] - a0, segments[b + 1] - b0, S - 3)
    L = la + lb + 3
    n = np.minimum(np.minimum(P, np.maximum(1, (3 * L + 10) // 20)), la + lb)
    return np.stack([a0, la, b0, lb, n, ords], axis=1).astype(np.int64), np.where(follow, 0, 1).astype(np.int64), L


@functools.lru_cache(maxsize=2)
def _epoch_permutation(seed: int, epoch: int, items: int) -> np.ndarray:
    """``sampler.batch_indices``'s permutation of the epoch, kept for the epoch's other batches: a corpus has far more
    segments than a batch, and a permutation per batch would cost more than the batch."""
    return sampler._gen(sampler._PERM, seed, epoch).permutation(items)


def train_items(seed: int, t: int, r: int, world: int, batch: int, items: int):
    """(item indices int64 [batch], ordinals int64 [batch]) of training batch ``t`` of rank ``r``: what
    ``sampler.batch_indices`` gives, and each sample's position in the global stream."""
    E = items // (batch * world)
    at = ((t % E) * world + r) * batch
    idx = _epoch_permutation(int(seed), t // E, int(items))[at:at + batch].astype(np.int64)
    return idx, (t * world + r) * batch + np.arange(batch, dtype=np.int64)


def eval_items(i: int, r: int, world: int, batch: int, items: int):
    """(item indices, ordinals, real bool [batch]) of evaluation batch ``i``: the split in order; rows past its end
    are not real and point at item 0."""
    idx = (i * world + r) * batch + np.arange(batch, dtype=np.int64)
    real = idx < items
    idx = np.where(real, idx, 0)
    return idx, idx.copy(), real


def windows(T: int, S: int) -> int:
    """Causal-LM items: the whole windows of ``S`` tokens that have a next token."""
    return max((T - 1) // S, 0)


def steps_per_epoch(items: int, batch: int, world: int, what: str) -> int:
    E = items // (batch * world)
    if E == 0:
        raise DataError("the training split's %d %s do not fill one global batch of %d x %d"
                        % (items, what, batch, world))
    return E
