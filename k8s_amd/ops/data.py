"""Dataset ops: the fused batch-assembly kernels (``csrc/kernels/augment.hip``, ``csrc/kernels/token_batch.hip``).

``augment`` turns N rows of an int32 table into the stem's input in one pass over the output: gather the source image,
crop (zero padded) or resize (bilinear) to S x S, flip, normalise, round to bf16 and lay out as "nhwc8" or as the
space-to-depth image "s2d" that ``stem_conv_s2d`` reads. A uint8 ``src`` on the GPU runs the HIP kernel; one on the
host runs ``ops.reference.augment``, the same definition in torch (float64), which is also the kernel's oracle.

``mlm_batch`` turns N rows of an int64 table into a BERT pretraining batch in one launch: ``[CLS] A [SEP] B [SEP] pad``,
token types, exactly ``n`` masked positions drawn without replacement from a counter generator, the 80 / 10 / 10 rule
and the compacted [N, P] labels and positions. ``causal_batch`` gathers causal-LM windows, and ``causal_doc_batch``
also returns every token's document bounds inside its row, its position inside the document and labels that stop at
document ends. ``mlm_batch_unpadded`` writes the same BERT samples back to back into one token stream, with the span
bounds of ``ops.attention``'s ``span=`` and the stream rows the heads gather. All are integer arithmetic: the GPU
kernels match ``ops.reference.mlm_batch`` / ``mlm_batch_unpadded`` / ``causal_batch`` / ``causal_doc_batch`` (the CPU
path) bit for bit.
"""
from __future__ import annotations

import torch

from k8s_amd.ops import reference as ref
from k8s_amd.ops._ext import load as _load_ext

LAYOUTS = ("nhwc8", "s2d")


def norm_constants(mean, std):
    """(a, b) with a_c = fp32(1 / std_c), b_c = fp32(-mean_c / std_c), as Python floats (0..255 scale)."""
    a = [float(torch.tensor(1.0 / float(s), dtype=torch.float32)) for s in std]
    b = [float(torch.tensor(-float(m) / float(s), dtype=torch.float32)) for m, s in zip(mean, std)]
    return a, b


def launches() -> int:
    """Augmentation kernels this process has launched (a rejected call launches none)."""
    return int(_load_ext().augment_launches())


def augment(src: torch.Tensor, table: torch.Tensor, a, b, S: int, layout: str = "s2d") -> torch.Tensor:
    """``src`` uint8 [M, Hs, Ws, 3]; ``table`` int32 [N, 6] on the host, rows (src index, y0, x0, h, w, flip);
    ``a``, ``b``: ``norm_constants``. Returns bf16 [N, S, S, 8] ("nhwc8") or [N, S/2+3, S/2+3, 16] ("s2d"). The GPU
    binding validates every table row on the host before anything is launched and raises on the first bad one."""
    if src.is_cuda:
        return _load_ext().augment(src, table, [float(v) for v in a], [float(v) for v in b], int(S), layout)
    return ref.augment(src, table, a, b, int(S), layout)


def token_launches() -> int:
    """Token batch kernels (``mlm_batch``, ``causal_batch``) this process has launched (a rejected call launches
    none)."""
    return int(_load_ext().token_launches())


def _seed64(seed: int) -> int:
    """Any 64-bit seed as the int64 with the same bits."""
    v = int(seed) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v


def mlm_batch(src: torch.Tensor, table: torch.Tensor, S: int, P: int, vocab: int, special, seed: int,
              stream: int = 0):
    """``src``: the 1-D token array, int32 or uint16 data as an int16 view (read unsigned); ``table`` int64 [N, 6] on
    the host, rows (a0, la, b0, lb, n, ord); ``special`` = (pad, cls, sep, mask); ``stream``: 0 training, 1
    evaluation (separate generator sites). Returns (ids [N, S], token_types [N, S], labels [N, P], positions [N, P]),
    int64 on ``src``'s device. The GPU binding validates every table row on the host before anything is launched and
    raises on the first bad one."""
    if src.is_cuda:
        return tuple(_load_ext().mlm_batch(src, table, int(S), int(P), int(vocab), [int(v) for v in special],
                                           _seed64(seed), int(stream)))
    return ref.mlm_batch(src, table, int(S), int(P), int(vocab), special, _seed64(seed), int(stream))


def mlm_batch_unpadded(src: torch.Tensor, table: torch.Tensor, cu: torch.Tensor, T: int, S: int, P: int, vocab: int,
                       special, seed: int, stream: int = 0):
    """``mlm_batch`` without padding, in one launch: the N samples back to back in one stream of ``T`` rows. ``cu``
    int64 [N + 1] on the host holds the samples' first rows (cu[0] = 0, cu[n + 1] - cu[n] = la + lb + 3) and ``T`` is
    cu[N] rounded up to a multiple of 128 (``ops.reference.unpad_stream_rows``). Returns ``(ids, token_types, pos)``
    int64 [T], ``(labels, rows)`` int64 [N, P] -- ``mlm_batch``'s labels, and the stream rows of its positions, unused
    slots pointing at the sample's first row --, ``cls_rows`` int64 [N] and the span bounds ``(lo, hi)`` int32 [1, T]
    that ``ops.attention``'s ``span=`` takes. The tail [cu[N], T) is one pad span. Sample n gets the masks
    ``mlm_batch`` gives it. The GPU binding validates the table, ``cu`` and ``T`` on the host before anything is
    launched and raises on the first failed check."""
    if src.is_cuda:
        return tuple(_load_ext().mlm_batch_unpadded(src, table, cu, int(T), int(S), int(P), int(vocab),
                                                    [int(v) for v in special], _seed64(seed), int(stream)))
    return ref.mlm_batch_unpadded(src, table, cu, int(T), int(S), int(P), int(vocab), special, _seed64(seed),
                                  int(stream))


def causal_batch(src: torch.Tensor, starts: torch.Tensor, S: int):
    """``starts`` int64 [N] on the host: (ids, labels) int64 [N, S] with ids = src[start : start + S] and labels the
    same window one token later; ``0 <= start`` and ``start + S + 1 <= len(src)`` are checked before the launch."""
    if src.is_cuda:
        return tuple(_load_ext().causal_batch(src, starts, int(S)))
    return ref.causal_batch(src, starts, int(S))


def doc_offsets(doc_tok, device) -> torch.Tensor:
    """The documents' token offsets (int64 [D + 1], e.g. ``segments[docs]`` of a token split) checked once on the host
    -- strictly ascending from 0, else ``ValueError`` -- and uploaded to ``device`` for ``causal_doc_batch``."""
    t = torch.as_tensor(doc_tok).contiguous()
    ref.check_doc_tok(t)
    return t.to(device)


def causal_doc_batch(src: torch.Tensor, starts: torch.Tensor, abs_starts: torch.Tensor, doc_tok: torch.Tensor, S: int,
                     split_tokens: int = None):
    """``causal_batch`` for rows that hold several documents, in one launch: ``(ids, labels, lo, hi, pos)``, ids and
    labels int64 [N, S], the rest int32 [N, S]. ``starts`` (int64 [N], host) index ``src``; ``abs_starts`` are the same
    windows' positions in the split (equal to ``starts`` when ``src`` is the whole split); ``doc_tok`` is
    ``doc_offsets``' tensor on ``src``'s device. ``lo`` / ``hi`` bound each token's document inside its row
    (``ops.attention``'s ``doc=``), ``pos`` restarts at every document (what ``rope_`` / ``linear_rope`` take), and the
    last token of a document carries the label -100. ``split_tokens``: ``doc_tok[-1]``, known to the caller from the
    host copy (read back from the device when not given). Windows that leave ``src`` or the split are rejected before
    the launch."""
    if src.is_cuda:
        total = int(doc_tok[-1]) if split_tokens is None else int(split_tokens)
        return tuple(_load_ext().causal_doc_batch(src, starts, abs_starts, doc_tok, int(S), total))
    return ref.causal_doc_batch(src, starts, abs_starts, doc_tok, int(S))
