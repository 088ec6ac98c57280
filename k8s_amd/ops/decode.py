"""Generation ops (K16): what one decode step needs beyond the training kernels.

``linear(x, pw)``: y = x W^T for the 1 to 16 rows of a decode step -- ``csrc/kernels/decode.hip``'s weight-streaming
skinny-M GEMM on the shapes it takes (GPU bf16, K % 64 == 0, N % 16 == 0), otherwise ``ops.nn.linear``; GPU calls that
leave the skinny kernel are counted in ``LINEAR_OTHER``.
``kv_append`` copies the k / v columns of a packed, rotated QKV projection output into a layer's caches;
``decode_attention`` is one query token per row against the first ``lens[b]`` cache positions, split over key chunks.
Both take a device table (``start`` / ``lens``, int32 [B]) with the host mirror the caller keeps: the mirror is checked
before anything is launched, the kernels clamp the device copy once more.
CPU tensors use the plain-torch definitions in ``ops/reference.py``, which the GPU tests compare against.
"""
from __future__ import annotations

import torch

from k8s_amd.ops import nn as K
from k8s_amd.ops import reference as ref
from k8s_amd.ops._ext import load as _load

# ops.decode.linear calls on the GPU: on the skinny kernel / through ops.nn.linear
LINEAR_SKINNY = 0
LINEAR_OTHER = 0


def reset_counters() -> None:
    global LINEAR_SKINNY, LINEAR_OTHER
    LINEAR_SKINNY = LINEAR_OTHER = 0


def skinny_ok(x, w) -> bool:
    """Whether ``linear_skinny`` takes the product: GPU bf16, dense, 16-byte aligned, and the shape contract."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.dim() == 2 and w.dim() == 2
            and x.is_contiguous() and w.is_contiguous() and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
            and bool(_load().linear_skinny_ok(x.shape[0], w.shape[0], x.shape[1])))


def linear_skinny(x, w):
    """The kernel itself (GPU; raises outside its contract), or its definition on CPU tensors."""
    if x.is_cuda:
        return _load().linear_skinny(x, w)
    return ref.linear_skinny(x, w)


def linear(x, pw):
    """y = x W^T, x [M, in], ``pw`` a flat-store parameter [out, in] (its bf16 working copy is what is streamed)."""
    global LINEAR_SKINNY, LINEAR_OTHER
    w = pw.weight
    if x.is_cuda and x.dtype == w.dtype and skinny_ok(x, w):
        LINEAR_SKINNY += 1
        return _load().linear_skinny(x, w)
    if x.is_cuda:
        LINEAR_OTHER += 1
    return K.linear(x, pw)


def rope_(qkv, rot_cols: int, pos, table):
    """Rotate the first ``rot_cols`` columns (the q and k heads) of a packed projection output in place; returns it."""
    if qkv.is_cuda and qkv.dtype == torch.bfloat16:
        _load().rope_(qkv[:, :rot_cols], pos, table, False)
    else:
        qkv[:, :rot_cols] = K._rope_ref(qkv[:, :rot_cols], pos, table)
    return qkv


def kv_append(qkv, cache_k, cache_v, start, start_host, S: int, Hq: int) -> None:
    """Token s of row b of ``qkv`` [B * S, (Hq + 2 Hkv) * D] goes to position ``start[b] + s`` of the caches
    [B, Hkv, Smax, D]. ``start``: int32 [B] on the caches' device; ``start_host``: its mirror, checked here
    (``0 <= start`` and ``start + S <= Smax``, a ``RuntimeError`` before anything is written)."""
    if cache_k.is_cuda:
        _load().kv_append(qkv, cache_k, cache_v, start, start_host, S, Hq)
        return
    ref.check_cache_table(start_host, cache_k.shape[0], 0, cache_k.shape[2] - S, "start")
    ref.kv_append(qkv, cache_k, cache_v, start_host, S, Hq)


def decode_attention(q, cache_k, cache_v, lens, lens_host, scale: float):
    """q [B, Hq, D] (bf16 on the GPU, D 64 or 128, Hq / Hkv <= 16) against keys 0 .. lens[b] - 1 of the caches; returns
    [B, Hq * D]. ``lens``: int32 [B] on the device; ``lens_host``: its mirror (``lens < 1`` is a ``RuntimeError``)."""
    if q.is_cuda:
        return _load().decode_attention(q, cache_k, cache_v, lens, lens_host, float(scale))
    ref.check_cache_table(lens_host, cache_k.shape[0], 1, cache_k.shape[2], "lens")
    return ref.decode_attention(q, cache_k, cache_v, lens_host, scale)
