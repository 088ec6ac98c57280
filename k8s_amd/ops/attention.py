"""Attention (K5) entry point.

``attention(q, k, v, causal, kv_lens)`` with token-major layouts:
q [B, S, Hq, D], k/v [B, S, Hkv, D] (GQA: Hq % Hkv == 0), bf16.

GPU: the gfx950 flash-attention kernels (``csrc/kernels/attention.hip``:
online-softmax forward writing the log-sum-exp, recompute backward with
dK/dV in registers and atomically accumulated dQ). q/k/v may be strided
views (e.g. column slices of the fused QKV projection) -- no copies. Head
dims other than 64/128 and CPU tensors use an explicit matmul/softmax
reference (no SDPA dispatch, so no Triton-built kernels run).

A call masks at most one thing beyond ``causal`` / ``kv_lens``: ``dropout``, ``doc`` or ``span``. ``_mask_spec`` checks
the combination once and returns one record (``_Mask``) that the autograd functions carry; whether the flash kernels
take the call, and which of them run, is one question to the extension (``flash_plan``), and a call they do not take
runs the reference with the same mask.

``dropout=(p, DropoutState, site)`` drops attention probabilities with the counter generator of
``csrc/kernels/rng.h`` (row = (b * Hq + h) * Sq + q, col = key): fused into the forward and the backward for the
shapes ``flash_plan`` takes with ``mask="drop"`` -- head_dim 64 and either the one-block backward's shapes (Sq, Sk <=
128, Hq == Hkv) or Sq and Sk multiples of 64 (the multi-tile forward and the three-kernel backward); any other GPU
shape runs the reference composition with the same mask, counted in ``DROPOUT_FALLBACKS`` and warned about once.

``doc=(lo, hi)``: a document-boundary mask inside the causal triangle, for rows that pack several documents. ``lo`` and
``hi`` are int32 [B, S]: ``lo[b, i]`` is the row index of the first token of token ``i``'s document and ``hi[b, i]`` one
past its last (``doc_bounds`` derives both from ``lo``). Query ``i`` sees key ``j`` iff ``lo[i] <= j <= i``. The DOC
forms of the multi-tile forward, the dK/dV and the dQ kernels skip the key (query) tiles no query (key) of a block can
see. Causal self-attention only: with ``kv_lens``, ``dropout`` or ``causal=False`` it is a ``ValueError``. GPU operands
outside the flash contract run the reference with the same mask.

``span=(lo, hi)``: a bidirectional span mask for rows that hold several sequences back to back (unpadded BERT). ``lo``
and ``hi`` are int32 [B, S] (``span_bounds`` derives both from the span starts): query ``i`` sees key ``j`` iff
``lo[i] <= j < hi[i]``; with consistent tables (constant inside a span, spans tiling the row) that equals
``lo[j] <= i < hi[j]``, and every query sees itself. The SPAN forms of the multi-tile forward, the dK/dV and the dQ
kernels (head_dim 64) visit only the tiles a block's spans reach. Non-causal self-attention only: with ``causal=True``,
``kv_lens``, ``dropout`` or ``doc=`` it is a ``ValueError``. head_dim 128 and GPU operands outside the flash contract
run the reference with the same mask.
"""
from __future__ import annotations

import math
import warnings
from typing import NamedTuple, Optional

import torch

from k8s_amd.ops import reference as ref
from k8s_amd.ops._ext import load as _load

# GPU attention calls with dropout that ran the reference composition instead of the fused kernels
DROPOUT_FALLBACKS = 0


def _dropout_fallback(q, k):
    global DROPOUT_FALLBACKS
    if DROPOUT_FALLBACKS == 0:
        warnings.warn("k8s_amd attention: dropout on q %s / k %s is outside the fused kernels' shape contract "
                      "(head_dim 64; Sq, Sk <= 128 with Hq == Hkv, or Sq and Sk multiples of 64); using the reference "
                      "composition"
                      % (tuple(q.shape), tuple(k.shape)))
    DROPOUT_FALLBACKS += 1


def _drop_spec(dropout):
    from k8s_amd.ops import nn as _nn

    return _nn._drop_spec(dropout, "attention")


def _flash_ok(q, k, v) -> bool:
    if not (q.is_cuda and q.dtype == torch.bfloat16 and q.shape[-1] in (64, 128)):
        return False
    ok = all(t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0
             for t in (q, k, v))
    return ok and hasattr(_load(), "flash_fwd")  # _load() raises if the extension is missing on a GPU box


def doc_mask_reference(doc_lo: torch.Tensor) -> torch.Tensor:
    """bool [B, S, S], True where query i may NOT see key j: the complement of ``lo[i] <= j <= i``."""
    S = doc_lo.shape[1]
    i = torch.arange(S, device=doc_lo.device)
    return (i[None, None, :] < doc_lo.long()[:, :, None]) | (i[None, None, :] > i[None, :, None])


def doc_bounds(doc_starts: torch.Tensor):
    """``doc_starts`` integer [B, S]: for every token the row index of the first token of its document. Returns the
    ``(lo, hi)`` int32 pair ``attention(..., doc=)`` takes, on the same device: ``lo`` is ``doc_starts`` and ``hi[i]``
    the next document's start after ``i`` (``S`` in the last document). A CPU tensor is checked first (``lo`` ascending,
    ``0 <= lo[i] <= i`` and ``lo[lo[i]] == lo[i]``) and a bad one raises ``ValueError``; device tensors are not read by
    the host, and the kernels clamp whatever they hold."""
    if doc_starts.dim() != 2 or doc_starts.dtype not in (torch.int32, torch.int64) or doc_starts.shape[1] < 1:
        raise ValueError("doc_starts must be an int32 or int64 [B, S] tensor")
    B, S = doc_starts.shape
    lo = doc_starts.long()
    idx = torch.arange(S, device=lo.device).expand(B, S)
    if not doc_starts.is_cuda:
        ok = bool((lo >= 0).all()) and bool((lo <= idx).all()) and bool((lo[:, 1:] >= lo[:, :-1]).all())
        if not (ok and bool((torch.gather(lo, 1, lo) == lo).all())):
            raise ValueError("doc_starts must ascend along each row with 0 <= start[i] <= i and start[start[i]] == "
                             "start[i]")
    # hi[i] = the smallest document start above i: a reversed running minimum over (j if a document starts at j else S)
    nxt = torch.where(lo == idx, idx, torch.full_like(idx, S))
    nxt = torch.cat([nxt[:, 1:], torch.full((B, 1), S, dtype=nxt.dtype, device=nxt.device)], 1)
    hi = torch.cummin(nxt.flip(1), 1).values.flip(1)
    return lo.to(torch.int32).contiguous(), hi.to(torch.int32).contiguous()


def span_mask_reference(span_lo: torch.Tensor, span_hi: torch.Tensor) -> torch.Tensor:
    """bool [B, S, S], True where query i may NOT see key j: the complement of ``lo[i] <= j < hi[i]``."""
    S = span_lo.shape[1]
    j = torch.arange(S, device=span_lo.device)[None, None, :]
    return (j < span_lo.long()[:, :, None]) | (j >= span_hi.long()[:, :, None])


def span_bounds(starts: torch.Tensor):
    """``starts`` integer [B, S]: for every token the row index of the first token of its span. Returns the ``(lo, hi)``
    int32 pair ``attention(..., span=)`` takes, on the same device: ``lo`` is ``starts`` and ``hi[i]`` the next span's
    start after ``i`` (``S`` in the last span). The tables ``doc_bounds`` builds, read without the causal triangle; a
    CPU tensor is checked the same way and a bad one raises ``ValueError``."""
    try:
        return doc_bounds(starts)
    except ValueError as e:
        raise ValueError(str(e).replace("doc_starts", "starts")) from None


class _Mask(NamedTuple):
    """What a call masks beyond ``causal`` / ``kv_lens``: at most one kind (the extension's names), its ``(lo, hi)``
    tables (doc, span) or its dropout spec ``(p, thr, scale, state, site)`` (drop)."""
    kind: str = "plain"
    lo: Optional[torch.Tensor] = None
    hi: Optional[torch.Tensor] = None
    drop: Optional[tuple] = None


def _mask_spec(causal, kv_lens, dropout, doc, span, B, Sq, Sk, who="attention") -> _Mask:
    """The checked mask of an ``attention`` / ``attention_qkv`` call. Every combination the masks do not have is a
    ``ValueError`` here: a span mask is non-causal self-attention with nothing else masked, a document mask causal
    self-attention without ``kv_lens`` or dropout."""
    qkv = who == "attention_qkv"

    def bad(msg):
        raise ValueError("%s: %s" % (who, msg))

    def check_span():
        if span is None:
            return
        if causal:
            bad("a span mask is bidirectional and cannot be combined with causal=True")
        if Sq != Sk:
            bad("a span mask is defined for self-attention (Sq == Sk) only")
        if kv_lens is not None:
            bad("a span mask cannot be combined with kv_lens")
        if dropout is not None:
            bad("a span mask cannot be combined with dropout")
        if doc is not None:
            bad("a span mask cannot be combined with a document mask")
        if not isinstance(span, (tuple, list)) or len(span) != 2 or span[0] is None or span[1] is None:
            bad("span = (lo, hi) needs both tables")
        if span[0].dtype != torch.int32 or span[1].dtype != torch.int32:
            bad("span = (lo, hi) must be int32 tensors (ops.attention.span_bounds)")
        if tuple(span[0].shape) != (B, Sq) or tuple(span[1].shape) != (B, Sq):
            bad("span = (lo, hi) must have the shape [B, S] of the queries")

    def check_doc():
        if doc is None:
            return
        if qkv and (not causal or kv_lens is not None or dropout is not None):
            bad("a document mask needs causal=True and takes neither kv_lens nor dropout")
        if not causal or Sq != Sk:
            bad("a document mask is defined for causal self-attention (Sq == Sk) only")
        if kv_lens is not None or dropout is not None:
            bad("a document mask cannot be combined with kv_lens or dropout")
        if any(tuple(t.shape) != (B, Sq) or t.dtype != torch.int32 for t in doc):
            bad("doc = (lo, hi) must be two int32 [B, S] tensors (ops.attention.doc_bounds)")

    # (the order conflicts are reported in: attention_qkv reads the dropout tuple first and the document mask second)
    drop = _drop_spec(dropout) if qkv else None
    for check in (check_doc, check_span) if qkv else (check_span, check_doc):
        check()
    if span is not None:
        return _Mask("span", span[0], span[1])
    if doc is not None:
        return _Mask("doc", doc[0], doc[1])
    drop = drop if qkv else _drop_spec(dropout)
    return _Mask("drop", drop=drop) if drop is not None else _Mask()


# keys per tile of the SPAN kernels: None takes the plan's default, 64 / 128 select a form
SPAN_TILE = None


def _mask_kw(mask: _Mask, device) -> dict:
    """flash_fwd / flash_bwd keyword arguments of a mask; none for a plain call."""
    if mask.kind == "drop":
        _, thr, scale, state, site = mask.drop
        return {"drop_state": state.tensor, "drop_thr": thr, "drop_scale": scale, "drop_site": site}
    if mask.kind == "plain":
        return {}
    kw = {mask.kind + "_lo": mask.lo.to(device).contiguous(), mask.kind + "_hi": mask.hi.to(device).contiguous()}
    if mask.kind == "span" and SPAN_TILE is not None:
        kw["span_tile"] = int(SPAN_TILE)
    return kw


def _plan(kind, D, B, Sq, Sk, Hq, Hkv, causal, has_lens, max_token_stride) -> dict:
    """The extension's plan for a shape (``flash_plan``): whether the flash kernels take the call, and which run."""
    return _load().flash_plan(D, B, Sq, Sk, Hq, Hkv, bool(causal), has_lens, kind, 0, max_token_stride)


def attention_reference(q, k, v, causal: bool, kv_lens: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                        keep: Optional[torch.Tensor] = None, keep_scale: float = 1.0,
                        doc_lo: Optional[torch.Tensor] = None, span_lo: Optional[torch.Tensor] = None,
                        span_hi: Optional[torch.Tensor] = None):
    """``span_lo`` / ``span_hi`` (int [B, S], non-causal, Sq == Sk): the span mask, query i sees the keys
    lo[i] <= j < hi[i].
    ``keep`` (bool [B, Hq, Sq, Sk], ``ref.attention_keep``) with ``keep_scale``: dropout on the probabilities.
    ``doc_lo`` (int [B, S], with ``causal`` and Sq == Sk): the document mask, query i sees the keys lo[i] <= j <= i."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    scale = scale or 1.0 / math.sqrt(D)
    qh = q.permute(0, 2, 1, 3).float()
    kh = k.permute(0, 2, 1, 3).float().repeat_interleave(rep, dim=1)
    vh = v.permute(0, 2, 1, 3).float().repeat_interleave(rep, dim=1)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    Sk = k.shape[1]
    if causal:
        mask = torch.ones(S, Sk, dtype=torch.bool, device=q.device).triu(1 + Sk - S)  # bottom-right aligned
        s = s.masked_fill(mask, float("-inf"))
    if kv_lens is not None:
        keymask = torch.arange(Sk, device=q.device)[None, :] >= kv_lens[:, None].to(q.device)
        s = s.masked_fill(keymask[:, None, None, :], float("-inf"))
    if doc_lo is not None:
        s = s.masked_fill(doc_mask_reference(doc_lo.to(q.device))[:, None], float("-inf"))
    if (span_lo is None) != (span_hi is None):
        raise ValueError("attention_reference: span_lo and span_hi must be given together")
    if span_lo is not None:
        if causal or kv_lens is not None or doc_lo is not None or S != Sk:
            raise ValueError("attention_reference: a span mask is defined for non-causal self-attention alone")
        s = s.masked_fill(span_mask_reference(span_lo.to(q.device), span_hi.to(q.device))[:, None], float("-inf"))
    p = torch.softmax(s, -1)
    if keep is not None:
        p = torch.where(keep, p * keep_scale, torch.zeros((), device=p.device))
    o = torch.matmul(p, vh)
    return o.permute(0, 2, 1, 3).to(q.dtype)


def _ref_args(mask: _Mask, q, k) -> tuple:
    """attention_reference's (keep, keep_scale, doc_lo, span_lo, span_hi) of a mask."""
    if mask.kind == "drop":
        p, _, scale, state, site = mask.drop
        B, Sq, Hq, _ = q.shape
        return ref.attention_keep(state.tensor.to(q.device), site, B, Hq, Sq, k.shape[1], p), scale, None, None, None
    span = (mask.lo, mask.hi) if mask.kind == "span" else (None, None)
    return (None, 1.0, mask.lo if mask.kind == "doc" else None) + span


class _Flash(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, kv_lens, scale, mask=_Mask()):
        C = _load()
        if kv_lens is not None:
            kv_lens = kv_lens.to(device=q.device, dtype=torch.int32).contiguous()
        ctx.mask_kw = _mask_kw(mask, q.device)
        o, lse = C.flash_fwd(q, k, v, causal, kv_lens, scale, **ctx.mask_kw)
        ctx.save_for_backward(q, k, v, o, lse, kv_lens if kv_lens is not None else torch.empty(0))
        ctx.causal, ctx.scale, ctx.has_lens = causal, scale, kv_lens is not None
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, lens = ctx.saved_tensors
        C = _load()
        dq, dk, dv = C.flash_bwd(do.contiguous(), q, k, v, o, lse, ctx.causal, lens if ctx.has_lens else None,
                                 ctx.scale, **ctx.mask_kw)
        return dq, dk, dv, None, None, None, None


class _Reference(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, kv_lens, scale, mask=_Mask()):
        ctx.save_for_backward(q, k, v)
        ctx.causal, ctx.kv_lens, ctx.scale, ctx.mask = causal, kv_lens, scale, mask
        with torch.no_grad():
            return attention_reference(q, k, v, causal, kv_lens, scale, *_ref_args(mask, q, k))

    @staticmethod
    def backward(ctx, do):
        q, k, v = ctx.saved_tensors
        with torch.enable_grad():
            qq, kk, vv = (t.detach().float().requires_grad_(True) for t in (q, k, v))
            # (dropout: the forward's mask again -- same seed, step and site)
            o = attention_reference(qq, kk, vv, ctx.causal, ctx.kv_lens, ctx.scale, *_ref_args(ctx.mask, q, k))
            dq, dk, dv = torch.autograd.grad(o, (qq, kk, vv), do.float())
        return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype), None, None, None, None


def attention(q, k, v, causal: bool = False, kv_lens: Optional[torch.Tensor] = None, scale: Optional[float] = None,
              dropout: Optional[tuple] = None, doc: Optional[tuple] = None, span: Optional[tuple] = None):
    scale = scale or 1.0 / math.sqrt(q.shape[-1])
    B, Sq, Hq, D = q.shape
    mask = _mask_spec(causal, kv_lens, dropout, doc, span, B, Sq, k.shape[1])
    # the flash kernels, or the reference with the same mask: never a call that drops it
    if _flash_ok(q, k, v) and _plan(mask.kind, D, B, Sq, k.shape[1], Hq, k.shape[2], causal, kv_lens is not None,
                                    max(t.stride(1) for t in (q, k, v)))["ok"]:
        return _Flash.apply(q, k, v, causal, kv_lens, scale, mask)
    if mask.kind == "drop" and q.is_cuda:
        _dropout_fallback(q, k)
    return _Reference.apply(q, k, v, causal, kv_lens, scale, mask)


class _FlashQKV(torch.autograd.Function):
    """Self-attention straight off a fused QKV projection [T = B*S, (H + 2*Hkv)*D]: q / k / v are strided views,
    the optional rotary embedding rotates the q and k columns of one copy in place, and the backward writes the
    packed gradient in place (flash_bwd ``dqkv``) and un-rotates it in place -- no split / concatenation / rope
    copies on either pass."""

    @staticmethod
    def forward(ctx, qkv, B, S, H, Hkv, D, causal, kv_lens, scale, pos, table, bias_link=None, rope_in_place=False,
                rope_applied=False, mask=_Mask()):
        C = _load()
        if kv_lens is not None:
            kv_lens = kv_lens.to(device=qkv.device, dtype=torch.int32).contiguous()
        x = qkv.contiguous()
        if pos is not None and not rope_applied:  # (applied: the projection's epilogue rotated q / k, ops.nn.linear_rope)
            if not rope_in_place:  # (in place: the caller's qkv is a temporary nothing else reads)
                x = x.clone() if x.data_ptr() == qkv.data_ptr() else x
            # (in place, the raw-pointer rotation does not bump autograd's version counter -- and cannot: qkv is
            # the view output of the projection's custom Function, where autograd forbids in-place modification
            # outright. Contract, see ``attention_qkv``: nothing else may hold the projection output.)
            C.rope_(x[:, : (H + Hkv) * D], pos, table, False)
        g = x.view(B, S, H + 2 * Hkv, D)
        q, k, v = g.narrow(2, 0, H), g.narrow(2, H, Hkv), g.narrow(2, H + Hkv, Hkv)
        ctx.mask_kw = _mask_kw(mask, qkv.device)
        o, lse = C.flash_fwd(q, k, v, causal, kv_lens, scale, **ctx.mask_kw)
        ctx.save_for_backward(x, o, lse, kv_lens if kv_lens is not None else torch.empty(0),
                              pos if pos is not None else torch.empty(0), table if table is not None else torch.empty(0))
        ctx.meta = (B, S, H, Hkv, D, causal, scale, kv_lens is not None, pos is not None, mask.kind)
        ctx.bias_link = bias_link
        return o

    @staticmethod
    def backward(ctx, do):
        x, o, lse, lens, pos, table = ctx.saved_tensors
        B, S, H, Hkv, D, causal, scale, has_lens, has_rope, kind = ctx.meta
        C = _load()
        g = x.view(B, S, H + 2 * Hkv, D)
        q, k, v = g.narrow(2, 0, H), g.narrow(2, H, Hkv), g.narrow(2, H + Hkv, Hkv)
        dqkv = torch.empty_like(x)
        # the projection's bias gradient (column sums of dqkv) from the one-block kernel (BiasLink); not with rope,
        # which rotates dqkv after the kernel
        bl, dsum, ss, lpb = ctx.bias_link, None, None, None
        if bl is not None and bl.pb is not None and not has_rope and \
                _plan(kind, D, B, S, S, H, Hkv, causal, has_lens, x.shape[1])["bwd"]["one_block"]:
            lpb = bl.pb
            ss = lpb.store.slot_for_write(lpb)
            dsum = ss.view(lpb.shape) if ss is not None else torch.empty(lpb.shape, device=x.device,
                                                                         dtype=torch.float32)
        C.flash_bwd(do.contiguous(), q, k, v, o, lse, causal, lens if has_lens else None, scale, dqkv, dsum,
                    **ctx.mask_kw)
        if dsum is not None:
            lpb.store.mark_written(lpb) if ss is not None else lpb.store.deposit(lpb, dsum)
            bl.done = True
        if has_rope:
            C.rope_(dqkv[:, : (H + Hkv) * D], pos, table, True)
        return (dqkv,) + (None,) * 14


def attention_qkv(qkv, B: int, S: int, heads: int, kv_heads: int, head_dim: int, causal: bool = False,
                  kv_lens: Optional[torch.Tensor] = None, rope: Optional[tuple] = None,
                  scale: Optional[float] = None, bias_link=None, rope_in_place: bool = False,
                  rope_applied: bool = False, dropout: Optional[tuple] = None, doc: Optional[tuple] = None,
                  span: Optional[tuple] = None):
    """Self-attention of a packed QKV projection ``qkv`` [B*S, (heads + 2*kv_heads) * head_dim] (q heads, then k,
    then v); ``rope`` = (pos [B*S] int32, table) applies rotary embeddings to q and k. Returns o [B, S, heads, D].
    GPU bf16: one fused path (``_FlashQKV``); otherwise the split + ``attention`` reference composition.
    ``bias_link`` (``nn.BiasLink``, also given to the projection ``linear``): short sequences emit the projection's
    bias gradient from the attention backward, and the linear skips its column-sum pass. ``rope_in_place``: rotate
    q / k inside ``qkv`` itself instead of a copy (the caller's projection output is a temporary: Llama's 201 MB
    per-layer clone at s4096 b4). Contract of ``rope_in_place``: the projection output has no other reader --
    no hook, no saved-for-backward reference (``_Linear`` saves its input, not its output), no ``grad_link`` --
    since those would see the rotated values; ``tests/test_attention_gpu.py`` pins in place == copy bitwise.
    ``rope_applied``: q / k already rotated by the projection's epilogue (``ops.nn.linear_rope``); the backward still
    returns the gradient of the UN-rotated projection output (dqkv rotated back), which is what that linear's backward
    takes. ``dropout`` = (p, DropoutState, site): dropout on the probabilities, fused on the shapes ``flash_plan``
    takes (see the module docstring; the bias gradient stays a one-block feature); other shapes take the split +
    ``attention`` composition, which counts the fallback. ``doc`` = (lo, hi): the document mask of ``attention``
    (causal, no ``kv_lens``, no dropout); with ``rope`` the caller passes positions that restart at every document.
    ``span`` = (lo, hi): the span mask of ``attention`` (non-causal, no ``kv_lens``, no dropout, no ``doc``); the SPAN
    kernels at head_dim 64, otherwise the split + ``attention`` composition, which keeps the mask."""
    D = head_dim
    scale = scale or 1.0 / math.sqrt(D)
    W = (heads + 2 * kv_heads) * D
    mask = _mask_spec(causal, kv_lens, dropout, doc, span, B, S, S, "attention_qkv")
    fused = qkv.is_cuda and qkv.dtype == torch.bfloat16 and D in (64, 128) and qkv.shape[-1] == W and \
        W % 8 == 0 and qkv.is_contiguous()
    if fused and _plan(mask.kind, D, B, S, S, heads, kv_heads, causal, kv_lens is not None, W)["ok"]:
        pos, table = rope if rope is not None else (None, None)
        return _FlashQKV.apply(qkv, B, S, heads, kv_heads, D, causal, kv_lens, scale, pos, table, bias_link,
                               rope_in_place, rope_applied, mask)
    if rope_applied:
        raise RuntimeError("attention_qkv: q / k rotated by the projection epilogue need the fused GPU path")
    q, k, v = qkv.split([heads * D, kv_heads * D, kv_heads * D], dim=-1)
    if rope is not None:
        from k8s_amd.ops import nn as _nn

        q, k = _nn.rope(q, rope[0], rope[1]), _nn.rope(k, rope[0], rope[1])
    return attention(q.reshape(B, S, heads, D), k.reshape(B, S, kv_heads, D), v.reshape(B, S, kv_heads, D),
                     causal=causal, kv_lens=kv_lens, scale=scale, dropout=dropout, doc=doc, span=span)
