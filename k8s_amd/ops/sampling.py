"""Next-token sampling for generation: greedy and top-k, in torch (16 x 128,256 numbers per step is not a hot path).

Ranks follow ``xent_eval``'s rule: column j ranks before column i when its logit is larger, or equal with j < i.
``temperature == 0`` takes the column of rank 0. Otherwise the candidates are the ``top_k`` (1 .. 64) columns of rank
< top_k in rank order, p_j = softmax(l_j / T) over them in fp32, and the token is the first candidate whose running sum
reaches u * sum, with u = (h + 0.5) / 2^32 and h the project's counter generator (``ops.reference.counter_bits``) at
(seed, step = index of the generated token, site 0, row, column 0). A draw is a pure function of (seed, step, row,
logits): generation is reproducible and can resume at any token.
"""
from __future__ import annotations

import torch

from k8s_amd.ops import reference as ref

MAX_TOP_K = 64


def greedy(logits):
    """int64 [B]: the arg-max of every row of [B, V] logits, ties to the lower index."""
    lf = logits.float()
    V = lf.shape[-1]
    top = lf.max(-1, keepdim=True).values
    idx = torch.arange(V, device=lf.device).expand_as(lf)
    return torch.where(lf == top, idx, torch.full_like(idx, V)).min(-1).values.clamp_max(V - 1)


def uniform(seed: int, step: int, rows):
    """fp64 [len(rows)] in (0, 1): (h + 0.5) / 2^32 of the counter generator at (seed, step, site 0, row, col 0)."""
    rows = torch.as_tensor(rows, dtype=torch.int64)
    h = ref.counter_bits((int(seed), int(step)), 0, rows.cpu(), torch.zeros(1, dtype=torch.int64))[:, 0]
    return (h.double() + 0.5) / 4294967296.0


def candidates(logits, top_k: int):
    """(values fp32 [B, top_k], columns int64 [B, top_k]): the columns of rank < top_k in rank order."""
    # a stable descending sort keeps equal logits in column order: exactly the rank rule
    vals, cols = torch.sort(logits.float(), dim=-1, descending=True, stable=True)
    return vals[:, :top_k].contiguous(), cols[:, :top_k].contiguous()


def sample(logits, temperature: float, top_k: int, seed: int, step: int, rows=None):
    """int64 [B] tokens of [B, V] logits; ``rows``: the rows' indices in the generator (default 0 .. B - 1)."""
    if temperature == 0:
        return greedy(logits)
    if temperature < 0:
        raise ValueError("temperature must not be negative, got %r" % (temperature,))
    if not 1 <= int(top_k) <= MAX_TOP_K:
        raise ValueError("top_k must be in [1, %d], got %r" % (MAX_TOP_K, top_k))
    B, V = logits.shape
    k = min(int(top_k), V)
    vals, cols = candidates(logits, k)
    p = torch.softmax(vals / float(temperature), -1)
    run = torch.cumsum(p, -1)
    u = uniform(seed, step, torch.arange(B) if rows is None else rows).to(run.device)
    reach = run.double() >= (u * run[:, -1].double())[:, None]
    first = torch.where(reach, torch.arange(k, device=run.device).expand(B, k), torch.full((B, k), k - 1,
                                                                                          device=run.device))
    return cols.gather(1, first.min(-1, keepdim=True).values)[:, 0]
