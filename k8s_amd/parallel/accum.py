"""Gradient accumulation on the flat gradient buffer.

An optimizer step over ``steps`` micro-batches. The accumulated gradient is the MEAN of the micro-batches'
gradients, each of its own mean loss -- the definition data parallelism already uses across ranks, so ``world``
ranks x ``steps`` micro-batches equal ``world * steps`` ranks.

Every micro-batch runs on the store-once fast paths unchanged (``ParamStore.begin_step`` clears ``Param.written``,
the backward kernels overwrite their slots). Accumulation is paid for with two streaming kernels over the flat
gradient (``csrc/kernels/accum.hip``):

* after each micro-batch but the last, ``accumulate(first)`` adds ``store.grad`` to one fp32 buffer of the same layout
  (a copy for the first micro-batch: the buffer is never zero-filled);
* on the last micro-batch the running sum is folded into ``store.grad`` range by range (``fold``), by the gradient
  transport as each bucket becomes ready and right before its collective (``parallel/ddp.py``, ``parallel/ps.py``),
  so communication still overlaps the last backward. With the bf16 transport the fold also writes the bucket's bf16
  send buffer, which replaces the transport's cast pass.

The sum stays unscaled in fp32: ``scale`` (1 / steps) goes into the optimizer's ``grad_scale`` next to 1 / world,
which the clip statistics and the LARS / LAMB sums already honour. Each element is a fixed-order fp32 sum
``g_last + (((g_1 + g_2) + g_3) + ...)``, so the layer-wise optimizers keep their bitwise reproducibility.

Memory: 4 B per parameter (32 GB for Llama-3-8B), allocated on the first ``accumulate`` and only when ``steps > 1``.
BatchNorm layers normalise each micro-batch by its own statistics (as each rank does under data parallelism).
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Tuple

import torch

from k8s_amd.ops.optim import grad_accumulate, grad_fold
from k8s_amd.parallel.flat import ParamStore


class GradAccumulator:
    def __init__(self, store: ParamStore, steps: int):
        steps = int(steps)
        if steps < 1:
            raise ValueError("steps must be >= 1")
        if steps > 1 and store.grad.dtype != torch.float32:
            raise ValueError("gradient accumulation needs an fp32 gradient store, not %s" % store.grad.dtype)
        self.store = store
        self.steps = steps
        self.buf: Optional[torch.Tensor] = None
        self.count = 0  # micro-batches in the buffer since the last fold
        self.folded: List[Tuple[int, int]] = []  # ranges folded in this optimizer step

    @property
    def active(self) -> bool:
        return self.steps > 1

    @property
    def scale(self) -> float:
        return 1.0 / self.steps

    def accumulate(self, first: bool) -> None:
        """Close a non-final micro-batch: zero the slots its backward never wrote, then add the whole gradient buffer
        to the running sum (``first``: start the sum with it)."""
        if not self.active:
            raise RuntimeError("steps == 1: there is no non-final micro-batch to accumulate")
        if bool(first) != (self.count == 0) or self.count >= self.steps - 1 or self.folded:
            raise RuntimeError("accumulate(first=%s) as micro-batch %d of %d" % (first, self.count, self.steps))
        s = self.store
        s.zero_unwritten()
        if self.buf is None:
            self.buf = torch.empty_like(s.grad)
        grad_accumulate(self.buf, s.grad, 0, s.total, bool(first))
        self.count += 1

    def fold(self, lo: int, hi: int, out_bf: Optional[torch.Tensor] = None) -> None:
        """Last micro-batch: ``store.grad[lo:hi] += running sum`` (and ``out_bf[:hi - lo]`` = its bf16 rounding)."""
        if hi == lo:
            return
        assert self.count == self.steps - 1, "fold after %d of %d micro-batches" % (self.count + 1, self.steps)
        assert all(hi <= a or b <= lo for a, b in self.folded), "range [%d, %d) folded twice" % (lo, hi)
        self.folded.append((lo, hi))
        grad_fold(self.store.grad, self.buf, lo, hi, out_bf)

    def end_step(self, ranges: Iterable[Tuple[int, int]]) -> None:
        """The transport's ranges must each have been folded exactly once; ready for the next optimizer step."""
        assert sorted(self.folded) == sorted((lo, hi) for lo, hi in ranges if hi > lo), "ranges not folded exactly once"
        self.folded = []
        self.count = 0
