"""Fused flat-buffer optimizers (K7 SGD+momentum, K8 Adam/AdamW).

One kernel launch updates every parameter of the model: fp32 master, fp32
state, gradient (fp32 or bf16) and the bf16 working copy in a single pass
over HBM (see ``csrc/kernels/optim.hip``). Gradient averaging for data
parallelism and gradient clipping are folded into the kernel's scale
(device-side clip factor: no host sync, hipGraph-capturable).

LARS and LAMB (``FusedLARS`` / ``FusedLAMB``) add a per-tensor trust ratio to the
two: four launches over a work-item table that knows where each parameter slot
begins and ends (``csrc/kernels/layerwise.hip``).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from k8s_amd.ops import reference as ref
from k8s_amd.ops._ext import load as _load_ext
from k8s_amd.parallel.flat import ParamStore


class _FlatOptimizer:
    # attribute -> state_dict key of every flat fp32 state buffer
    STATE: Dict[str, str] = {}

    def __init__(self, store: ParamStore, lr: float, weight_decay: float, max_grad_norm: Optional[float] = None):
        self.store = store
        self.lr = lr
        self.weight_decay = weight_decay
        self.max_grad_norm = max_grad_norm
        self.step_count = 0
        self.hyper: Optional[torch.Tensor] = None  # device [lr, step] (hipGraph replay), see use_device_hyper
        self.layout: Optional[List[Tuple[int, int, int]]] = None  # ZeRO-1 shard layout [(lo, hi, offset)]
        for attr in self.STATE:
            setattr(self, attr, torch.zeros_like(store.master))

    # ---- ZeRO-1: optimizer state only for the shards this rank owns
    def shard(self, ranges: Sequence[Tuple[int, int]]):
        """Keep state only for ``ranges`` of the flat buffers (the parameter service's owned shards), packed
        back to back: a rank then holds 1/world of the fp32 moments. ``step`` must be called with exactly
        these ranges afterwards."""
        layout, off = [], 0
        for lo, hi in ranges:
            layout.append((lo, hi, off))
            off += hi - lo
        self.layout = layout
        for attr in self.STATE:
            setattr(self, attr, torch.zeros(off, dtype=torch.float32, device=self.store.master.device))

    def _st(self, t: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
        """State slice for flat range [lo, hi) (a sub-range of one owned shard when sharded)."""
        if self.layout is None:
            return t[lo:hi]
        for a, b, off in self.layout:
            if a <= lo and hi <= b:
                return t[off + lo - a: off + hi - a]
        raise ValueError("range [%d, %d) is not owned by this rank's optimizer shard" % (lo, hi))

    def state_numel(self) -> int:
        return sum(getattr(self, a).numel() for a in self.STATE)

    def use_device_hyper(self):
        """Kernels read lr (and Adam's step) from a device tensor instead of launch arguments, so a step
        captured in a hipGraph replays with the current schedule (``utils/graph.StepGraph``)."""
        if self.hyper is None:
            self.hyper = torch.zeros(2, dtype=torch.float32, device=self.store.master.device)
        return self.hyper

    def set_hyper(self, lr: float, step: int):
        self.hyper[0].fill_(float(lr))
        self.hyper[1].fill_(float(step))

    def prepare_replay(self, lr: float):
        """Host bookkeeping + device hyperparameters for one replay of a captured step (mirrors ``step``)."""
        raise NotImplementedError

    def _ranges(self, ranges: Optional[Sequence[Tuple[int, int]]]) -> List[Tuple[int, int]]:
        return [(0, self.store.total)] if ranges is None else list(ranges)

    def _views(self, lo: int, hi: int):
        s = self.store
        return (s.master[lo:hi], s.grad[lo:hi], None if s.half is None else s.half[lo:hi],
                s.decay_mask[lo // 64: hi // 64])

    def _clip(self, scale: float, ranges, stats_reduce: Optional[Callable] = None) -> Optional[torch.Tensor]:
        """Device-side clip factor from the gradient norm over ``ranges``; ``stats_reduce`` (e.g. an
        all-reduce) combines the [sum of squares, non-finite count] partials of a sharded update. (Also the step's
        first read of the gradients.)"""
        if not self.max_grad_norm:
            return None
        g = self.store.grad
        if g.is_cuda:
            C = _load_ext()
            stats = None
            for lo, hi in ranges:
                st = C.grad_sumsq(g[lo:hi])
                stats = st if stats is None else stats + st
            if stats_reduce is not None:
                stats_reduce(stats)
            # the clip test sees the *scaled* (averaged) gradient norm
            stats[0:1].mul_(scale * scale)
            return C.clip_factor(stats, float(self.max_grad_norm))
        stats = sum(ref.grad_sumsq(g[lo:hi]) for lo, hi in ranges)
        if stats_reduce is not None:
            stats_reduce(stats)
        norm = float(stats[0].sqrt()) * scale
        f = min(1.0, self.max_grad_norm / (norm + 1e-6)) if bool(stats[1] == 0) else 0.0
        return torch.tensor([f])

    def state_tensors(self):
        return [getattr(self, a) for a in self.STATE]

    def state_dict(self, full: Optional[Dict[str, torch.Tensor]] = None):
        """Flat state by key; when sharded pass ``full`` (attribute -> full-size tensor, gathered by the
        parameter service) to get checkpointable whole-model tensors."""
        d = {key: (full[attr] if full is not None else getattr(self, attr)) for attr, key in self.STATE.items()}
        d["step"] = self.step_count
        return d

    def load_state_dict(self, sd):
        """Accepts whole-model flat tensors (a checkpoint); a sharded optimizer keeps its owned slices."""
        for attr, key in self.STATE.items():
            src, dst = sd[key], getattr(self, attr)
            if self.layout is None:
                dst.copy_(src.reshape(-1)[:dst.numel()])
            else:
                src = src.reshape(-1)
                for lo, hi, off in self.layout:
                    dst[off:off + hi - lo].copy_(src[lo:hi])
        self.step_count = int(sd["step"])


class FusedSGD(_FlatOptimizer):
    STATE = {"mom": "momentum_buffer"}

    def __init__(self, store: ParamStore, lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=False,
                 max_grad_norm=None):
        super().__init__(store, lr, weight_decay, max_grad_norm)
        self.momentum = momentum
        self.nesterov = nesterov

    def step(self, grad_scale: float = 1.0, lr: Optional[float] = None, ranges=None, stats_reduce=None):
        """Update the flat buffers (or only ``ranges`` of them: the shards this rank owns)."""
        lr = self.lr if lr is None else lr
        ranges = self._ranges(ranges)
        clip = self._clip(grad_scale, ranges, stats_reduce)
        first = self.step_count == 0
        for lo, hi in ranges:
            p, g, h, mask = self._views(lo, hi)
            m = self._st(self.mom, lo, hi)
            if p.is_cuda:
                _load_ext().fused_sgd(p, m, g, h, mask, lr, self.momentum, self.weight_decay, grad_scale, clip,
                                      self.nesterov, first, self.hyper)
            else:
                ref.sgd(p, m, g, h, mask, lr, self.momentum, self.weight_decay, grad_scale, clip, self.nesterov,
                        first)
        self.step_count += 1

    def prepare_replay(self, lr: float):
        if self.step_count == 0:
            raise RuntimeError("capture after at least one eager step (momentum initialisation)")
        self.set_hyper(lr, self.step_count)
        self.step_count += 1



class FusedAdam(_FlatOptimizer):
    STATE = {"m1": "exp_avg", "m2": "exp_avg_sq"}

    def __init__(self, store: ParamStore, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
                 adamw=True, max_grad_norm=None):
        super().__init__(store, lr, weight_decay, max_grad_norm)
        self.b1, self.b2 = betas
        self.eps = eps
        self.adamw = adamw

    def step(self, grad_scale: float = 1.0, lr: Optional[float] = None, ranges=None, stats_reduce=None):
        lr = self.lr if lr is None else lr
        ranges = self._ranges(ranges)
        clip = self._clip(grad_scale, ranges, stats_reduce)
        self.step_count += 1
        for lo, hi in ranges:
            p, g, h, mask = self._views(lo, hi)
            a, b = self._st(self.m1, lo, hi), self._st(self.m2, lo, hi)
            if p.is_cuda:
                _load_ext().fused_adam(p, a, b, g, h, mask, lr, self.b1, self.b2, self.eps, self.weight_decay,
                                       grad_scale, clip, self.step_count, self.adamw, self.hyper)
            else:
                ref.adam(p, a, b, g, h, mask, lr, self.b1, self.b2, self.eps, self.weight_decay, grad_scale, clip,
                         self.step_count, self.adamw)

    def prepare_replay(self, lr: float):
        self.step_count += 1
        self.set_hyper(lr, self.step_count)


# --------------------------------------------------------------------------- layer-wise adaptive (LARS / LAMB)
ITEM = 16384  # elements per work item, at most (the extension's layer_item_max)
DECAY, LOWP = 1, 2  # per-segment flag bits (csrc/kernels/layerwise.hip)


class _Table:
    """What a layer-wise step needs besides the flat buffers, built once per (store, ranges, shard layout).

    ``pieces``: [(flat lo, flat hi, state offset, segment)], one per (parameter slot x range) overlap, in
    parameter order, so a segment's pieces are contiguous; segment = ``Param.index``. A slot is its 64-aligned
    extent, the padding included (it holds zeros). Elements outside every slot belong to no piece. On the GPU the
    pieces are cut into work items of at most ``ITEM`` elements and handed to the extension, which validates them
    against the buffer sizes and keeps them on the device (``handle``); ``partial`` / ``sums`` / ``ratio`` are
    the step's persistent outputs (static addresses: a captured step replays on them)."""

    def __init__(self, opt: "_LayerwiseOptimizer", ranges: Sequence[Tuple[int, int]]):
        s = opt.store
        dev = s.master.device
        n = len(s.params)
        for lo, hi in ranges:
            if lo % 64 or hi % 64 or not 0 <= lo <= hi <= s.total:
                raise ValueError("range [%d, %d) must be 64-aligned and inside the store" % (lo, hi))
        self.pieces: List[Tuple[int, int, int, int]] = []
        for p in s.params:
            a, b = p.offset, p.offset + (p.numel + 63) // 64 * 64
            for lo, hi in ranges:
                x, y = max(a, lo), min(b, hi)
                if x < y:
                    self.pieces.append((x, y, opt._state_offset(x, y), p.index))
        offs = torch.tensor([p.offset // 64 for p in s.params], dtype=torch.long, device=dev)
        lowp = torch.tensor([LOWP if p.lowp else 0 for p in s.params], dtype=torch.uint8, device=dev)
        # the decay flag is the store's mask at the slot's first chunk (a chunk never straddles two slots)
        self.flags = (s.decay_mask.index_select(0, offs) != 0).to(torch.uint8) * DECAY + lowp
        self.decay = (self.flags & DECAY) != 0
        self.sums = torch.zeros(n, 2, dtype=torch.float32, device=dev)
        self.ratio = torch.ones(n, dtype=torch.float32, device=dev)
        self.handle = self.partial = None
        if dev.type == "cuda":
            C = _load_ext()
            assert C.layer_item_max == ITEM
            rows = []
            for x, y, so, seg in self.pieces:
                k = torch.arange(0, y - x, ITEM, dtype=torch.long)
                rows.append(torch.stack([x + k, so + k, torch.clamp(y - x - k, max=ITEM), torch.full_like(k, seg)], 1))
            items = torch.cat(rows) if rows else torch.zeros(0, 4, dtype=torch.long)
            self.handle = C.layer_table(items.contiguous(), s.total, opt.state_tensors()[0].numel(), n, dev)
            self.partial = torch.zeros(max(items.shape[0], 1) * 2, dtype=torch.float32, device=dev)[:items.shape[0] * 2]


class _LayerwiseOptimizer(_FlatOptimizer):
    """Per-tensor trust ratios on the flat store. A step is: clip (as the base class), pass 1 (per-item partial
    sums of p^2 and x^2; LAMB also advances its moments here), fold (per-slot sums), ``stats_reduce(sums)`` (the
    ZeRO-1 all-reduce: a slot's norm covers every rank's pieces), ratio, pass 2 (the update). Nothing reads the
    device from the host, so the step captures into a hipGraph like the SGD / Adam ones. A skipped step (zero clip
    factor) leaves every buffer, ``last_trust_ratio`` included, as it was. The passes use no atomics and a fixed
    summation order: without ``max_grad_norm`` (whose global norm is the base class's atomics-based one) a step is
    bitwise reproducible."""

    LAMB = False

    def __init__(self, store, lr, weight_decay, max_grad_norm=None):
        super().__init__(store, lr, weight_decay, max_grad_norm)
        self._tables: Dict[tuple, _Table] = {}
        self.last_trust_ratio: Optional[torch.Tensor] = None  # device fp32 [len(store.params)], latest step
        self.last_sums: Optional[torch.Tensor] = None  # its [len(store.params)][2] sums of p^2 and x^2 (reduced)

    def shard(self, ranges):
        super().shard(ranges)
        self._tables = {}

    def _state_offset(self, lo: int, hi: int) -> int:
        if self.layout is None:
            return lo
        for a, b, off in self.layout:
            if a <= lo and hi <= b:
                return off + lo - a
        raise ValueError("range [%d, %d) is not owned by this rank's optimizer shard" % (lo, hi))

    def _table(self, ranges) -> _Table:
        key = tuple(ranges)
        if key not in self._tables:
            self._tables[key] = _Table(self, ranges)
        return self._tables[key]

    def trust_ratio_stats(self) -> Optional[Dict[str, float]]:
        """min / mean / max of the latest trust ratios over the decaying slots (one host read)."""
        if self.last_trust_ratio is None:
            return None
        tab = next(iter(self._tables.values()))
        r = self.last_trust_ratio[tab.decay]
        if r.numel() == 0:
            return None
        lo, mean, hi = torch.stack([r.min(), r.mean(), r.max()]).tolist()
        return {"trust_ratio_min": lo, "trust_ratio_mean": mean, "trust_ratio_max": hi}

    # the per-optimizer parts of a step
    def _args(self):  # (eta, mu, b1, b2, eps) with the other family's values unused
        raise NotImplementedError

    def _layer_step(self, grad_scale, lr, ranges, stats_reduce, step, first):
        ranges = self._ranges(ranges)
        clip = self._clip(grad_scale, ranges, stats_reduce)
        tab = self._table(ranges)
        s = self.store
        eta, mu, b1, b2, eps = self._args()
        wd = self.weight_decay
        st = self.state_tensors()
        if s.master.is_cuda:
            C = _load_ext()
            m1, m2 = (st[0], st[1]) if self.LAMB else (None, None)
            C.layer_sums(tab.handle, s.master, m1, m2, s.grad, tab.flags, tab.partial, b1, b2, eps, wd, grad_scale,
                         clip, step, self.hyper)
            C.layer_fold(tab.handle, tab.partial, tab.sums, clip)
            if stats_reduce is not None:
                stats_reduce(tab.sums)
            C.layer_ratio(tab.handle, tab.sums, tab.flags, tab.ratio, self.LAMB, eta, wd, clip)
            C.layer_update(tab.handle, s.master, st[0], st[1] if self.LAMB else None, s.grad, s.half, tab.flags,
                           tab.ratio, lr, mu, b1, b2, eps, wd, grad_scale, clip, step, first, self.hyper)
        elif not ref._skipped(clip):
            sc = grad_scale * (float(clip.reshape(-1)[0]) if clip is not None else 1.0)
            decay = tab.decay.tolist()
            tab.sums.zero_()
            for x, y, so, seg in tab.pieces:
                p, g, w = s.master[x:y], s.grad[x:y], (wd if decay[seg] else 0.0)
                if self.LAMB:
                    a, b = st[0][so:so + y - x], st[1][so:so + y - x]
                    ref.lamb_moments(a, b, g, sc, b1, b2)
                    tab.sums[seg] += ref.layer_sums(p, ref.lamb_u(p, a, b, b1, b2, eps, w, step))
                else:
                    tab.sums[seg] += ref.layer_sums(p, g.float() * sc)
            if stats_reduce is not None:
                stats_reduce(tab.sums)
            tab.ratio.copy_(ref.trust_ratio(tab.sums, tab.decay, self.LAMB, eta, wd))
            ratio = tab.ratio.tolist()
            for x, y, so, seg in tab.pieces:
                p, w = s.master[x:y], (wd if decay[seg] else 0.0)
                h = s.half[x:y] if (s.half is not None and s.params[seg].lowp) else None
                if self.LAMB:
                    ref.lamb(p, st[0][so:so + y - x], st[1][so:so + y - x], h, ratio[seg], lr, b1, b2, eps, w, step)
                else:
                    ref.lars(p, st[0][so:so + y - x], s.grad[x:y], h, ratio[seg], lr, mu, w, sc, first)
        self.last_trust_ratio, self.last_sums = tab.ratio, tab.sums


class FusedLARS(_LayerwiseOptimizer):
    """LARS on momentum SGD: per slot r = eta ||p|| / (||g|| + wd ||p||) where the slot decays and both norms are
    positive, else 1; d = r (g + wd_slot p); m = mu m + d (m = d on the first step); p -= lr m. No Nesterov."""
    STATE = {"mom": "momentum_buffer"}

    def __init__(self, store: ParamStore, lr=0.1, momentum=0.9, weight_decay=1e-4, trust_coef=0.001,
                 max_grad_norm=None):
        super().__init__(store, lr, weight_decay, max_grad_norm)
        self.momentum = momentum
        self.trust_coef = trust_coef

    def _args(self):
        return self.trust_coef, self.momentum, 0.0, 0.0, 0.0

    def step(self, grad_scale: float = 1.0, lr: Optional[float] = None, ranges=None, stats_reduce=None):
        self._layer_step(grad_scale, self.lr if lr is None else lr, ranges, stats_reduce, 0, self.step_count == 0)
        self.step_count += 1

    def prepare_replay(self, lr: float):
        if self.step_count == 0:
            raise RuntimeError("capture after at least one eager step (momentum initialisation)")
        self.set_hyper(lr, self.step_count)
        self.step_count += 1


class FusedLAMB(_LayerwiseOptimizer):
    """LAMB: Adam moments, u = m_hat / (sqrt(v_hat) + eps) + wd_slot p, per slot r = ||p|| / ||u|| where the slot
    decays and both norms are positive, else 1; p -= lr r u."""
    STATE = {"m1": "exp_avg", "m2": "exp_avg_sq"}
    LAMB = True

    def __init__(self, store: ParamStore, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01,
                 max_grad_norm=None):
        super().__init__(store, lr, weight_decay, max_grad_norm)
        self.b1, self.b2 = betas
        self.eps = eps

    def _args(self):
        return 0.0, 0.0, self.b1, self.b2, self.eps

    def step(self, grad_scale: float = 1.0, lr: Optional[float] = None, ranges=None, stats_reduce=None):
        self.step_count += 1
        self._layer_step(grad_scale, self.lr if lr is None else lr, ranges, stats_reduce, self.step_count, False)

    def prepare_replay(self, lr: float):
        self.step_count += 1
        self.set_hyper(lr, self.step_count)


# --------------------------------------------------------------------------- gradient accumulation
def grad_accumulate(acc: torch.Tensor, g: torch.Tensor, lo: int, hi: int, first: bool) -> None:
    """``acc[lo:hi] = g[lo:hi] if first else acc[lo:hi] + g[lo:hi]`` on two flat fp32 buffers of one layout
    (``csrc/kernels/accum.hip``); ``lo`` / ``hi`` are multiples of 64."""
    if acc.is_cuda or g.is_cuda:
        _load_ext().grad_accumulate(acc, g, lo, hi, bool(first))
    else:
        ref.grad_accumulate(acc, g, lo, hi, first)


def grad_fold(g: torch.Tensor, acc: torch.Tensor, lo: int, hi: int, out_bf: Optional[torch.Tensor] = None) -> None:
    """``g[lo:hi] = g[lo:hi] + acc[lo:hi]`` and, with ``out_bf`` (bf16, at least ``hi - lo`` elements), the same
    pass stores ``bf16(g[lo:hi])`` at its start (round to nearest even)."""
    if g.is_cuda or acc.is_cuda:
        _load_ext().grad_fold(g, acc, lo, hi, out_bf)
    else:
        ref.grad_fold(g, acc, lo, hi, out_bf)
