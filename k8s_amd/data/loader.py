"""From a split on disk to the stem's input: indices and table rows (``sampler``), then one ``ops.data.augment`` call.

Two GPU modes, chosen by ``resident_gb``, end in the same kernel call and produce the same bits:

* resident: the split (at most ``resident_gb`` GiB) is uploaded once as uint8 and the table's indices address it;
* streamed: one background thread gathers the next batch's rows from the memory map into one of two pinned
  [N, Hs, Ws, 3] buffers, copies it on a side stream and records an event; the table then indexes 0..N-1 and the
  compute stream waits on the event (the host does not). The thread prefetches batch ``t + 1`` while ``t`` runs; a
  request for any other index restarts the prefetch from there.

On the CPU the batch's rows are gathered from the memory map and ``ops.reference.augment`` runs on them.
"""
from __future__ import annotations

import time
from concurrent.futures import ThreadPoolExecutor
from typing import Optional, Tuple

import numpy as np
import torch

from k8s_amd.data import sampler
from k8s_amd.data.dataset import Dataset
from k8s_amd.ops import data as kdata


def is_resident(nbytes: int, resident_gb: float, device) -> bool:
    """Resident mode: a GPU run whose split fits ``resident_gb`` GiB (0: always streamed)."""
    return bool(torch.device(device).type == "cuda" and resident_gb > 0 and nbytes <= resident_gb * 2 ** 30)


class _Streamer:
    """The background gather + upload of streamed mode. ``get(key, rows)`` returns the device buffer that holds the
    source rows of request ``key`` and starts on ``next_key``; ``done(slot)`` marks the buffer's consumer launched."""

    def __init__(self, images: np.ndarray, n: int, device, rows_of, gather=None, shape=None, dtype=torch.uint8):
        """``gather(rows, out)`` (default: ``np.take`` of ``images``' rows) fills the pinned numpy buffer ``out`` of
        ``shape`` (default: ``n`` source images) from what ``rows_of(key)`` returned."""
        self.images, self.rows_of, self.device = images, rows_of, device
        self.gather = gather or (lambda rows, out: np.take(self.images, rows, axis=0, out=out, mode="clip"))
        shape = shape or ((n,) + tuple(images.shape[1:]))
        self.pinned = [torch.empty(shape, dtype=dtype).pin_memory() for _ in range(2)]
        self.staged = [torch.empty(shape, dtype=dtype, device=device) for _ in range(2)]
        self.copied = [torch.cuda.Event() for _ in range(2)]
        self.consumed = [torch.cuda.Event() for _ in range(2)]
        self.stream = torch.cuda.Stream(device)
        self.pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="k8s_amd-data")
        self.pending = None  # (key, future) of the prefetch in flight
        self.count = 0
        self.gather_s, self.gather_bytes, self.restarts = 0.0, 0, 0
        self.requests, self.pending_copies = 0, 0  # batches handed out / of them, upload unfinished when asked for

    def _work(self, key, slot):
        rows = self.rows_of(key)
        self.copied[slot].synchronize()  # the pinned buffer's previous upload has left it
        t0 = time.perf_counter()
        self.gather(rows, self.pinned[slot].numpy())
        self.gather_s += time.perf_counter() - t0
        self.gather_bytes += self.pinned[slot].numel() * self.pinned[slot].element_size()
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(self.consumed[slot])  # the kernel that read this device buffer last
            self.staged[slot].copy_(self.pinned[slot], non_blocking=True)
            self.copied[slot].record(self.stream)
        return slot

    def _submit(self, key):
        fut = self.pool.submit(self._work, key, self.count % 2)
        self.count += 1
        return key, fut

    def get(self, key, next_key) -> Tuple[torch.Tensor, int]:
        if self.pending is not None and self.pending[0] != key:
            self.pending[1].result()  # a resume or another order: the prefetch starts over from `key`
            self.pending = None
            self.restarts += 1
        _, fut = self.pending if self.pending is not None else self._submit(key)
        slot = fut.result()
        self.pending = self._submit(next_key) if next_key is not None else None
        self.requests += 1
        self.pending_copies += not self.copied[slot].query()
        torch.cuda.current_stream(self.device).wait_event(self.copied[slot])
        return self.staged[slot], slot

    def done(self, slot):
        self.consumed[slot].record(torch.cuda.current_stream(self.device))

    def close(self):
        self.pool.shutdown(wait=True, cancel_futures=True)
        self.pending = None


class Loader:
    """Batches of one split. ``train``: batch ``t`` of this rank by ``sampler.batch_indices`` / ``train_table``;
    otherwise evaluation batch ``i`` = samples ``[(i * world + r) * batch, + batch)`` with centred rows, and rows past
    the end of the split carry label -100. ``batch(t)`` -> (stem input, int64 labels), both on ``device``."""

    def __init__(self, ds: Dataset, split: str, device, batch: int, image: Optional[int] = None,
                 augment: str = "crop", crop_pad: int = 4, seed: int = 0, rank: int = 0, world: int = 1,
                 resident_gb: float = 4.0, train: bool = True, layout: Optional[str] = None, dtype=None):
        self.ds, self.split, self.device = ds, ds.split(split), torch.device(device)
        self.images, self.labels = self.split.images, self.split.labels
        self.M, self.Hs, self.Ws = (int(v) for v in self.images.shape[:3])
        self.batch_size, self.augment, self.pad, self.train = int(batch), augment, int(crop_pad), train
        self.seed, self.rank, self.world = int(seed), int(rank), int(world)
        self.S = int(image) if image else min(self.Hs, self.Ws)
        sampler.check_geometry(augment, self.Hs, self.Ws, self.S, self.pad)
        self.steps_per_epoch = sampler.steps_per_epoch(self.M, self.batch_size, self.world) if train else None
        self.a, self.b = kdata.norm_constants(ds.mean, ds.std)
        gpu = self.device.type == "cuda"
        self.layout = layout or ("s2d" if gpu else "nhwc8")
        self.dtype = dtype or (torch.bfloat16 if gpu else torch.float32)
        self.resident = is_resident(self.split.nbytes, resident_gb, self.device)
        self.src, self.streamer = None, None
        if self.resident:
            self.src = torch.from_numpy(np.array(self.images)).to(self.device)  # one read of the map, one upload
        elif gpu:
            self.streamer = _Streamer(self.images, self.batch_size, self.device, lambda t: self.rows(t)[0])

    # ------------------------------------------------------------------ what batch t is
    def rows(self, t: int):
        """(source indices int64 [N], labels int64 [N]) of batch ``t``."""
        if self.train:
            idx = sampler.batch_indices(self.seed, t, self.rank, self.world, self.batch_size, self.M)
            return idx, self.labels[idx]
        idx = (t * self.world + self.rank) * self.batch_size + np.arange(self.batch_size, dtype=np.int64)
        real = idx < self.M
        idx = np.where(real, idx, 0)
        return idx, np.where(real, self.labels[idx], -100)

    def table(self, t: int, indices) -> np.ndarray:
        if self.train:
            return sampler.train_table(indices, self.seed, t, self.rank, self.Hs, self.Ws, self.S, self.augment,
                                       self.pad)
        return sampler.eval_table(indices, self.Hs, self.Ws, self.S, self.augment)

    def batch(self, t: int):
        t = int(t)
        idx, labels = self.rows(t)
        local = np.arange(self.batch_size, dtype=np.int64)
        slot = None
        if self.resident:
            src, tab = self.src, self.table(t, idx)
        elif self.streamer is not None:
            src, slot = self.streamer.get(t, t + 1)
            tab = self.table(t, local)
        else:  # CPU: this batch's rows, then the reference
            src, tab = torch.from_numpy(np.take(self.images, idx, axis=0)), self.table(t, local)
        x = kdata.augment(src, torch.from_numpy(tab), self.a, self.b, self.S, self.layout)
        if slot is not None:
            self.streamer.done(slot)
        if x.dtype != self.dtype:
            x = x.to(self.dtype)
        y = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64))
        if x.is_cuda:  # pinned and asynchronous, like the table: the host never waits for the stream
            y = y.pin_memory().to(self.device, non_blocking=True)
        return x, y

    def info(self) -> dict:
        out = {"resident": self.resident}
        if self.streamer is not None and self.streamer.gather_s > 0:
            out["gather_gb_per_s"] = round(self.streamer.gather_bytes / self.streamer.gather_s / 1e9, 3)
            out["restarts"] = self.streamer.restarts
            # an upload still in flight when the host asked for its batch (the compute stream may then wait on the event;
            # finished uploads never make it wait)
            out["uploads_pending_at_request"] = [self.streamer.pending_copies, self.streamer.requests]
        return out

    def close(self):
        if self.streamer is not None:
            self.streamer.close()
            self.streamer = None
