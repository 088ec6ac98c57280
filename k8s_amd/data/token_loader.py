"""From a token split on disk to a model's input: items and table rows (``token_sampler``), then one
``ops.data.mlm_batch`` (BERT) or ``ops.data.causal_batch`` (Llama) call.

As ``loader.Loader``, three paths end in the same call and produce the same bits:

* resident: the split's tokens (at most ``resident_gb`` GiB) are uploaded once and the table's offsets address them;
* streamed: the background thread of ``loader._Streamer`` gathers each sample's A and B tokens (Llama: its window of
  ``S + 1`` tokens) back to back into one of two pinned compact buffers and copies it on the side stream; the table is
  rebased to offsets in that buffer and the compute stream waits on the copy's event;
* CPU: the same compact buffer, then ``ops.reference``.

``batch(t)`` returns, for BERT, ``(ids, token_types, labels [N, P], nsp, positions [N, P], kv_lens)`` --
``BertForPreTraining.forward``'s positional order, so the real sequence lengths reach attention -- and for Llama
``(ids, labels)``, or with ``doc_mask=True`` ``(ids, labels, lo, hi, pos)`` from one ``ops.data.causal_doc_batch`` call:
the bounds of every token's document inside its row, positions that restart at each document, and -100 labels on every
document's last token -- ``LlamaForCausalLM.forward``'s positional order.

``unpad=True`` (BERT): one ``ops.data.mlm_batch_unpadded`` call writes the batch as one token stream, the sequences back
to back, and ``batch(t)`` returns ``(ids, token_types, pos, labels [N, P], nsp, rows [N, P], cls_rows, lo, hi)`` --
``BertForPreTraining.forward_unpadded``'s positional order. The stream offsets ``cu`` come from the plan's ``kv_lens``
on the host, so nothing reads the device.
"""
from __future__ import annotations

import numpy as np
import torch

from k8s_amd.data import token_sampler as ts
from k8s_amd.data.dataset import DataError
from k8s_amd.data.loader import _Streamer, is_resident
from k8s_amd.data.tokens import TokenDataset
from k8s_amd.ops import data as kdata

KINDS = ("bert", "llama")


def _as_torch(tokens: np.ndarray) -> torch.Tensor:
    """A token array as the tensor the ops take: uint16 data as an int16 view."""
    return torch.from_numpy(tokens.view(np.int16) if tokens.dtype == np.uint16 else tokens)


class TokenLoader:
    """Batches of one split for a ``kind`` ("bert" or "llama") model. ``train``: batch ``t`` of this rank by
    ``token_sampler.train_items``; otherwise evaluation batch ``i`` in split order (``stream = 1``), rows past the end
    carrying only -100 labels."""

    def __init__(self, ds: TokenDataset, split: str, device, batch: int, seq: int, kind: str = "bert",
                 max_predictions: int = 20, seed: int = 0, rank: int = 0, world: int = 1, resident_gb: float = 4.0,
                 train: bool = True, doc_mask: bool = False, unpad: bool = False):
        assert kind in KINDS
        self.unpad = bool(unpad)
        if self.unpad and (kind != "bert" or doc_mask):
            raise DataError("unpadded batches are implemented for the BERT models only (not Llama, not with a "
                            "document mask)")
        self.ds, self.split, self.device, self.kind = ds, ds.split(split), torch.device(device), kind
        self.tokens = self.split.tokens
        self.batch_size, self.S, self.P, self.train = int(batch), int(seq), int(max_predictions), train
        self.seed, self.rank, self.world = int(seed), int(rank), int(world)
        self.stream = 0 if train else 1
        self.doc_mask, self.doc_tok_host, self.doc_tok = bool(doc_mask), None, None
        if self.doc_mask:
            if kind != "llama":
                raise DataError("document-boundary masks are implemented for the Llama models only")
            if self.split.segments is None or self.split.docs is None:
                raise DataError("dataset %s: a document mask needs %s_segments.npy and %s_docs.npy"
                                % (ds.path, split, split))
            self.doc_tok_host = np.ascontiguousarray(self.split.segments[self.split.docs], dtype=np.int64)
        if kind == "bert":
            ts.check_seq(self.S, self.P)
            if ds.special is None or self.split.segments is None or self.split.docs is None or self.split.D < 2:
                raise DataError("dataset %s: BERT needs the special ids, %s_segments.npy and %s_docs.npy with at "
                                "least two documents" % (ds.path, split, split))
            self.items, self.what = self.split.G, "segments"
            self.capacity = self.batch_size * (self.S - 3)
        else:
            if self.S < 1:
                raise DataError("--seq must be positive, got %d" % self.S)
            self.items, self.what = ts.windows(self.split.T, self.S), "windows of %d tokens" % self.S
            self.capacity = self.batch_size * (self.S + 1)
            if self.items < 1:
                raise DataError("the %s split's %d tokens hold no window of --seq %d + 1" % (split, self.split.T,
                                                                                             self.S))
        self.steps_per_epoch = ts.steps_per_epoch(self.items, self.batch_size, self.world, self.what) if train \
            else None
        gpu = self.device.type == "cuda"
        self.resident = is_resident(self.split.nbytes, resident_gb, self.device)
        self.src, self.streamer, self._plans = None, None, {}
        self.last_real_tokens = 0  # non-pad positions of the batch ``batch`` returned last (from its host plan)
        if self.doc_mask:  # checked on the host and uploaded once
            self.doc_tok = kdata.doc_offsets(self.doc_tok_host, self.device)
        if self.resident:
            self.src = _as_torch(np.array(self.tokens)).to(self.device)  # one read of the map, one upload
        elif gpu:
            dtype = torch.int16 if self.tokens.dtype == np.uint16 else torch.int32
            self.streamer = _Streamer(None, self.batch_size, self.device, self._plan_for_thread,
                                      gather=lambda plan, out: self.compact(plan, out), shape=(self.capacity,),
                                      dtype=dtype)

    # ------------------------------------------------------------------ what batch t is
    def plan(self, t: int) -> dict:
        """The host side of batch ``t``: {"table" int64 [N, 6] (BERT) or "starts" int64 [N] (Llama), with offsets
        into the split; "nsp", "kv_lens" (BERT); "real" bool [N] or None (every row real)}."""
        if self.train:
            idx, ords = ts.train_items(self.seed, t, self.rank, self.world, self.batch_size, self.items)
            real = None
        else:
            idx, ords, real = ts.eval_items(t, self.rank, self.world, self.batch_size, self.items)
            real = None if bool(real.all()) else real
        if self.kind == "llama":
            return {"starts": idx * self.S, "real": real}
        tab, nsp, lens = ts.pair_rows(self.split.segments, self.split.docs, idx, ords, self.seed, self.S, self.P,
                                      self.stream)
        if real is not None:
            nsp = np.where(real, nsp, -100)
        return {"table": tab, "nsp": nsp, "kv_lens": lens, "real": real}

    @staticmethod
    def stream_offsets(plan: dict):
        """(cu int64 [N + 1], T) of an unpadded batch from its host plan: the sequences' first stream rows and the
        stream's row count, their total rounded up to a multiple of 128."""
        cu = np.zeros(len(plan["kv_lens"]) + 1, dtype=np.int64)
        np.cumsum(plan["kv_lens"], out=cu[1:])
        return cu, (int(cu[-1]) + 127) // 128 * 128

    def stream_rows(self, t: int = 0) -> int:
        """Rows of batch ``t``'s unpadded stream (from the host table)."""
        return self.stream_offsets(self.plan(t))[1]

    def real_tokens(self, t: int) -> int:
        """Non-pad positions of batch ``t`` (from the host table; every position of a causal window)."""
        if self.kind == "llama":
            return self.batch_size * self.S
        return int(self.plan(t)["kv_lens"].sum())

    def compact(self, plan: dict, out: np.ndarray) -> None:
        """Gather the batch's tokens back to back into ``out`` ([capacity], the tokens' dtype or its int16 view) and
        add the rebased table (``"local"``) to ``plan``."""
        out = out.view(self.tokens.dtype)
        if self.kind == "llama":
            w = self.S + 1
            at = plan["starts"][:, None] + np.arange(w, dtype=np.int64)
            out[:at.size] = self.tokens[at.reshape(-1)]
            plan["local"] = np.arange(len(at), dtype=np.int64) * w
            return
        tab = plan["table"]
        starts = tab[:, [0, 2]].reshape(-1)
        lens = tab[:, [1, 3]].reshape(-1)
        offs = np.cumsum(lens) - lens
        total = int(lens.sum())
        out[:total] = self.tokens[np.repeat(starts - offs, lens) + np.arange(total, dtype=np.int64)]
        local = tab.copy()
        local[:, 0], local[:, 2] = offs[0::2], offs[1::2]
        plan["local"] = local

    def _plan_for_thread(self, t: int) -> dict:
        plan = self.plan(t)
        self._plans[t] = plan  # read by batch(t) after the future's result: the gather has added "local"
        return plan

    def batch(self, t: int):
        t = int(t)
        slot = None
        if self.resident:
            plan = self.plan(t)
            src, rows = self.src, plan["starts" if self.kind == "llama" else "table"]
        elif self.streamer is not None:
            src, slot = self.streamer.get(t, t + 1)
            plan = self._plans.pop(t)
            for k in list(self._plans):  # prefetches a restart abandoned
                if k != t + 1:
                    self._plans.pop(k, None)
            rows = plan["local"]
        else:  # CPU: the compact buffer, then the reference
            plan = self.plan(t)
            buf = np.empty(self.capacity, dtype=self.tokens.dtype)
            self.compact(plan, buf)
            src, rows = _as_torch(buf), plan["local"]
        rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64))
        self.last_real_tokens = self.batch_size * self.S if self.kind == "llama" else int(plan["kv_lens"].sum())
        doc = ()
        if self.kind == "llama" and self.doc_mask:
            at = torch.from_numpy(np.ascontiguousarray(plan["starts"], dtype=np.int64))
            ids, labels, *doc = kdata.causal_doc_batch(src, rows, at, self.doc_tok, self.S, self.split.T)
        elif self.kind == "llama":
            ids, labels = kdata.causal_batch(src, rows, self.S)
        elif self.unpad:
            cu, T = self.stream_offsets(plan)
            ids, types, pos, labels, positions, cls_rows, lo, hi = kdata.mlm_batch_unpadded(
                src, rows, torch.from_numpy(cu), T, self.S, self.P, self.ds.vocab, self.ds.special, self.seed,
                self.stream)
        else:
            ids, types, labels, positions = kdata.mlm_batch(src, rows, self.S, self.P, self.ds.vocab, self.ds.special,
                                                            self.seed, self.stream)
        if slot is not None:
            self.streamer.done(slot)
        if plan["real"] is not None:  # evaluation rows past the end of the split: no label counts
            labels = labels.masked_fill(~self._upload(plan["real"]).unsqueeze(1), -100)
        if self.kind == "llama":
            return (ids, labels) + tuple(doc)
        if self.unpad:
            return (ids, types, pos, labels, self._upload(plan["nsp"]), positions, cls_rows, lo, hi)
        return (ids, types, labels, self._upload(plan["nsp"]), positions,
                self._upload(plan["kv_lens"].astype(np.int32)))

    def _upload(self, arr: np.ndarray) -> torch.Tensor:
        x = torch.from_numpy(np.ascontiguousarray(arr))
        if self.device.type == "cuda":  # pinned and asynchronous, like the table: the host never waits for the stream
            x = x.pin_memory().to(self.device, non_blocking=True)
        return x

    def pad_fraction(self, t: int = 0) -> float:
        """The mean share of pad positions in batch ``t`` (from the host table; 0 for causal windows)."""
        if self.kind == "llama":
            return 0.0
        return float(1.0 - self.plan(t)["kv_lens"].mean() / self.S)

    def docs_per_row(self, t: int = 0) -> float:
        """The mean number of documents a row of batch ``t`` holds (from the host tables)."""
        at = self.plan(t)["starts"]
        first = np.searchsorted(self.doc_tok_host, at, side="right")
        last = np.searchsorted(self.doc_tok_host, at + self.S - 1, side="right")
        return float((last - first + 1).mean())

    def info(self) -> dict:
        out = {"resident": self.resident}
        if self.unpad:
            out.update(unpad=True, stream_rows=self.stream_rows(0))
        if self.doc_mask:
            out.update(doc_mask=True, docs_per_row=round(self.docs_per_row(0), 4))
        if self.streamer is not None and self.streamer.gather_s > 0:
            out["gather_gb_per_s"] = round(self.streamer.gather_bytes / self.streamer.gather_s / 1e9, 3)
            out["restarts"] = self.streamer.restarts
            out["uploads_pending_at_request"] = [self.streamer.pending_copies, self.streamer.requests]
        return out

    def close(self):
        if self.streamer is not None:
            self.streamer.close()
            self.streamer = None
