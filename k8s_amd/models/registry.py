"""Model registry: name -> (model on a flat ParamStore, synthetic batch, loss).

Every workload the trainer (``python -m k8s_amd.trainer``) and the benches
can run, at the exact BASELINE.json shapes plus small variants for CPU tests.
Data is synthetic by default (random images / token ids of the named shape): the
reference's workloads are external TF programs. Every workload can also read a
dataset directory (``build(..., data=...)``, ``k8s_amd.data``): batches then
come from its ``train`` split through a fused batch kernel (augmentation for
the ResNet models and an image directory; MLM or causal batch assembly for the
BERT and Llama models and a token directory) and held-out batches from its
``val`` split.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

import torch

from k8s_amd.ops import nn as K
from k8s_amd.parallel.flat import ParamStore


@dataclass
class Workload:
    name: str
    model: torch.nn.Module
    store: ParamStore
    batch: Callable[[int], Tuple]          # step -> inputs tuple (on device)
    loss: Callable[[Tuple], torch.Tensor]  # inputs -> scalar loss
    units_per_step: int                    # images or tokens per step per rank
    unit: str                              # "images" | "tokens"
    optimizer: str = "sgd"                 # default optimizer family
    lr: float = 0.1
    meta: Dict = field(default_factory=dict)
    # ---- evaluation (no autograd, nothing written to parameters, statistics or gradient slots)
    # evaluate(inputs, folded=None) -> sums as device tensors: {"loss_sum" fp64, "count" int64} (+ {"top1", "top5"}
    # int64 for ResNet); ``folded``: eval_state()'s tensor, computed here when None
    evaluate: Optional[Callable] = None
    # eval_batch(i, batch=None) -> held-out batch i (its own generator seed: identical every time it is requested)
    eval_batch: Optional[Callable] = None
    # eval_state() -> the flat tensor an evaluation pass shares between ranks (ResNet: the folded BatchNorms), or None
    eval_state: Optional[Callable] = None
    # close() releases what the batches hold (a dataset loader's background thread); None: nothing to release
    close: Optional[Callable] = None


MODELS = ("resnet50", "resnet_tiny", "bert_base", "bert_tiny", "llama3_8b", "llama_1b", "llama_tiny")
# each model's default optimizer family (Workload.optimizer), known before the model is built
MODEL_OPTIMIZER = {"resnet50": "sgd", "resnet_tiny": "sgd", "bert_base": "adam", "bert_tiny": "adam",
                   "llama3_8b": "adam", "llama_1b": "adam", "llama_tiny": "adam"}


# ResNet evaluation path: ``ResNet.forward_infer`` (BatchNorms folded into the convolutions' epilogue) or, False, the
# model's eval-mode forward (separate BatchNorm passes). Set from benchmarks/eval_throughput.py's A/B.
EVAL_FOLDED = True


def _plain_eval_forward(model, x):
    """Logits of the model's own forward in eval mode, its training flag restored afterwards."""
    was = model.training
    model.eval()
    try:
        return model(x)
    finally:
        model.train(was)


def _resnet_evaluate(model):
    """``Workload.evaluate`` of a ResNet: the sums of one batch (rows labelled -100 are not counted)."""
    def evaluate(b, folded=None):
        with torch.no_grad():
            logits = model.forward_infer(b[0], folded) if EVAL_FOLDED else _plain_eval_forward(model, b[0])
            loss, rank = K.xent_eval(logits, b[1])
            return {"loss_sum": loss.double().sum(), "count": (b[1] != -100).sum(),
                    "top1": (rank < 1).sum(), "top5": (rank < 5).sum()}

    return evaluate


def dataset_plan(name: str, device, batch: int, image: Optional[int], data: Dict, need_val: bool = False):
    """(dataset, Loader keyword arguments, description) of ``build(name, ..., data=data)``, with every check of the
    configuration made (``DataError``): what the trainer's ``start`` event reports before the model is built."""
    from k8s_amd.data import dataset_kind, open_dataset, sampler
    from k8s_amd.data.loader import is_resident

    check_data_kind(name, dataset_kind(data["dir"]))
    ds = open_dataset(data["dir"], need=("train", "val") if need_val else ("train",))
    kw = dict(image=image, augment=data.get("augment", "crop"), crop_pad=data.get("crop_pad", 4),
              seed=data.get("seed", 0), rank=data.get("rank", 0), world=data.get("world", 1),
              resident_gb=data.get("resident_gb", 4.0))
    tr = ds.split("train")
    Hs, Ws = (int(v) for v in tr.images.shape[1:3])
    if not image:  # crop / none: the source size; a resize has no natural size, so the model's preset
        kw["image"] = (224 if name == "resnet50" else 32) if kw["augment"] == "rrc" else min(Hs, Ws)
    sampler.check_geometry(kw["augment"], Hs, Ws, kw["image"], kw["crop_pad"])
    info = {"dir": data["dir"], "train": int(tr.images.shape[0]),
            "val": int(ds.splits["val"].images.shape[0]) if "val" in ds.splits else 0, "source": [Hs, Ws],
            "image": kw["image"], "augment": kw["augment"],
            "resident": is_resident(tr.nbytes, kw["resident_gb"], torch.device(device)),
            "steps_per_epoch": sampler.steps_per_epoch(int(tr.images.shape[0]), batch, kw["world"])}
    return ds, kw, info


def check_data_kind(name: str, kind: str) -> None:
    """An image directory feeds the ResNet models and a token directory the BERT and Llama models, nothing else."""
    if name not in MODELS:
        raise ValueError("unknown model %r (choose from %s)" % (name, ", ".join(MODELS)))
    images = name in ("resnet50", "resnet_tiny")
    if kind == "images" and not images:
        raise ValueError("an image dataset directory can be read by the ResNet models only, not %r" % name)
    if kind == "tokens" and images:
        raise ValueError("a token dataset directory can be read by the BERT and Llama models only, not %r" % name)


def token_config(name: str):
    if name in ("bert_base", "bert_tiny"):
        from k8s_amd.models import bert as M

        return M.BERT_BASE if name == "bert_base" else M.BERT_TINY
    from k8s_amd.models import llama as M

    return {"llama3_8b": M.LLAMA3_8B, "llama_1b": M.LLAMA_1B, "llama_tiny": M.LLAMA_TINY}[name]


def default_seq(name: str) -> int:
    return {"bert_base": 128, "bert_tiny": 32, "llama_tiny": 64}.get(name, 4096)


def token_dataset_plan(name: str, device, batch: int, seq: Optional[int], data: Dict, need_val: bool = False,
                       mlm_every_token: bool = False):
    """``dataset_plan`` for the BERT and Llama models and a token directory: (dataset, TokenLoader keyword arguments,
    description), with every check of the configuration made (``DataError``)."""
    from k8s_amd.data import DataError, dataset_kind, open_token_dataset
    from k8s_amd.data import token_sampler as ts
    from k8s_amd.data.loader import is_resident
    from k8s_amd.ops.reference import MLM_MAX_SEQ

    check_data_kind(name, dataset_kind(data["dir"]))
    bert = name.startswith("bert")
    cfg = token_config(name)
    seq = int(seq or default_seq(name))
    if seq > cfg.max_position or (bert and seq > MLM_MAX_SEQ):
        raise DataError("--seq %d exceeds %s" % (seq, "the model's max_position = %d" % cfg.max_position
                                                 if seq > cfg.max_position else
                                                 "the %d positions the MLM batch kernel assembles" % MLM_MAX_SEQ))
    if bert and mlm_every_token:
        raise DataError("a token dataset yields the masked-position format: not with --mlm-head every-token")
    ds = open_token_dataset(data["dir"], need=("train", "val") if need_val else ("train",), pairs=bert)
    if ds.vocab > cfg.vocab_size:
        raise DataError("dataset %s: vocab = %d exceeds %s's vocab_size = %d" % (ds.path, ds.vocab, name,
                                                                                cfg.vocab_size))
    kw = dict(seq=seq, kind="bert" if bert else "llama", max_predictions=cfg.max_predictions if bert else 1,
              seed=data.get("seed", 0), rank=data.get("rank", 0), world=data.get("world", 1),
              resident_gb=data.get("resident_gb", 4.0))
    tr = ds.split("train")
    doc_mask = bool(data.get("doc_mask"))
    if doc_mask:
        if bert:
            raise DataError("document-boundary masks are implemented for the Llama models only, not %s" % name)
        for sp_name in ("train", "val") if need_val else ("train",):
            sp = ds.split(sp_name)
            if sp.segments is None or sp.docs is None:
                raise DataError("dataset %s: --doc-mask needs %s_segments.npy and %s_docs.npy"
                                % (ds.path, sp_name, sp_name))
        kw["doc_mask"] = True
    unpad = bool(data.get("unpad"))
    if unpad:
        if not bert or doc_mask:
            raise DataError("unpadded batches are implemented for the BERT models only, not %s%s"
                            % (name, " with a document mask" if doc_mask else ""))
        kw["unpad"] = True
    if bert:
        ts.check_seq(seq, kw["max_predictions"])
        items, what = tr.G, "segments"
    else:
        items, what = ts.windows(tr.T, seq), "windows of %d tokens" % seq
    E = ts.steps_per_epoch(items, batch, kw["world"], what)
    pad_fraction = 0.0
    if bert:  # the first epoch's first batch, from the host table alone
        idx, ords = ts.train_items(kw["seed"], 0, kw["rank"], kw["world"], batch, items)
        lens = ts.pair_rows(tr.segments, tr.docs, idx, ords, kw["seed"], seq, kw["max_predictions"])[2]
        pad_fraction = round(float(1.0 - lens.mean() / seq), 4)
        stream_rows = (int(lens.sum()) + 127) // 128 * 128  # (unpad) the rows of that batch's token stream
    size = lambda sp: {"tokens": sp.T, "segments": sp.G, "documents": sp.D}  # noqa: E731
    info = {"dir": data["dir"], "kind": "tokens", "vocab": ds.vocab, "train": size(tr),
            "val": size(ds.splits["val"]) if "val" in ds.splits else None, "seq": seq,
            "resident": is_resident(tr.nbytes, kw["resident_gb"], torch.device(device)), "steps_per_epoch": E,
            "pad_fraction": pad_fraction}
    if unpad:
        info.update(unpad=True, stream_rows=stream_rows)
    if doc_mask:  # the documents per row of the first batch, from the host tables alone
        import numpy as np

        idx = ts.train_items(kw["seed"], 0, kw["rank"], kw["world"], batch, items)[0]
        doc_tok = tr.segments[tr.docs]
        first = np.searchsorted(doc_tok, idx * seq, side="right")
        last = np.searchsorted(doc_tok, idx * seq + seq - 1, side="right")
        info.update(doc_mask=True, docs_per_row=round(float((last - first + 1).mean()), 4))
    return ds, kw, info


def _token_loaders(name, device, batch, seq, seed, data, mlm_every_token):
    """(training TokenLoader, eval_batch, close, description) of a token model on a dataset directory."""
    from k8s_amd.data.token_loader import TokenLoader

    ds, kw, info = token_dataset_plan(name, device, batch, seq, dict(data, seed=data.get("seed", seed)),
                                      mlm_every_token=mlm_every_token)
    train = TokenLoader(ds, "train", device, batch, train=True, **kw)
    evals = {}

    def eval_batch(i, batch_=None):
        n = batch_ or batch
        if n not in evals:
            evals[n] = TokenLoader(ds, "val", device, n, train=False, **kw)
        return evals[n].batch(i)

    def close():
        for ld in [train] + list(evals.values()):
            ld.close()

    return train, eval_batch, close, info


def _resnet_on_dataset(name, store, device, batch, image, seed, grad_dtype, pad_to, data) -> Workload:
    """A ResNet workload whose batches come from a dataset directory (see ``build``)."""
    from k8s_amd.data.loader import Loader
    from k8s_amd.models.resnet import resnet50, resnet_tiny

    ds, kw, info = dataset_plan(name, device, batch, image, dict(data, seed=data.get("seed", seed)))
    train = Loader(ds, "train", device, batch, train=True, **kw)  # raises DataError before the model is built
    model = (resnet50 if name == "resnet50" else resnet_tiny)(store, ds.classes)
    model = model.finalize(device, grad_dtype=grad_dtype, seed=seed, pad_to=pad_to)
    evals = {}

    def eval_batch(i, batch_=None):
        n = batch_ or batch
        if n not in evals:
            evals[n] = Loader(ds, "val", device, n, train=False, **dict(kw, image=train.S))
        return evals[n].batch(i)

    def close():
        for ld in [train] + list(evals.values()):
            ld.close()

    return Workload(name, model, store, train.batch, lambda b: K.cross_entropy(model(b[0]), b[1]), batch, "images",
                    "sgd", 0.1, {"image": train.S, "classes": ds.classes, "data": info, "loader": train},
                    evaluate=_resnet_evaluate(model), eval_batch=eval_batch, eval_state=lambda: model.fold_bn()[0], close=close)


def build(name: str, device, batch: int, seq: Optional[int] = None, image: Optional[int] = None,
          seed: int = 0, grad_dtype=torch.float32, fixed_batch: bool = True, pad_to: int = 64,
          data_seed: Optional[int] = None, mlm_every_token: bool = False, dropout: Optional[float] = None,
          dropout_seed: Optional[int] = None, data: Optional[Dict] = None) -> Workload:
    """Construct ``name`` on ``device`` with per-rank ``batch``. ``fixed_batch`` reuses one synthetic batch
    (what a throughput benchmark wants); otherwise every step draws a new one. ``dropout`` (BERT only): the hidden
    and attention-probability dropout of the training forward, seeded by ``dropout_seed`` (default ``seed``);
    evaluation runs without it. ``data``: train on a dataset directory instead of synthetic batches --
    ``{"dir", "augment", "crop_pad", "resident_gb", "seed", "rank", "world"}`` (``k8s_amd.data.loader.Loader``'s
    arguments, or without the two augmentation keys ``TokenLoader``'s; only ``dir`` is required). The directory's
    With ``"unpad": True`` (BERT, no dropout) batches are unpadded token streams and the loss is
    ``forward_unpadded``'s. The directory's
    kind must fit the model: images for ResNet (``classes`` then comes from its meta.json), tokens for BERT and Llama.
    ``batch(t)`` is batch ``t`` of the ``train`` split and ``eval_batch(i)`` batch ``i`` of the ``val`` split."""
    if data is not None:
        from k8s_amd.data import dataset_kind

        check_data_kind(name, dataset_kind(data["dir"]))
    if dropout and name not in ("bert_base", "bert_tiny"):
        raise ValueError("dropout is implemented for the BERT models only, not %r" % name)
    if data is not None and data.get("unpad") and dropout:
        raise ValueError("unpadded batches cannot be combined with dropout (the span kernels have no dropout form)")
    device = torch.device(device)
    dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
    store = ParamStore()
    gen = torch.Generator(device=device)
    gen.manual_seed(1000 + (seed if data_seed is None else data_seed))
    # held-out data: a generator of its own, re-seeded per requested batch, so batch i never depends on what was
    # drawn before it and never overlaps the training stream's seed
    eval_gen = torch.Generator(device=device)
    eval_seed = 1000 + (seed if data_seed is None else data_seed) + 2 ** 20

    def heldout(make_with):
        def get(i, batch_=None):
            eval_gen.manual_seed(eval_seed + int(i))
            return make_with(batch_ or batch, eval_gen)

        return get

    def token_eval(loss_of, labels_of, model=None):
        """Evaluation of a token model: its own forward under no_grad -- in eval mode when ``model`` is given (BERT:
        no dropout), the training flag restored afterwards as ``_plain_eval_forward`` does."""
        def evaluate(b, folded=None):
            was = model.training if model is not None else None
            if model is not None:
                model.eval()
            try:
                with torch.no_grad():
                    count = (labels_of(b) != -100).sum()
                    # a batch without a labelled row (past the end of a held-out split) adds exactly nothing,
                    # whatever its mean over no rows is
                    total = loss_of(b).double() * count.double()
                    return {"loss_sum": torch.where(count > 0, total, torch.zeros_like(total)), "count": count}
            finally:
                if model is not None:
                    model.train(was)

        return evaluate

    def cached(make):
        box = {}

        def get(step):
            if fixed_batch:
                if "b" not in box:
                    box["b"] = make()
                return box["b"]
            # fresh batches are consecutive draws of one generator, so batch i is the (i + 1)-th draw: a run resumed
            # at batch i first discards the draws an uninterrupted run made before it and then sees the same data
            done = box.get("next", 0)
            for _ in range(done, int(step)):
                make()
            box["next"] = max(done, int(step)) + 1
            return make()

        return get

    if name in ("resnet50", "resnet_tiny"):
        from k8s_amd.models.resnet import resnet50, resnet_tiny

        ncls = 1000 if name == "resnet50" else 10
        if data is not None:
            return _resnet_on_dataset(name, store, device, batch, image, seed, grad_dtype, pad_to, data)
        image = image or (224 if name == "resnet50" else 32)
        model = (resnet50(store, ncls) if name == "resnet50" else resnet_tiny(store, ncls))
        model = model.finalize(device, grad_dtype=grad_dtype, seed=seed, pad_to=pad_to)

        def make(n=batch, g=gen):
            x = torch.randn(n, image, image, 3, device=device, generator=g).to(dtype)
            return model.prepare_input(x).contiguous(), torch.randint(0, ncls, (n,), device=device, generator=g)

        return Workload(name, model, store, cached(make), lambda b: K.cross_entropy(model(b[0]), b[1]), batch,
                        "images", "sgd", 0.1, {"image": image, "classes": ncls}, evaluate=_resnet_evaluate(model),
                        eval_batch=heldout(make), eval_state=lambda: model.fold_bn()[0])

    if name in ("bert_base", "bert_tiny"):
        from k8s_amd.models import bert as M

        import dataclasses

        cfg = M.BERT_BASE if name == "bert_base" else M.BERT_TINY
        if mlm_every_token:  # the MLM head on every token (dense labels), like HF BertForPreTraining
            cfg = dataclasses.replace(cfg, max_predictions=0)
        if dropout:
            cfg = dataclasses.replace(cfg, hidden_dropout=float(dropout), attention_dropout=float(dropout))
        seq = seq or default_seq(name)
        if data is not None:  # raises DataError before the model is built
            train, eval_batch, close, info = _token_loaders(name, device, batch, seq, seed, data, mlm_every_token)
        model = M.BertForPreTraining(store, cfg).finalize(device, grad_dtype=grad_dtype, seed=seed, pad_to=pad_to)
        model.drop_state = K.DropoutState(seed if dropout_seed is None else dropout_seed, device)
        if data is not None and data.get("unpad"):  # batches in forward_unpadded's positional order
            return Workload(name, model, store, train.batch, lambda b: model.forward_unpadded(*b, dtype=dtype)[0],
                            batch * seq, "tokens", "adam", 1e-4, {"seq": seq, "data": info, "loader": train},
                            evaluate=token_eval(lambda b: model.forward_unpadded(*b, dtype=dtype)[0], lambda b: b[3],
                                                model),
                            eval_batch=eval_batch, close=close)
        if data is not None:  # batches are (ids, types, labels, nsp, positions, kv_lens): forward's positional order
            return Workload(name, model, store, train.batch, lambda b: model(*b, dtype=dtype)[0], batch * seq,
                            "tokens", "adam", 1e-4, {"seq": seq, "data": info, "loader": train},
                            evaluate=token_eval(lambda b: model(*b, dtype=dtype)[0], lambda b: b[2], model),
                            eval_batch=eval_batch, close=close)

        def make(n=batch, g=gen):
            return M.synthetic_batch(cfg, n, seq, device, generator=g)

        return Workload(name, model, store, cached(make), lambda b: model(*b, dtype=dtype)[0], batch * seq,
                        "tokens", "adam", 1e-4, {"seq": seq},
                        evaluate=token_eval(lambda b: model(*b, dtype=dtype)[0], lambda b: b[2], model),
                        eval_batch=heldout(make))

    if name in ("llama3_8b", "llama_1b", "llama_tiny"):
        from k8s_amd.models import llama as M

        cfg = {"llama3_8b": M.LLAMA3_8B, "llama_1b": M.LLAMA_1B, "llama_tiny": M.LLAMA_TINY}[name]
        seq = seq or default_seq(name)
        if data is not None:
            train, eval_batch, close, info = _token_loaders(name, device, batch, seq, seed, data, False)
        model = M.LlamaForCausalLM(store, cfg).finalize(device, grad_dtype=grad_dtype, seed=seed, pad_to=pad_to)
        if data is not None:
            return Workload(name, model, store, train.batch, lambda b: model(*b, dtype=dtype), batch * seq, "tokens",
                            "adam", 3e-4, {"seq": seq, "data": info, "loader": train},
                            evaluate=token_eval(lambda b: model(*b, dtype=dtype), lambda b: b[1]),
                            eval_batch=eval_batch, close=close)

        def make(n=batch, g=gen):
            return M.synthetic_batch(cfg, n, seq, device, generator=g)

        return Workload(name, model, store, cached(make), lambda b: model(*b, dtype=dtype), batch * seq, "tokens",
                        "adam", 3e-4, {"seq": seq},
                        evaluate=token_eval(lambda b: model(*b, dtype=dtype), lambda b: b[1]),
                        eval_batch=heldout(make))

    raise ValueError("unknown model %r (choose from %s)" % (name, ", ".join(MODELS)))
