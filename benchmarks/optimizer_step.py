"""Optimizer step time: the layer-wise optimizers (LARS / LAMB) against the fused ones they build on.

    A  FusedSGD / FusedAdam     one launch over the flat store
    B  FusedLARS / FusedLAMB    four launches: per-item sums, fold, ratio, update (csrc/kernels/layerwise.hip)

No model runs: the flat stores are laid out from the parameter slot lists of ``resnet50``, ``bert_base`` and
``llama_1b`` (the constructors only register slots) and filled with random weights and fp32 gradients. Both paths run
in one process on the same store, alternating A / B per sample; a sample is at least ``--min-sec`` of device time
measured with device events. One JSON line per sample, and a summary line per (store, family) with ms per step, GB/s
from the byte counts below, B / A and A's own sample-to-sample spread, goes to ``--out``.

Bytes per parameter, counted from the kernels' accesses with fp32 gradients (+2 for the bf16 copy of a low-precision
slot, counted for every slot here):

    SGD   read p, m, g; write p, m                                   20 + 2 = 22
    Adam  read p, m, v, g; write p, m, v                             28 + 2 = 30
    LARS  pass 1 read p, g; pass 2 read p, m, g; write p, m          28 + 2 = 30
    LAMB  pass 1 read p, m, v, g; write m, v; pass 2 read p, m, v;
          write p                                                    40 + 2 = 42

    python benchmarks/optimizer_step.py [--models resnet50 bert_base llama_1b] [--samples 3] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BYTES = {"sgd": 22, "adam": 30, "lars": 30, "lamb": 42}


def slot_list(name):
    """[(name, shape, decay, lowp)] of a model's parameters, from its constructor (nothing is allocated)."""
    from k8s_amd.parallel.flat import ParamStore

    store = ParamStore()
    if name == "resnet50":
        from k8s_amd.models.resnet import resnet50

        resnet50(store, 1000)
    elif name == "bert_base":
        from k8s_amd.models import bert

        bert.BertForPreTraining(store, bert.BERT_BASE)
    elif name == "llama_1b":
        from k8s_amd.models import llama

        llama.LlamaForCausalLM(store, llama.LLAMA_1B)
    else:
        raise ValueError("no slot list for %r" % name)
    return [(p.name, p.shape, p.decay, p.lowp) for p in store.params]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["resnet50", "bert_base", "llama_1b"])
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--min-sec", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_layerwise_ab.jsonl"))
    a = ap.parse_args(argv)

    import torch

    from k8s_amd.ops.optim import FusedAdam, FusedLAMB, FusedLARS, FusedSGD
    from k8s_amd.parallel.flat import ParamStore, init_const

    dev = torch.device("cuda", 0)

    def timed(opt, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            opt.step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters  # ms per step

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for model in a.models:
            slots = slot_list(model)
            store = ParamStore()
            for name, shape, decay, lowp in slots:
                store.new(name, shape, init_const(0.0), decay=decay, lowp=lowp)
            store.finalize(dev)
            n = store.num_parameters()
            for family in (("sgd", "lars"), ("adam", "lamb")):
                torch.manual_seed(0)
                store.master.normal_(0.0, 0.02)
                store.grad.normal_(0.0, 1e-3)
                store.refresh_lowp()
                # a learning rate that leaves the weights where they are over thousands of timed steps
                opts = {"sgd": lambda: FusedSGD(store, lr=1e-6, weight_decay=5e-5),
                        "adam": lambda: FusedAdam(store, lr=1e-7, weight_decay=0.01),
                        "lars": lambda: FusedLARS(store, lr=1e-6, weight_decay=5e-5),
                        "lamb": lambda: FusedLAMB(store, lr=1e-7, weight_decay=0.01)}
                paths = {"A": (family[0], opts[family[0]]()), "B": (family[1], opts[family[1]]())}
                iters = {}
                for key, (_, opt) in paths.items():  # first steps (momentum initialisation, item table), then size
                    opt.step()
                    opt.step()
                    torch.cuda.synchronize()
                    iters[key] = max(3, math.ceil(1.1 * a.min_sec * 1e3 / timed(opt, 3)))
                ms = {"A": [], "B": []}
                for s in range(a.samples):
                    for key, (kind, opt) in paths.items():
                        t = timed(opt, iters[key])
                        while t * iters[key] < a.min_sec * 1e3:  # a sample shorter than --min-sec is taken again
                            iters[key] = math.ceil(iters[key] * 1.2)
                            t = timed(opt, iters[key])
                        ms[key].append(t)
                        emit({"path": key, "optimizer": kind, "model": model, "slots": len(slots), "parameters": n,
                              "sample": s, "iters": iters[key], "ms_per_step": round(t, 5),
                              "gb_per_sec": round(BYTES[kind] * n / t / 1e6, 1)})
                mean = {k: sum(v) / len(v) for k, v in ms.items()}
                ka, kb = family
                emit({"summary": True, "model": model, "slots": len(slots), "parameters": n, "a": ka, "b": kb,
                      "a_ms": round(mean["A"], 5), "b_ms": round(mean["B"], 5),
                      "a_gb_per_sec": round(BYTES[ka] * n / mean["A"] / 1e6, 1),
                      "b_gb_per_sec": round(BYTES[kb] * n / mean["B"] / 1e6, 1),
                      "b_over_a": round(mean["B"] / mean["A"], 4), "byte_ratio": round(BYTES[kb] / BYTES[ka], 4),
                      "a_spread": round((max(ms["A"]) - min(ms["A"])) / mean["A"], 4),
                      "b_spread": round((max(ms["B"]) - min(ms["B"])) / mean["B"], 4),
                      "finite": bool(torch.isfinite(store.master).all())})
                del paths, opts
                torch.cuda.empty_cache()
            del store
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
