"""ResNet-50 forward-only (evaluation) throughput: the eval-mode forward against ``forward_infer``.

    A  model.eval() + torch.no_grad() + model(x)       every BatchNorm a separate eval-mode pass, convolutions on
                                                       their training kernels (statistics epilogue included)
    B  model.forward_infer(x, folded)                  BatchNorm folded into the tile kernel's inference epilogue

Both run in one process, alternating A / B per sample, after warming every shape; a sample is at least ``--min-sec``
of device time measured with device events. One JSON line per sample (and one summary line per batch size: B / A and
A's own sample-to-sample spread) goes to ``--out``.

    python benchmarks/eval_throughput.py [--batches 256 1024] [--image 224] [--samples 3] [--out FILE]
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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--min-sec", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_forward_ab.jsonl"))
    a = ap.parse_args(argv)

    import torch

    from k8s_amd.models.resnet import resnet50
    from k8s_amd.ops import conv
    from k8s_amd.parallel.flat import ParamStore

    dev = torch.device("cuda", 0)
    store = ParamStore()
    model = resnet50(store).finalize(dev)
    # a trained model's BatchNorms: bn3's gamma is zero-initialised, running statistics start at (0, 1)
    g = torch.Generator(device="cpu").manual_seed(0)
    with torch.no_grad():
        for bn in model.batch_norms():
            c = bn.running_mean.numel()
            bn.gamma.master.copy_((torch.rand(c, generator=g) * 0.5 + 0.75).to(dev))
            bn.running_mean.copy_((torch.randn(c, generator=g) * 0.1).to(dev))
            bn.running_var.copy_((torch.rand(c, generator=g) + 0.5).to(dev))
    store.refresh_lowp()
    folded = model.fold_bn()

    def path_a(x):
        model.eval()
        with torch.no_grad():
            y = model(x)
        model.train()
        return y

    def path_b(x):
        return model.forward_infer(x, folded)

    paths = {"A": path_a, "B": path_b}

    def timed(fn, x, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn(x)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters  # ms per forward

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for batch in a.batches:
            torch.manual_seed(batch)
            x = model.prepare_input(torch.randn(batch, a.image, a.image, 3, device=dev).bfloat16()).contiguous()
            iters, stats = {}, {}
            for name, fn in paths.items():  # warm every shape, count the kernels each path runs, size a sample
                fn(x)
                before = dict(conv.STATS)
                fn(x)
                stats[name] = {k: conv.STATS[k] - before[k] for k in conv.STATS if conv.STATS[k] != before[k]}
                torch.cuda.synchronize()
                iters[name] = max(3, math.ceil(1.1 * a.min_sec * 1e3 / timed(fn, x, 3)))
                print("batch %d path %s conv.STATS per forward: %s" % (batch, name, json.dumps(stats[name])),
                      file=sys.stderr, flush=True)
            ms = {"A": [], "B": []}
            for s in range(a.samples):
                for name, fn in paths.items():
                    t = timed(fn, x, iters[name])
                    while t * iters[name] < a.min_sec * 1e3:  # a sample shorter than --min-sec is taken again, longer
                        iters[name] = math.ceil(iters[name] * 1.2)
                        t = timed(fn, x, iters[name])
                    ms[name].append(t)
                    emit({"path": name, "batch": batch, "image": a.image, "sample": s, "iters": iters[name],
                          "ms_per_forward": round(t, 4), "images_per_sec": round(batch / t * 1e3, 1),
                          "conv_stats": stats[name]})
            mean = {k: sum(v) / len(v) for k, v in ms.items()}
            emit({"summary": True, "batch": batch, "image": a.image,
                  "a_images_per_sec": round(batch / mean["A"] * 1e3, 1),
                  "b_images_per_sec": round(batch / mean["B"] * 1e3, 1),
                  "b_over_a": round(mean["A"] / mean["B"], 4),
                  "a_spread": round((max(ms["A"]) - min(ms["A"])) / mean["A"], 4),
                  "b_spread": round((max(ms["B"]) - min(ms["B"])) / mean["B"], 4)})
            del x
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
