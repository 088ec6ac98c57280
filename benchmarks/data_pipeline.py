"""The dataset path measured: the fused augmentation kernel against the torch composition it replaces, and the trainer
on a dataset against the trainer on its synthetic fixed batch.

Kernel alone (default). Per shape, A and B alternate in one process, timed with device events, ``--samples`` samples of
at least ``--min-seconds`` each:

    A torch   index gather of the crop (flip folded into the column index), float, normalise (bilinear weights for a
              resized row: four gathers and three lerps), zero outside the source, bf16, pad to 8 channels,
              ``stem_s2d_input``
    B augment ``ops.data.augment(..., layout="s2d")`` -- table validation and upload included, as the loader calls it

One JSON line per sample; one summary line per shape with the medians, B / A, A's spread, and B's GB/s over the bytes
it must move (the bytes of every row's box inside the source, plus the output), also as a fraction of the project's
6.25 TB/s read-1-write-1 streaming figure. The gather is not a stream: that fraction is reported, not a bar. A and B
are compared once per shape before they are timed (within one bf16 step of each other).

``--e2e``: ``python -m k8s_amd.trainer --model resnet50 --batch 1024`` in three configurations alternating,
``--runs`` runs each: A the synthetic fixed batch, B1 a resident toy set (256 x 256, ``--e2e-images`` images,
``--augment rrc``), B2 the same set streamed (``--data-resident-gb 0``). Images/s is the median of each run's logged
windows after the first; B2 also reports the loader thread's gather rate, timed on the host.

    python benchmarks/data_pipeline.py [--samples 3] [--e2e] [--out profiles/data_pipeline_ab.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STREAM_CEILING_GBS = 6250.0  # profiles/r02_stream_bw_patterns_v2.jsonl, read 1 : write 1
# (name, N, source side, M resident sources, S, augment)
SHAPES = [("b3072.rrc", 3072, 256, 4096, 224, "rrc"), ("b3072.crop", 3072, 256, 4096, 224, "crop"),
          ("b1024.rrc", 1024, 256, 4096, 224, "rrc"), ("b1024.crop", 1024, 256, 4096, 224, "crop"),
          ("b3072.cifar", 3072, 32, 50000, 32, "crop")]


def torch_composition(src, tab, a, b, S):
    """What the kernel replaces, from torch ops on the device. ``tab``: the int32 table on the host."""
    import torch

    from k8s_amd.ops import nn as K

    dev = src.device
    Hs, Ws = src.shape[1:3]
    t = tab.to(dev).long()
    idx, y0, x0, h, w, flip = (t[:, k] for k in range(6))
    ar = torch.arange(S, device=dev)
    jj = torch.where(flip[:, None] > 0, S - 1 - ar[None], ar[None])  # [N, S]
    av = torch.tensor(a, device=dev, dtype=torch.float32)
    bv = torch.tensor(b, device=dev, dtype=torch.float32)
    n = idx[:, None, None]
    if bool(((h == S) & (w == S)).all()):
        ys, xs = y0[:, None] + ar[None], x0[:, None] + jj
        inside = ((ys >= 0) & (ys < Hs))[:, :, None] & ((xs >= 0) & (xs < Ws))[:, None, :]
        g = src[n, ys.clamp(0, Hs - 1)[:, :, None], xs.clamp(0, Ws - 1)[:, None, :]]  # [N, S, S, 3] uint8
        v = (g.float() * av + bv) * inside[..., None]
    else:
        fy = ((ar[None].float() + 0.5) * (h[:, None].float() / S) - 0.5).clamp(min=0)
        fx = ((jj.float() + 0.5) * (w[:, None].float() / S) - 0.5).clamp(min=0)
        iy0 = torch.minimum(fy.long(), h[:, None] - 1)
        ix0 = torch.minimum(fx.long(), w[:, None] - 1)
        iy1, ix1 = torch.minimum(iy0 + 1, h[:, None] - 1), torch.minimum(ix0 + 1, w[:, None] - 1)
        ly, lx = (fy - iy0)[:, :, None, None], (fx - ix0)[:, None, :, None]
        ya, yb = (y0[:, None] + iy0)[:, :, None], (y0[:, None] + iy1)[:, :, None]
        xa, xb = (x0[:, None] + ix0)[:, None, :], (x0[:, None] + ix1)[:, None, :]
        top = torch.lerp(src[n, ya, xa].float(), src[n, ya, xb].float(), lx)
        bot = torch.lerp(src[n, yb, xa].float(), src[n, yb, xb].float(), lx)
        v = torch.lerp(top, bot, ly) * av + bv
    x8 = torch.nn.functional.pad(v.to(torch.bfloat16), (0, 5))
    return K.stem_s2d_input(x8, 3)


def needed_bytes(tab, Hs, Ws, S):
    """Bytes B must move: every row's box inside the source, read once, plus the s2d output."""
    import numpy as np

    t = tab.numpy().astype(np.int64)
    hh = np.minimum(t[:, 1] + t[:, 3], Hs) - np.maximum(t[:, 1], 0)
    ww = np.minimum(t[:, 2] + t[:, 4], Ws) - np.maximum(t[:, 2], 0)
    read = int((np.maximum(hh, 0) * np.maximum(ww, 0) * 3).sum())
    return read, len(t) * (S // 2 + 3) ** 2 * 32


def kernels(a, emit):
    import torch

    from k8s_amd.data import sampler
    from k8s_amd.ops import data as kdata
    from k8s_amd.ops._ext import load

    load()
    dev = torch.device("cuda", 0)
    na, nb = kdata.norm_constants([125.3, 123.0, 113.9], [63.0, 62.1, 66.7])

    def sample(fn):
        """ms per call over at least --min-seconds of back-to-back calls, by device events."""
        iters, total = 1, 0.0
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            total = e0.elapsed_time(e1)
            if total >= a.min_seconds * 1e3:
                return total / iters
            iters = max(iters + 1, int(iters * a.min_seconds * 1.2e3 / max(total, 1e-3)))

    src, last = None, None
    for name, N, side, M, S, aug in SHAPES:
        if a.only and name not in a.only:
            continue
        if last != (side, M):
            del src
            torch.cuda.empty_cache()
            src = torch.randint(0, 256, (M, side, side, 3), device=dev, dtype=torch.uint8)
            last = (side, M)
        idx = sampler.batch_indices(0, 1, 0, 1, N, M)
        tab = torch.from_numpy(sampler.train_table(idx, 0, 1, 0, side, side, S, aug, 4))
        paths = {"torch": lambda: torch_composition(src, tab, na, nb, S),
                 "augment": lambda: kdata.augment(src, tab, na, nb, S, "s2d")}
        xa, xb = paths["torch"](), paths["augment"]()
        # the same batch both ways, up to fp32 rounding before the bf16 one: one bf16 step of the larger value (2^-7
        # relative), plus what one fp32 step of a source coordinate near 256 (1.5e-5; B contracts its multiply-add, A
        # does not) moves a bilinear sample of uniform noise -- up to 255 * 1.5e-5 per axis, / std: about 1e-4 each
        fa, fb = xa.float(), xb.float()
        off = ((fa - fb).abs() - torch.maximum(fa.abs(), fb.abs()) * 2.0 ** -7).max().item()
        if off > 1e-3:
            raise RuntimeError("%s: the torch composition and the kernel disagree by %g" % (name, off))
        worst = (fa - fb).abs().max().item()
        del xa, xb, fa, fb
        read, written = needed_bytes(tab, side, side, S)
        ms = {k: [] for k in paths}
        for s in range(a.samples):
            for key, fn in paths.items():
                t = sample(fn)
                ms[key].append(t)
                emit({"kernel": True, "shape": name, "path": key, "sample": s, "ms": round(t, 4)})
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        gbs = (read + written) / med["augment"] / 1e6
        emit({"summary": True, "shape": name, "N": N, "source": side, "S": S, "augment": aug,
              "torch_ms": round(med["torch"], 4), "augment_ms": round(med["augment"], 4),
              "torch_spread_ms": round(spread["torch"], 4), "augment_spread_ms": round(spread["augment"], 4),
              "augment_over_torch": round(med["augment"] / med["torch"], 4),
              "beats_torch_by_more_than_its_spread": bool(med["torch"] - med["augment"] > spread["torch"]),
              "max_abs_difference": worst, "read_gb": round(read / 1e9, 4),
              "written_gb": round(written / 1e9, 4), "augment_gb_per_sec": round(gbs, 1),
              "share_of_stream_ceiling": round(gbs / STREAM_CEILING_GBS, 4)})


def trainer_run(extra, steps, log_every):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "k8s_amd.trainer", "--model", "resnet50", "--batch", "1024", "--steps", str(steps),
           "--log-every", str(log_every)] + extra
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("trainer failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    ev = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    rates = [e["images_per_sec"] for e in ev if e.get("event") == "step"][1:]  # the first window holds the warm-up
    done = [e for e in ev if e.get("event") == "done"][-1]
    return statistics.median(rates), done.get("data")


def e2e(a, emit):
    from k8s_amd.tools.make_dataset import make_toy

    with tempfile.TemporaryDirectory() as d:
        make_toy(d, train=a.e2e_images, val=16, size=256)
        data = ["--data-dir", d, "--augment", "rrc"]
        configs = {"A.synthetic": [], "B1.resident": data, "B2.streamed": data + ["--data-resident-gb", "0"]}
        rates = {k: [] for k in configs}
        for run in range(a.runs):
            for key, extra in configs.items():
                rate, info = trainer_run(extra, a.e2e_steps, a.e2e_log_every)
                rates[key].append(rate)
                emit({"e2e": True, "config": key, "run": run, "images_per_sec": rate, "data": info})
        emit({"e2e_summary": True, "images": a.e2e_images,
              **{k: {"images_per_sec": round(statistics.median(v), 1), "spread": round(max(v) - min(v), 1)}
                 for k, v in rates.items()}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--only", nargs="*", default=None, help="shape names")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--e2e-images", type=int, default=4096)
    ap.add_argument("--e2e-steps", type=int, default=60)
    ap.add_argument("--e2e-log-every", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_pipeline_ab.jsonl"))
    a = ap.parse_args(argv)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    if not a.no_kernels:
        kernels(a, emit)
    if a.e2e:
        e2e(a, emit)
    f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
