"""Gradient accumulation: the two streaming kernels on real store sizes, and the trainer end to end.

No model runs in the kernel part: the flat stores are laid out from the parameter slot lists of ``resnet50``,
``bert_base`` and ``llama_1b`` (``benchmarks/optimizer_step.py``'s ``slot_list``) and filled with random fp32
gradients. Per store, in one process, alternating per sample (a sample is at least ``--min-sec`` of device time between
device events):

    accumulate_first   acc = g                       read g, write acc                       8 B / element
    accumulate         acc = acc + g                 read acc, g; write acc                 12 B / element
    fold               g = g + acc                   read g, acc; write g                   12 B / element
    A fold_bf16_torch  g.add_(acc); cast_bf16(g)     12 + read g, write bf16 = 18 B moved   (GB/s on the 14 B below)
    B fold_bf16        g = g + acc, out = bf16(g)    read g, acc; write g, bf16             14 B / element

One JSON line per sample and a summary line per (store, path) with ms, GB/s, the share of the project's read-1-write-1
streaming ceiling (``profiles/r02_stream_bw_patterns_v2.jsonl``: 6.25 TB/s) and, where
``profiles/optimizer_layerwise_ab.jsonl`` has the store, the ratio to ``fused_sgd``'s GB/s on it, go to ``--out``.

``--e2e`` adds the trainer pair: ``python -m k8s_amd.trainer --model bert_base --batch 1024 --seq 128`` at
``--accum-steps 1`` and ``--accum-steps 4``, alternating, ``--e2e-runs`` each, tokens/s from the logged steps after
the first window.

    python benchmarks/accum_step.py [--models resnet50 bert_base llama_1b] [--samples 3] [--e2e] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from benchmarks.optimizer_step import slot_list  # noqa: E402

BYTES = {"accumulate_first": 8, "accumulate": 12, "fold": 12, "fold_bf16_torch": 14, "fold_bf16": 14}
STREAM_CEILING_GBS = 6250.0  # read-1-write-1, profiles/r02_stream_bw_patterns_v2.jsonl


def sgd_gbs():
    """{model: fused_sgd GB/s} from the optimizer benchmark's summary lines, where that profile exists."""
    out = {}
    path = os.path.join(ROOT, "profiles", "optimizer_layerwise_ab.jsonl")
    if os.path.exists(path):
        for line in open(path):
            r = json.loads(line)
            if r.get("summary") and r.get("a") == "sgd":
                out[r["model"]] = r["a_gb_per_sec"]
    return out


def e2e_run(accum, steps, log_every):
    """tokens/s of one trainer run: the mean of the logged windows after the first."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("TF_CONFIG", "RANK", "WORLD_SIZE"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "k8s_amd.trainer", "--model", "bert_base", "--batch", "1024", "--seq", "128",
           "--accum-steps", str(accum), "--steps", str(steps), "--log-every", str(log_every)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("trainer failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    ev = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    rates = [e["tokens_per_sec"] for e in ev if e.get("event") == "step"][1:]
    done = [e for e in ev if e.get("event") == "done"][0]
    return sum(rates) / len(rates), done.get("peak_mem_gb")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="*", default=["resnet50", "bert_base", "llama_1b"],
                    help="stores of the kernel part (none: only --e2e)")
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--min-sec", type=float, default=1.0)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-runs", type=int, default=3)
    ap.add_argument("--e2e-opt-steps", type=int, default=40, help="optimizer steps of an --accum-steps 1 run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum_ab.jsonl"))
    a = ap.parse_args(argv)

    import torch

    from k8s_amd.ops._ext import load
    from k8s_amd.parallel.flat import ParamStore, init_const

    C = load()
    dev = torch.device("cuda", 0)
    sgd = sgd_gbs()

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters  # ms per pass

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
            n = store.total
            torch.manual_seed(0)
            g = store.grad
            g.normal_(0.0, 1e-3)
            acc = torch.zeros_like(g)  # the accumulate paths' destination: grows by g per pass, linearly
            zero = torch.zeros_like(g)  # the fold paths' running sum: thousands of timed folds leave g as it is
            out_bf = torch.empty(n, dtype=torch.bfloat16, device=dev)

            def torch_fold_cast():
                g.add_(zero)
                C.cast_bf16(g, out_bf)

            paths = {"accumulate_first": lambda: C.grad_accumulate(acc, g, 0, n, True),
                     "accumulate": lambda: C.grad_accumulate(acc, g, 0, n, False),
                     "fold": lambda: C.grad_fold(g, zero, 0, n, None),
                     "fold_bf16_torch": torch_fold_cast,
                     "fold_bf16": lambda: C.grad_fold(g, zero, 0, n, out_bf)}
            iters = {}
            for key, fn in paths.items():
                fn()
                torch.cuda.synchronize()
                iters[key] = max(3, math.ceil(1.1 * a.min_sec * 1e3 / timed(fn, 3)))
            ms = {k: [] for k in paths}
            for s in range(a.samples):
                for key, fn in paths.items():
                    t = timed(fn, iters[key])
                    while t * iters[key] < a.min_sec * 1e3:  # a sample shorter than --min-sec is taken again
                        iters[key] = math.ceil(iters[key] * 1.2)
                        t = timed(fn, iters[key])
                    ms[key].append(t)
                    emit({"path": key, "model": model, "elements": n, "sample": s, "iters": iters[key],
                          "ms": round(t, 5), "gb_per_sec": round(BYTES[key] * n / t / 1e6, 1)})
            for key in paths:
                mean = sum(ms[key]) / len(ms[key])
                gbs = BYTES[key] * n / mean / 1e6
                rec = {"summary": True, "model": model, "elements": n, "path": key, "bytes_per_element": BYTES[key],
                       "ms": round(mean, 5), "gb_per_sec": round(gbs, 1),
                       "of_stream_ceiling": round(gbs / STREAM_CEILING_GBS, 4),
                       "spread": round((max(ms[key]) - min(ms[key])) / mean, 4),
                       "finite": bool(torch.isfinite(g).all() and torch.isfinite(acc).all())}
                if model in sgd:
                    rec["of_fused_sgd_gb_per_sec"] = round(gbs / sgd[model], 4)
                if key == "fold_bf16":
                    rec["b_over_a"] = round(mean / (sum(ms["fold_bf16_torch"]) / len(ms["fold_bf16_torch"])), 4)
                emit(rec)
            del store, g, acc, zero, out_bf, paths
            torch.cuda.empty_cache()

        if a.e2e:
            rates = {1: [], 4: []}
            mem = {}
            for run in range(a.e2e_runs):
                for accum in (1, 4):  # alternating; the same number of micro-batches in both
                    steps = max(4, a.e2e_opt_steps // accum)
                    rate, mem[accum] = e2e_run(accum, steps, max(1, steps // 4))
                    rates[accum].append(rate)
                    emit({"e2e": True, "model": "bert_base", "batch": 1024, "seq": 128, "accum_steps": accum,
                          "run": run, "steps": steps, "tokens_per_sec": round(rate, 1), "peak_mem_gb": mem[accum]})
            m1, m4 = (sum(rates[k]) / len(rates[k]) for k in (1, 4))
            emit({"e2e": True, "summary": True, "model": "bert_base", "batch": 1024, "seq": 128,
                  "tokens_per_sec_accum1": round(m1, 1), "tokens_per_sec_accum4": round(m4, 1),
                  "accum4_over_accum1": round(m4 / m1, 4), "peak_mem_gb": mem,
                  "spread_accum1": round((max(rates[1]) - min(rates[1])) / m1, 4),
                  "spread_accum4": round((max(rates[4]) - min(rates[4])) / m4, 4)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
