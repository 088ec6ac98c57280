"""The token dataset path measured: the fused MLM batch kernel against its torch definition on the device, and the
trainer on a token dataset against the trainer on its synthetic fixed batch.

Kernel alone (default). Per shape, A and B alternate in one process, timed with device events, ``--samples`` samples of
at least ``--min-seconds`` each:

    A reference  ``ops.reference.mlm_batch`` on device tensors (the definition in torch integer ops: gathers, one sort
                 per row for the ranks, a cumulative sum for the slots), its host-side table check included
    B mlm_batch  ``ops.data.mlm_batch`` -- table validation and upload included, as the loader calls it

One JSON line per sample; one summary line per shape with the medians, B / A and A's spread. A and B are compared once
per shape before they are timed (``torch.equal``). The only bar: B is faster than A by more than A's spread.

``--e2e``: ``python -m k8s_amd.trainer --model bert_base --batch 1024 --seq 128`` in three configurations alternating,
``--runs`` runs each: A the synthetic fixed batch, B1 the resident toy token set written at BERT-base's vocabulary, B2
the same set streamed (``--data-resident-gb 0``). Tokens/s (pad positions included, as the trainer counts them) is the
median of each run's logged windows after the first, reported with the dataset's ``pad_fraction`` beside it: real rows
are shorter than the synthetic batch's full rows, so attention has less to do.

    python benchmarks/token_pipeline.py [--samples 3] [--e2e] [--out profiles/token_pipeline_ab.jsonl]
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

VOCAB, SPECIAL, TOKENS = 30522, (0, 101, 102, 103), 1 << 24
SHAPES = [("n1024.s128.p20", 1024, 128, 20), ("n256.s512.p76", 256, 512, 76)]  # (name, N, S, P)


def kernels(a, emit):
    import numpy as np
    import torch

    from k8s_amd.data.token_sampler import n_predictions
    from k8s_amd.ops import data as kdata
    from k8s_amd.ops import reference as ref
    from k8s_amd.ops._ext import load

    load()
    dev = torch.device("cuda", 0)
    g = np.random.default_rng(0)
    src = torch.from_numpy(g.integers(1000, VOCAB, size=TOKENS).astype(np.uint16).view(np.int16)).to(dev)

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

    for name, N, S, P in SHAPES:
        if a.only and name not in a.only:
            continue
        # segment pairs that fill between half of the row and all of it
        total = g.integers((S - 3) // 2, S - 2, size=N)
        la = np.maximum(1, (total * g.uniform(0.3, 0.7, size=N)).astype(np.int64))
        lb = np.maximum(1, total - la)
        n = [n_predictions(int(x + y + 3), P, int(x + y)) for x, y in zip(la, lb)]
        tab = torch.from_numpy(np.stack([g.integers(0, TOKENS - S, size=N), la, g.integers(0, TOKENS - S, size=N), lb,
                                         np.asarray(n), np.arange(N) + 12345], axis=1).astype(np.int64))
        paths = {"reference": lambda: ref.mlm_batch(src, tab, S, P, VOCAB, SPECIAL, 1),
                 "mlm_batch": lambda: kdata.mlm_batch(src, tab, S, P, VOCAB, SPECIAL, 1)}
        for x, y in zip(paths["reference"](), paths["mlm_batch"]()):
            if not torch.equal(x, y):
                raise RuntimeError("%s: the kernel and its definition disagree" % name)
        ms = {k: [] for k in paths}
        for s in range(a.samples):
            for key, fn in paths.items():
                t = sample(fn)
                ms[key].append(t)
                emit({"kernel": True, "shape": name, "path": key, "sample": s, "ms": round(t, 4)})
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        emit({"summary": True, "shape": name, "N": N, "S": S, "P": P, "reference_ms": round(med["reference"], 4),
              "mlm_batch_ms": round(med["mlm_batch"], 4), "reference_spread_ms": round(spread["reference"], 4),
              "mlm_batch_spread_ms": round(spread["mlm_batch"], 4),
              "mlm_batch_over_reference": round(med["mlm_batch"] / med["reference"], 5),
              "beats_reference_by_more_than_its_spread": bool(med["reference"] - med["mlm_batch"] >
                                                              spread["reference"])})


def trainer_run(extra, steps, log_every):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "k8s_amd.trainer", "--model", "bert_base", "--batch", "1024", "--seq", "128",
           "--steps", str(steps), "--log-every", str(log_every)] + extra
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("trainer failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    ev = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    rates = [e["tokens_per_sec"] for e in ev if e.get("event") == "step"][1:]  # the first window holds the warm-up
    start = [e for e in ev if e.get("event") == "start"][-1]
    done = [e for e in ev if e.get("event") == "done"][-1]
    return statistics.median(rates), (start.get("data") or {}).get("pad_fraction"), done.get("data")


def e2e(a, emit):
    from k8s_amd.tools.make_dataset import make_toy_tokens

    with tempfile.TemporaryDirectory() as d:
        make_toy_tokens(d, train_docs=a.e2e_docs, val_docs=2, vocab=VOCAB)
        data = ["--data-dir", d]
        configs = {"A.synthetic": [], "B1.resident": data, "B2.streamed": data + ["--data-resident-gb", "0"]}
        rates, pads = {k: [] for k in configs}, {}
        for run in range(a.runs):
            for key, extra in configs.items():
                rate, pad, info = trainer_run(extra, a.e2e_steps, a.e2e_log_every)
                rates[key].append(rate)
                pads[key] = pad
                emit({"e2e": True, "config": key, "run": run, "tokens_per_sec": rate, "pad_fraction": pad,
                      "data": info})
        emit({"e2e_summary": True, "documents": a.e2e_docs,
              **{k: {"tokens_per_sec": round(statistics.median(v), 1), "spread": round(max(v) - min(v), 1),
                     "pad_fraction": pads[k]} for k, v in rates.items()}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--only", nargs="*", default=None, help="shape names")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--e2e-docs", type=int, default=8192)
    ap.add_argument("--e2e-steps", type=int, default=30)
    ap.add_argument("--e2e-log-every", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_pipeline_ab.jsonl"))
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
