"""What training BERT without padding (``--unpad``) gains, end to end and in attention alone.

Two token sets, both at vocabulary 30522 and ``--docs`` documents: "toy" (4 to 12 tokens per segment, the set of
``benchmarks/token_pipeline.py``: ``pad_fraction`` about 0.85 at ``--seq 128``) and "half" (``--tokens-per-segment 8
56``: pairs of 67 tokens on average that never need truncation, ``pad_fraction`` about 0.48).

``--attention``: the attention of ``bert_base --batch 1024 --seq 128`` (12 heads, D 64) on the first batch of each set,
forward and backward timed separately, three configurations alternating in one process, a sample at least ``--min-sec``
of device time between device events:

    P     padded: [1024, 128] rows with ``kv_lens`` -- the one-tile forward and the one-block backward
    S64   the stream of T rows with the span mask, 64-key tiles
    S128  the same on 128-key tiles

``--e2e``: ``python -m k8s_amd.trainer --model bert_base --batch 1024 --seq 128 --data-dir SET`` padded and with
``--unpad``, and with ``--parent-root DIR`` the padded run of the tree checked out and built at ``DIR`` (the parent
commit), alternating, ``--runs`` runs each. ``tokens_per_sec`` counts ``batch x seq`` positions in every
configuration, so the three compare directly; the median over the logged windows after the first is a run's figure.

One JSON line per sample / run and a summary line per comparison go to ``--out``.

    python benchmarks/unpad_bert.py --attention --e2e [--parent-root DIR] [--out profiles/unpad_ab.jsonl]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

VOCAB = 30522
SETS = {"toy": (4, 12), "half": (8, 56)}
BATCH, SEQ, HEADS, D = 1024, 128, 12, 64


def make_sets(root, docs):
    from k8s_amd.tools.make_dataset import make_toy_tokens

    out = {}
    for name, per_segment in SETS.items():
        out[name] = os.path.join(root, name)
        make_toy_tokens(out[name], train_docs=docs, val_docs=2, vocab=VOCAB, tokens_per_segment=per_segment)
    return out


def attention(a, sets, emit):
    import numpy as np
    import torch

    from k8s_amd.data import open_token_dataset
    from k8s_amd.data.token_loader import TokenLoader
    from k8s_amd.ops._ext import load

    dev = torch.device("cuda", 0)
    C = load()
    sc = 1.0 / math.sqrt(D)

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters  # ms per call

    def compare(what, paths, extra):
        iters = {}
        for key, fn in paths.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[key] = max(3, math.ceil(1.1 * a.min_sec * 1e3 / timed(fn, 3)))
        ms = {key: [] for key in paths}
        for s in range(a.samples):
            for key, fn in paths.items():
                t = timed(fn, iters[key])
                while t * iters[key] < a.min_sec * 1e3:  # a sample shorter than --min-sec is taken again
                    iters[key] = math.ceil(iters[key] * 1.2)
                    t = timed(fn, iters[key])
                ms[key].append(t)
                emit({"what": what, "path": key, "sample": s, "iters": iters[key], "ms": round(t, 5), **extra})
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        emit({"summary": True, "what": what, **extra,
              **{k: {"ms": round(mean[k], 5), "spread": round((max(v) - min(v)) / mean[k], 4),
                     "over_P": round(mean[k] / mean["P"], 4)} for k, v in ms.items()}})

    for name, path in sets.items():
        ds = open_token_dataset(path, need=("train",), pairs=True)
        ld = TokenLoader(ds, "train", "cpu", BATCH, SEQ, kind="bert", max_predictions=20)
        plan = ld.plan(0)
        cu, T = ld.stream_offsets(plan)
        lens = torch.from_numpy(plan["kv_lens"].astype(np.int32)).to(dev)
        seq = np.repeat(np.arange(BATCH), np.diff(cu))
        lo = np.full(T, cu[-1], dtype=np.int32)
        hi = np.full(T, T, dtype=np.int32)
        lo[:cu[-1]], hi[:cu[-1]] = cu[seq], cu[seq + 1]
        lo, hi = torch.from_numpy(lo)[None].to(dev), torch.from_numpy(hi)[None].to(dev)
        torch.manual_seed(0)
        W = 3 * HEADS * D

        def operands(B, S):
            x = torch.randn(B * S, W, device=dev).bfloat16()
            g = x.view(B, S, 3 * HEADS, D)
            return (x, g.narrow(2, 0, HEADS), g.narrow(2, HEADS, HEADS), g.narrow(2, 2 * HEADS, HEADS),
                    torch.randn(B, S, HEADS, D, device=dev).bfloat16(), torch.empty_like(x))

        fwd, bwd = {}, {}
        keep = []
        for key, (B, S, kw, kv) in {"P": (BATCH, SEQ, {}, lens),
                                    "S64": (1, T, {"span_lo": lo, "span_hi": hi, "span_tile": 64}, None),
                                    "S128": (1, T, {"span_lo": lo, "span_hi": hi, "span_tile": 128}, None)}.items():
            x, q, k, v, do, dqkv = operands(B, S)
            o, lse = C.flash_fwd(q, k, v, False, kv, sc, **kw)
            keep.append((x, do, dqkv, o, lse))
            fwd[key] = lambda q=q, k=k, v=v, kv=kv, kw=kw: C.flash_fwd(q, k, v, False, kv, sc, **kw)
            bwd[key] = lambda q=q, k=k, v=v, kv=kv, kw=kw, do=do, o=o, lse=lse, dqkv=dqkv: C.flash_bwd(
                do, q, k, v, o, lse, False, kv, sc, dqkv, None, **kw)
        extra = {"set": name, "pad_fraction": round(float(1 - plan["kv_lens"].mean() / SEQ), 4), "stream_rows": T,
                 "mean_len": round(float(plan["kv_lens"].mean()), 2)}
        compare("attention_fwd", fwd, extra)
        compare("attention_bwd", bwd, extra)
        del keep, fwd, bwd
        torch.cuda.empty_cache()


def trainer_run(root, extra, steps, log_every):
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, "-m", "k8s_amd.trainer", "--model", "bert_base", "--batch", str(BATCH), "--seq", str(SEQ),
           "--steps", str(steps), "--log-every", str(log_every)] + extra
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("trainer failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    ev = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    steps_ = [e for e in ev if e.get("event") == "step"][1:]  # the first window holds the warm-up
    start = [e for e in ev if e.get("event") == "start"][-1]
    done = [e for e in ev if e.get("event") == "done"][-1]
    real = [e["real_tokens_per_sec"] for e in steps_ if "real_tokens_per_sec" in e]
    return {"tokens_per_sec": statistics.median(e["tokens_per_sec"] for e in steps_),
            "real_tokens_per_sec": statistics.median(real) if real else None,
            "pad_fraction": (start.get("data") or {}).get("pad_fraction"),
            "stream_rows": (start.get("data") or {}).get("stream_rows"), "peak_mem_gb": done.get("peak_mem_gb"),
            "gemm_fallbacks": done.get("gemm_fallbacks"), "loss": done.get("loss")}


def e2e(a, sets, emit):
    for name, path in sets.items():
        data = ["--data-dir", path]
        configs = {"padded": (ROOT, data), "unpad": (ROOT, data + ["--unpad"])}
        if a.parent_root:
            configs["parent_padded"] = (os.path.abspath(a.parent_root), data)
        runs = {k: [] for k in configs}
        for run in range(a.runs):
            for key, (root, extra) in configs.items():
                rec = trainer_run(root, extra, a.e2e_steps, a.e2e_log_every)
                runs[key].append(rec)
                emit({"e2e": True, "set": name, "config": key, "run": run, **rec})
        med = {k: statistics.median(r["tokens_per_sec"] for r in v) for k, v in runs.items()}
        spread = {k: max(r["tokens_per_sec"] for r in v) - min(r["tokens_per_sec"] for r in v) for k, v in runs.items()}
        pad = runs["padded"][0]["pad_fraction"]
        base = "parent_padded" if a.parent_root else "padded"
        emit({"e2e_summary": True, "set": name, "pad_fraction": pad, "ideal_ratio": round(1 / (1 - pad), 3),
              "baseline": base, "unpad_over_baseline": round(med["unpad"] / med[base], 4),
              "unpad_beats_baseline_by_more_than_its_spread": bool(med["unpad"] - med[base] > spread[base]),
              **{k: {"tokens_per_sec": round(med[k], 1), "spread": round(spread[k], 1),
                     "peak_mem_gb": runs[k][0]["peak_mem_gb"]} for k in runs}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--attention", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--sets", nargs="*", default=sorted(SETS, reverse=True), choices=sorted(SETS))
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--min-sec", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--docs", type=int, default=8192)
    ap.add_argument("--e2e-steps", type=int, default=30)
    ap.add_argument("--e2e-log-every", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unpad_ab.jsonl"))
    a = ap.parse_args(argv)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    with tempfile.TemporaryDirectory() as d:
        sets = {k: v for k, v in make_sets(d, a.docs).items() if k in a.sets}
        if a.attention:
            attention(a, sets, emit)
        if a.e2e:
            e2e(a, sets, emit)
    f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
