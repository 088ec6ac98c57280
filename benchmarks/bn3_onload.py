"""bn3's backward applied on load by the fused 1x1 backward (bwd1x1_fused.hip with x3 / mask / params) against the
apply pass followed by the plain fused backward, on ResNet-50's two real shapes.

Per shape (batch 3072: M = 3072 * 56 * 56 with C 64 / K 256, M = 3072 * 28 * 28 with C 128 / K 512), in one process,
interleaved per sample:

    A apply+fused  bn_bwd_apply (read dy, x3, mask; write dx3), then bwd1x1_fused (read dx3, x; write dz)
    B onload       bwd1x1_fused with x3 / mask / params: reads dy, x3, mask and x, writes dz
    (fused         the plain fused backward alone, for what the on-load form adds to it)

One JSON line per sample with ms and GB/s over the bytes the on-load form needs (dy, x3, mask and x read once, dz
written: the 12.6 GB / 6.3 GB ledgers), and a summary line per shape: the medians, the spread of the interleaved
samples, the ratio, and the on-load form's share of its bytes floor at the project's 6.25 TB/s streaming ceiling.

``--step`` adds the whole-step A/B: ``bench.py`` at its defaults, alternating ``K8S_AMD_BN3_ONLOAD`` 1 / 0,
``--step-runs`` each, every run's result line recorded.

    python benchmarks/bn3_onload.py [--batch 3072] [--samples 5] [--step] [--out profiles/bn3_onload_ab.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STREAM_CEILING_GBS = 6250.0  # profiles/r02_stream_bw_patterns_v2.jsonl
SHAPES = [("s0.conv3", 56, 64, 256), ("s1.conv3", 28, 128, 512)]


def bench_run(onload: bool):
    env = dict(os.environ, PYTHONPATH=ROOT, K8S_AMD_BN3_ONLOAD="1" if onload else "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("bench.py failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")][-1]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=3072)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-runs", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true", help="only --step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn3_onload_ab.jsonl"))
    a = ap.parse_args(argv)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    if not a.no_kernels:
        import torch

        from k8s_amd.ops._ext import load

        C_ = load()
        dev = torch.device("cuda", 0)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.iters

        for name, hw, C, K in SHAPES:
            M = a.batch * hw * hw
            torch.manual_seed(0)
            dy = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            x3 = torch.randn(M, K, device=dev, dtype=torch.bfloat16) + 0.5
            mask = torch.randint(0, 256, (M * K // 8,), device=dev, dtype=torch.uint8)
            params = torch.cat([torch.rand(K, device=dev) + 0.5, torch.randn(K, device=dev) * 0.1,
                                torch.randn(K, device=dev) * 0.1, torch.zeros(K, device=dev)]).contiguous()
            x = torch.randn(M, C, device=dev, dtype=torch.bfloat16) * 1.5 + 0.2
            w = (torch.randn(K, C, device=dev) * 0.05).bfloat16()
            mean = torch.full((C,), 0.2, device=dev)
            invstd = torch.full((C,), 1 / 1.5, device=dev)
            gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
            scale = gamma * invstd
            xform = torch.cat([scale, torch.addcmul(beta, -mean, scale)]).contiguous()
            dw = torch.zeros(K, C, device=dev)
            sums = torch.zeros(C_.conv_stat_replicas, 2, C, device=dev)
            bn = (xform, gamma, beta, mean, invstd)
            need = 2 * M * (2 * K + 2 * C) + M * K // 8  # dy, x3, mask and x read once, dz written
            dx3 = C_.bn_bwd_apply(dy, x3, mask, params)

            def apply_fused():
                return C_.bwd1x1_fused(C_.bn_bwd_apply(dy, x3, mask, params), x, w, *bn, dw, sums, False)

            def onload():
                return C_.bwd1x1_fused(dy, x, w, *bn, dw, sums, False, x3=x3, mask=mask, params=params)

            def fused():
                return C_.bwd1x1_fused(dx3, x, w, *bn, dw, sums, False)

            paths = {"apply+fused": apply_fused, "onload": onload, "fused": fused}
            for fn in paths.values():
                fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in paths}
            for s in range(a.samples):
                for key, fn in paths.items():
                    t = timed(fn)
                    ms[key].append(t)
                    emit({"shape": name, "M": M, "C": C, "K": K, "path": key, "sample": s, "ms": round(t, 4),
                          "gb_per_sec": round(need / t / 1e6, 1)})
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = max(max(v) - min(v) for v in ms.values())
            floor_ms = need / STREAM_CEILING_GBS / 1e6
            emit({"summary": True, "shape": name, "M": M, "C": C, "K": K,
                  "apply_fused_ms": round(med["apply+fused"], 4), "onload_ms": round(med["onload"], 4),
                  "fused_ms": round(med["fused"], 4), "spread_ms": round(spread, 4),
                  "onload_over_apply_fused": round(med["onload"] / med["apply+fused"], 4),
                  "needed_gb": round(need / 1e9, 3), "onload_gb_per_sec": round(need / med["onload"] / 1e6, 1),
                  "floor_ms": round(floor_ms, 4), "onload_share_of_floor": round(floor_ms / med["onload"], 4)})
            del dy, x3, dx3, mask, x, dw, sums
            torch.cuda.empty_cache()

    if a.step:
        for run in range(a.step_runs):
            for on in (True, False):
                emit({"step": True, "bn3_onload": on, "run": run, "result": bench_run(on)})
    f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
