"""The fused 1x1 backward (bwd1x1_fused.hip) against the two kernels it replaces, on ResNet-50's two real shapes.

Per shape (batch 3072: M = 3072 * 56 * 56 with C 64 / K 256, M = 3072 * 28 * 28 with C 128 / K 512), in one process,
interleaved per sample:

    A pair   weight gradient with x normalised on load (gemm, xform_b), then the data gradient with the
             BatchNorm-backward sums (gemm_dgrad_bnstats): gy and x read twice
    B fused  bwd1x1_fused: one pass

One JSON line per sample with ms and GB/s over the bytes the result needs (gy + x read once, dz written), and a summary
line per shape: both medians, the spread of the interleaved samples, the ratio, and the fused pass's share of the
bytes floor at the project's 6.25 TB/s streaming ceiling.

``--step`` adds the whole-step A/B: ``bench.py`` at its defaults, alternating ``K8S_AMD_BWD1X1_FUSED`` 1 / 0,
``--step-runs`` each, every run's result line recorded.

    python benchmarks/bwd1x1_fused.py [--batch 3072] [--samples 5] [--step] [--out profiles/bwd1x1_fused_ab.jsonl]
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


def bench_run(fused: bool):
    env = dict(os.environ, PYTHONPATH=ROOT, K8S_AMD_BWD1X1_FUSED="1" if fused else "0")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bwd1x1_fused_ab.jsonl"))
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
            gy = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            x = torch.randn(M, C, device=dev, dtype=torch.bfloat16) * 1.5 + 0.2
            w = (torch.randn(K, C, device=dev) * 0.05).bfloat16()
            mean = torch.full((C,), 0.2, device=dev)
            invstd = torch.full((C,), 1 / 1.5, device=dev)
            gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
            scale = gamma * invstd
            xform = torch.cat([scale, torch.addcmul(beta, -mean, scale)]).contiguous()
            dw = torch.zeros(K, C, device=dev)
            sums = torch.zeros(C_.conv_stat_replicas, 2, C, device=dev)
            need = 2 * M * (K + 2 * C)  # gy and x read once, dz written

            def pair():
                C_.gemm(gy, False, x, False, dw, True, None, 0, None, False, 1.0, 0, xform_b=xform, xform_c=C)
                return C_.gemm_dgrad_bnstats(gy, w, x, gamma, beta, mean, invstd, sums)

            def fused():
                return C_.bwd1x1_fused(gy, x, w, xform, gamma, beta, mean, invstd, dw, sums, False)

            paths = {"pair": pair, "fused": fused}
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
            emit({"summary": True, "shape": name, "M": M, "C": C, "K": K, "pair_ms": round(med["pair"], 4),
                  "fused_ms": round(med["fused"], 4), "spread_ms": round(spread, 4),
                  "fused_over_pair": round(med["fused"] / med["pair"], 4), "needed_gb": round(need / 1e9, 3),
                  "floor_ms": round(floor_ms, 4), "fused_share_of_floor": round(floor_ms / med["fused"], 4)})
            del gy, x, dw, sums
            torch.cuda.empty_cache()

    if a.step:
        runs = {True: [], False: []}
        for run in range(a.step_runs):
            for on in (True, False):
                r = bench_run(on)
                runs[on].append(r)
                emit({"step": True, "fused": on, "run": run, "result": r})
    f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
