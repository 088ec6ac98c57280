"""An identity bottleneck's conv1 backward with bn1's apply pass on load (conv1_fused.hip) against the three launches
it replaces, on ResNet-50's two real shapes.

Per shape (batch 3072: M = 3072 * 56 * 56 with W 64 / N 256 -- layer1.2; M = 3072 * 28 * 28 with W 128 / N 512 --
layer2.2, layer2.3), in one process on the same tensors, interleaved per sample:

    A parent  bn_bwd_apply (read dz1, x1; write dx1), gemm_short's masked-addend data gradient with the sums (read dx1,
              dy, x3, two masks; write dx), the weight gradient ops.conv._wgrad_hip picks (read dx1, xin)
    B fused   conv1_fused: reads dz1, x1, xin, dy, x3 and the two masks once, writes dx

One JSON line per sample with ms and GB/s over the bytes the fused form needs (the 22.8 GB / 11.4 GB ledgers), and a
summary line per shape: the medians, each path's own spread over the interleaved samples, the ratio, and the fused
form's share of its bytes floor at the project's 6.25 TB/s streaming ceiling. A layer stays on the route only where the
fused median beats the parent's by more than the parent's spread (``keeps_route``).

``--step`` adds the whole-step A/B: ``bench.py`` at its defaults, alternating K8S_AMD_CONV1_FUSED 1 / 0 and, with
``--parent DIR`` (a built checkout of the parent commit), that tree; ``--step-runs`` each, every result line recorded.

    python benchmarks/conv1_fused.py [--batch 3072] [--samples 5] [--step] [--parent DIR]
                                     [--out profiles/conv1_fused_ab.jsonl]
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
SHAPES = [("layer1.2.conv1", 56, 64), ("layer2.2-3.conv1", 28, 128)]


def bench_run(root: str, fused):
    env = dict(os.environ, PYTHONPATH=root)
    if fused is not None:
        env["K8S_AMD_CONV1_FUSED"] = "1" if fused else "0"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"], env=env, cwd=root,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("bench.py failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")][-1]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=3072)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-runs", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for --step")
    ap.add_argument("--no-kernels", action="store_true", help="only --step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv1_fused_ab.jsonl"))
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

        from k8s_amd.ops import conv as kc
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

        for name, hw, W in SHAPES:
            N, M = 4 * W, a.batch * hw * hw
            torch.manual_seed(0)
            dz1 = torch.randn(M, W, device=dev, dtype=torch.bfloat16)
            x1 = torch.randn(M, W, device=dev, dtype=torch.bfloat16) * 1.5
            params = torch.cat([torch.rand(W, device=dev) + 0.5, torch.randn(W, device=dev) * 0.1,
                                torch.randn(W, device=dev) * 0.1, torch.randn(W, device=dev) * 0.2]).contiguous()
            w = (torch.randn(W, N, device=dev) * 0.05).bfloat16()
            xin = torch.randn(M, N, device=dev, dtype=torch.bfloat16) + 0.3
            dy = torch.randn(M, N, device=dev, dtype=torch.bfloat16)
            x3 = torch.randn(M, N, device=dev, dtype=torch.bfloat16) * 1.5 + 0.2
            amask = torch.randint(0, 256, (M * N // 8,), device=dev, dtype=torch.uint8)
            bits = torch.randint(0, 256, (M * N // 8,), device=dev, dtype=torch.uint8)
            mean = torch.full((N,), 0.2, device=dev)
            dw = torch.zeros(W, 1, 1, N, device=dev)
            sums = torch.zeros(C_.conv_stat_replicas, 2, N, device=dev)
            # dz1, x1, xin, dy, x3 and two masks read once, dx written
            need = 2 * M * (2 * W + 4 * N) + 2 * (M * N // 8)
            parent_bytes = need + 3 * 2 * M * W  # + dx1 written once and read twice

            def parent():
                dx1 = C_.bn_bwd_apply(dz1, x1, None, params)
                dx = C_.dgrad_short_bnstats(dx1, w, dy, amask, x3, bits, mean, sums)
                kc._wgrad_hip(C_, dx1.view(a.batch, hw, hw, W), xin.view(a.batch, hw, hw, N), dw, 1, 0, False)
                return dx

            def fused():
                return C_.conv1_fused(dz1, x1, params, w, xin, dy, amask, x3, bits, mean, sums, dw.view(W, N), False)

            paths = {"parent": parent, "fused": fused}
            for fn in paths.values():
                fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in paths}
            for s in range(a.samples):
                for key, fn in paths.items():
                    t = timed(fn)
                    ms[key].append(t)
                    emit({"shape": name, "M": M, "W": W, "N": N, "path": key, "sample": s, "ms": round(t, 4),
                          "gb_per_sec": round(need / t / 1e6, 1)})
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = {k: max(v) - min(v) for k, v in ms.items()}
            floor_ms = need / STREAM_CEILING_GBS / 1e6
            emit({"summary": True, "shape": name, "M": M, "W": W, "N": N,
                  "parent_ms": round(med["parent"], 4), "fused_ms": round(med["fused"], 4),
                  "parent_spread_ms": round(spread["parent"], 4), "fused_spread_ms": round(spread["fused"], 4),
                  "fused_over_parent": round(med["fused"] / med["parent"], 4),
                  "keeps_route": bool(med["parent"] - med["fused"] > spread["parent"]),
                  "needed_gb": round(need / 1e9, 3), "parent_gb": round(parent_bytes / 1e9, 3),
                  "predicted_fused_over_parent": round(need / parent_bytes, 4),
                  "fused_gb_per_sec": round(need / med["fused"] / 1e6, 1),
                  "parent_gb_per_sec": round(parent_bytes / med["parent"] / 1e6, 1),
                  "floor_ms": round(floor_ms, 4), "fused_share_of_floor": round(floor_ms / med["fused"], 4)})
            del dz1, x1, xin, dy, x3, amask, bits, dw, sums
            torch.cuda.empty_cache()

    if a.step:
        arms = [("fused", ROOT, True), ("switch_off", ROOT, False)]
        if a.parent:
            arms.append(("parent", os.path.abspath(a.parent), None))
        for run in range(a.step_runs):
            for arm, root, fused in arms:
                emit({"step": True, "arm": arm, "run": run, "result": bench_run(root, fused)})
    f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
