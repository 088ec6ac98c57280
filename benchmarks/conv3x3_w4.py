"""ResNet-50's 256 / 512-channel 3x3 convolutions on the 4-wave GEMM with gathered A rows (gemm256.hip ConvGather)
against the kernels they ran on before, on the four real layer shapes at batch 3072.

Per (shape, product), in one process on the same tensors, interleaved per sample:

    fwd    A parent   conv_fwd with the statistics epilogue: the staged-window kernel (14x14 / stride 1) or the generic
                      implicit GEMM (the rest)
           B w4       conv3x3_w4_fwd with the statistics epilogue
    dgrad  A parent   conv3x3_dgrad_bnstats (14x14: staged window with the BatchNorm-backward sums) or conv_fwd on dy with
                      the transformed weight (7x7: generic implicit GEMM, no sums)
           B w4       conv3x3_w4_dgrad with the BatchNorm-backward sums
           (w4_plain  the same without the sums)
           (stride-1 shapes only: the stride-2 data gradients stay on their parity route)
    wgrad  A parent   conv_wgrad with K8S_AMD_CONV3X3_W4=0: the tiled kernel (14x14), else the generic split-K GEMM
           B w4       conv_wgrad with the switch on: conv3x3_w4_wgrad (gathered B rows, tall-K split)

Every product is the same 710 GFLOP; its floor at 2.5 PF/s is 0.284 ms. One JSON line per sample with ms and TF/s, and
a summary line per (shape, product): the medians, each side's own spread (max - min), whether B's median beats A's by
more than A's spread (the rule a shape's route is kept by), and B's share of the floor.

``--step`` adds the whole-step A/B: ``bench.py`` at its defaults, alternating K8S_AMD_CONV3X3_W4 = 1 / 0 on this tree
and, with ``--parent DIR`` (a built checkout of the parent commit), that tree too; ``--step-runs`` each.

    python benchmarks/conv3x3_w4.py [--batch 3072] [--samples 5] [--step] [--parent DIR] [--out profiles/conv3x3_w4_ab.jsonl]
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

PEAK_TFS = 2500.0
# (r06 layer name, H = W, C, K, stride)
SHAPES = [("s2.b0.conv2", 28, 256, 256, 2), ("s2.bx.conv2", 14, 256, 256, 1),
          ("s3.b0.conv2", 14, 512, 512, 2), ("s3.bx.conv2", 7, 512, 512, 1)]


def bench_run(root: str, switch: str):
    env = dict(os.environ, PYTHONPATH=root, K8S_AMD_CONV3X3_W4=switch)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"], env=env, cwd=root,
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
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit for --step")
    ap.add_argument("--no-kernels", action="store_true", help="only --step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv3x3_w4_ab.jsonl"))
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

        for name, hw, C, K, st in SHAPES:
            N, ho = a.batch, (hw - 1) // st + 1
            flops = 2.0 * N * ho * ho * K * 9 * C
            torch.manual_seed(0)
            x = torch.randn(N, hw, hw, C, device=dev, dtype=torch.bfloat16) * 1.5 + 0.2
            w = (torch.randn(K, 3, 3, C, device=dev) * 0.05).bfloat16()
            stats = torch.zeros(C_.conv_stat_replicas, 2, K, device=dev)
            products = {"fwd": {
                "parent": lambda: C_.conv_fwd(x, w, st, 1, 1, False, None, 0, stats),
                "w4": lambda: C_.conv3x3_w4_fwd(x, w, st, stats)}}
            if st == 1:
                gy = torch.randn(N, hw, hw, K, device=dev, dtype=torch.bfloat16)
                wt = C_.conv_dgrad_wtrans(w)
                mean, invstd = torch.full((C,), 0.2, device=dev), torch.full((C,), 1 / 1.5, device=dev)
                gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
                sums = torch.zeros(C_.conv_stat_replicas, 2, C, device=dev)
                bn = (x, gamma, beta, mean, invstd, sums)
                staged = C_.conv3x3_staged_ok(hw, hw, C, K, 3, 3, 1, 1)
                products["dgrad"] = {
                    "parent": (lambda: C_.conv3x3_dgrad_bnstats(gy, wt, *bn)) if staged
                    else (lambda: C_.conv_fwd(gy, wt, 1, 1, 1, False, None, 0, None)),
                    "w4": lambda: C_.conv3x3_w4_dgrad(gy, wt, *bn),
                    "w4_plain": lambda: C_.conv3x3_w4_dgrad(gy, wt)}
            # the weight gradient: conv_wgrad with the switch on / off (read per call) -- off is the parent's choice
            # among the tiled, the streaming and the generic split-K kernels
            dyw = torch.randn(N, ho, ho, K, device=dev, dtype=torch.bfloat16)
            dw = torch.zeros(K, 3, 3, C, device=dev)

            def wgrad(switch):
                def run():
                    os.environ["K8S_AMD_CONV3X3_W4"] = switch
                    C_.conv_wgrad(x, dyw, dw, st, 1, 1, 0, False)
                    os.environ["K8S_AMD_CONV3X3_W4"] = "1"
                return run

            assert C_.conv3x3_w4_wgrad_use(N, hw, hw, C, K, st)
            products["wgrad"] = {"parent": wgrad("0"), "w4": wgrad("1")}
            for prod, paths in products.items():
                for fn in paths.values():
                    fn()
                torch.cuda.synchronize()
                ms = {k: [] for k in paths}
                for s in range(a.samples):
                    for key, fn in paths.items():
                        t = timed(fn)
                        ms[key].append(t)
                        emit({"shape": name, "product": prod, "N": N, "H": hw, "C": C, "K": K, "stride": st,
                              "path": key, "sample": s, "ms": round(t, 4), "tf_per_sec": round(flops / t / 1e9, 1)})
                med = {k: statistics.median(v) for k, v in ms.items()}
                spread = {k: max(v) - min(v) for k, v in ms.items()}
                floor_ms = flops / PEAK_TFS / 1e9
                rec = {"summary": True, "shape": name, "product": prod, "N": N, "H": hw, "C": C, "K": K, "stride": st,
                       "floor_ms": round(floor_ms, 4)}
                for k in paths:
                    rec[k + "_ms"] = round(med[k], 4)
                    rec[k + "_spread_ms"] = round(spread[k], 4)
                    rec[k + "_tf_per_sec"] = round(flops / med[k] / 1e9, 1)
                rec["w4_over_parent"] = round(med["w4"] / med["parent"], 4)
                rec["w4_wins"] = bool(med["parent"] - med["w4"] > spread["parent"])
                rec["w4_share_of_floor"] = round(floor_ms / med["w4"], 4)
                emit(rec)
            del x, w, products
            torch.cuda.empty_cache()

    if a.step:
        trees = [("this", ROOT, "1"), ("this_off", ROOT, "0")] + ([("parent", a.parent, "1")] if a.parent else [])
        for run in range(a.step_runs):
            for tree, root, switch in trees:
                emit({"step": True, "tree": tree, "run": run, "result": bench_run(root, switch)})
    f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
