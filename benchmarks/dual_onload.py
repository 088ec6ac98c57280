"""The stage-1 entry block's two BatchNorm backwards applied on load (bn_bwd_dual_params, then bwd1x1_fused on load for
conv3 and its final form on load for the downsample convolution) against the dual apply pass followed by the four
kernels it feeds, at ResNet-50's real shape (batch 3072, 56x56, C 64 / K 256).

In one process, interleaved per sample, every kernel timed on its own:

    A  dual_apply        bn_bwd_dual (sums)      read dy, mask, x3, xr; write dx3, dxr       (+ the two finals)
       conv3_fused       bwd1x1_fused            read dx3, x2; write dz
       down_wgrad        conv_wgrad              read dxr, x
       down_dgrad        gemm_dgrad_bnstats_mask read dxr, addend, winner x, bits; write the addend
    B  dual_params       bn_bwd_dual_params      the two finals only
       conv3_onload      bwd1x1_fused, on load   read dy, mask, x3, x2; write dz
       down_final_onload bwd1x1_fused, final form on load
                                                 read dy, mask, xr, x, addend, winner x, bits; write the addend
    (down_final_plain    the final form fed a materialised dxr: what the form alone is worth)

One JSON line per sample with ms and TB/s over the bytes the kernel needs, and a summary line: the medians, the spread
of the interleaved samples, both chains' totals, and the byte ledger.

``--step`` adds the whole-step A/B: ``bench.py`` at its defaults, alternating ``K8S_AMD_DUAL_ONLOAD`` 0 / 1,
``--step-runs`` each, every run's result line recorded.

    python benchmarks/dual_onload.py [--batch 3072] [--samples 5] [--step] [--out profiles/dual_onload_ab.jsonl]
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


def bench_run(on: bool, extra=()):
    env = dict(os.environ, PYTHONPATH=ROOT, K8S_AMD_DUAL_ONLOAD="1" if on else "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *extra], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("bench.py failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")][-1]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=3072)
    ap.add_argument("--hw", type=int, default=56)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-runs", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true", help="only --step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dual_onload_ab.jsonl"))
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
        C, K = 64, 256
        N, H = a.batch, a.hw
        M = N * H * H

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.iters

        torch.manual_seed(0)
        bf = dict(device=dev, dtype=torch.bfloat16)
        dy = torch.randn(M, K, **bf)
        x3 = torch.randn(M, K, **bf) + 0.5
        xr = torch.randn(M, K, **bf) - 0.3
        mask = torch.randint(0, 256, (M * K // 8,), device=dev, dtype=torch.uint8)
        x2 = torch.randn(M, C, **bf) * 1.5 + 0.2   # conv3's input (bn2's, normalised on load)
        x = torch.randn(N, H, H, C, **bf)          # the block's input (the stem pool's output)
        addend = torch.randn(M, C, **bf)           # conv1's dx
        xw = torch.randn(M, C, **bf) * 1.5 + 0.4   # the pool winners' x and ReLU bits
        wbits = torch.randint(0, 256, (M * C // 8,), device=dev, dtype=torch.uint8)
        w3 = (torch.randn(K, C, device=dev) * 0.05).bfloat16()
        wd = (torch.randn(K, C, device=dev) * 0.05).bfloat16()
        R = C_.conv_stat_replicas

        def vec(c, lo=0.5):
            return torch.rand(c, device=dev) + lo

        bnK = [torch.randn(K, device=dev) * 0.1, vec(K), vec(K), torch.randn(K, device=dev) * 0.1,
               torch.zeros(K, device=dev), torch.zeros(K, device=dev)]  # mean invstd gamma beta dgamma dbeta
        bnKr = [t.clone() for t in bnK]
        sumsK, sumsKr = torch.randn(R, 2, K, device=dev), torch.randn(R, 2, K, device=dev)
        mean2, invstd2 = torch.full((C,), 0.2, device=dev), torch.full((C,), 1 / 1.5, device=dev)
        gamma2, beta2 = vec(C), torch.randn(C, device=dev) * 0.2
        scale = gamma2 * invstd2
        xform = torch.cat([scale, torch.addcmul(beta2, -mean2, scale)]).contiguous()
        bn2 = (xform, gamma2, beta2, mean2, invstd2)
        wmean = torch.full((C,), 0.4, device=dev)
        dw3, dwd = torch.zeros(K, C, device=dev), torch.zeros(K, 1, 1, C, device=dev)
        sums2, sumsp = torch.zeros(R, 2, C, device=dev), torch.zeros(R, 2, C, device=dev)
        fin = dict(addend=addend, winner_x=xw, winner_bits=wbits, winner_mean=wmean)
        none5 = (None,) * 5

        dx3, dxr = C_.bn_bwd_dual(dy, mask, x3, *bnK, xr, *bnKr, sumsK, sumsKr)
        params, params_r = C_.bn_bwd_dual_params(dy, mask, x3, *bnK, xr, *bnKr, sumsK, sumsKr)
        wide, narrow, bits = 2 * M * K, 2 * M * C, M * K // 8
        paths = {
            "dual_apply": (lambda: C_.bn_bwd_dual(dy, mask, x3, *bnK, xr, *bnKr, sumsK, sumsKr),
                           5 * wide + bits),
            "conv3_fused": (lambda: C_.bwd1x1_fused(dx3, x2, w3, *bn2, dw3, sums2, False), wide + 2 * narrow),
            "down_wgrad": (lambda: C_.conv_wgrad(x, dxr.view(N, H, H, K), dwd, 1, 0, 1, 0, False), wide + narrow),
            "down_dgrad": (lambda: C_.gemm_dgrad_bnstats_mask(dxr, wd, addend, xw, wbits, wmean, sumsp),
                           wide + 3 * narrow + M * C // 8),
            "dual_params": (lambda: C_.bn_bwd_dual_params(dy, mask, x3, *bnK, xr, *bnKr, sumsK, sumsKr), 0),
            "conv3_onload": (lambda: C_.bwd1x1_fused(dy, x2, w3, *bn2, dw3, sums2, False, x3=x3, mask=mask,
                                                     params=params), 2 * wide + bits + 2 * narrow),
            "down_final_onload": (lambda: C_.bwd1x1_fused(dy, x.view(M, C), wd, *none5, dwd.view(K, C), sumsp, False,
                                                          x3=xr, mask=mask, params=params_r, **fin),
                                  2 * wide + bits + 4 * narrow + M * C // 8),
            "down_final_plain": (lambda: C_.bwd1x1_fused(dxr, x.view(M, C), wd, *none5, dwd.view(K, C), sumsp, False,
                                                         **fin), wide + 4 * narrow + M * C // 8),
        }
        for fn, _ in paths.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        for s in range(a.samples):
            for key, (fn, need) in paths.items():
                t = timed(fn)
                ms[key].append(t)
                emit({"shape": "layer1.0", "M": M, "path": key, "sample": s, "ms": round(t, 4),
                      "needed_gb": round(need / 1e9, 3), "tb_per_sec": round(need / t / 1e9, 3)})
        med = {k: statistics.median(v) for k, v in ms.items()}
        chain_a = med["dual_apply"] + med["conv3_fused"] + med["down_wgrad"] + med["down_dgrad"]
        chain_b = med["dual_params"] + med["conv3_onload"] + med["down_final_onload"]
        emit({"summary": True, "shape": "layer1.0", "M": M, **{k + "_ms": round(v, 4) for k, v in med.items()},
              "spread_ms": round(max(max(v) - min(v) for v in ms.values()), 4),
              "chain_apply_ms": round(chain_a, 4), "chain_onload_ms": round(chain_b, 4),
              "saved_ms": round(chain_a - chain_b, 4),
              "plain_final_vs_two_kernels_ms": round(med["down_wgrad"] + med["down_dgrad"] - med["down_final_plain"], 4),
              "needed_gb": {k: round(n / 1e9, 3) for k, (_, n) in paths.items()}})

    if a.step:
        for run in range(a.step_runs):
            for on in (False, True):
                emit({"step": True, "dual_onload": on, "run": run, "result": bench_run(on)})
    f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
