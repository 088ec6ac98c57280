"""What the document-boundary mask costs and saves in the attention kernels.

    A   the plain causal call
    B1  the DOC forms with one document per row    (the cost of the DOC form itself: the same tiles as A)
    B2  the DOC forms with 8 documents of 512 tokens
    B3  the DOC forms with 64 documents of 64 tokens

at two shapes, B 1 x S 4096: Llama-3-8B's attention (32 query / 8 KV heads, D 128) and ``llama_1b``'s (32 / 8, D 64),
q / k / v as column slices of one packed tensor, the backward writing the packed gradient. Forward and backward are
timed separately. All configurations run in one process, alternating per sample; a sample is at least ``--min-sec`` of
device time between device events. One JSON line per sample and a summary line per (shape, pass, configuration) go to
``--out``: ms, B / A, each path's own sample-to-sample spread and, from the tables alone, the share of A's tiles the
configuration visits (key tiles per 128-query block in the forward, query tiles per 64-key block in dK/dV).

    python benchmarks/doc_mask_attention.py [--seq 4096] [--samples 3] [--min-sec 1.0] [--out FILE]
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


def tile_shares(lo, hi, S, D):
    """(forward, dK/dV): tiles a configuration visits over the tiles A visits, at the kernels' block-level bounds."""
    tile = 64 if D == 128 else (128 if S >= 1024 else 64)
    fwd_a = fwd_b = kv_a = kv_b = 0
    for q0 in range(0, S, 128):
        ntiles = -(-min(S, q0 + 128) // tile)
        fwd_a += ntiles
        fwd_b += ntiles - int(lo[q0]) // tile
    for k0 in range(0, S, 64):
        qt0, nqt = k0 // tile, -(-S // tile)
        kv_a += nqt - qt0
        kv_b += min(nqt, -(-int(hi[min(k0 + 63, S - 1)]) // tile)) - qt0
    return fwd_b / fwd_a, kv_b / kv_a


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--min-sec", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "doc_mask_ab.jsonl"))
    a = ap.parse_args(argv)

    import torch

    from k8s_amd.ops._ext import load
    from k8s_amd.ops.attention import doc_bounds

    dev = torch.device("cuda", 0)
    C = load()
    S = a.seq

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters  # ms per call

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    def compare(what, paths, extra, shares):
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
        spread = {k: (max(v) - min(v)) / mean[k] for k, v in ms.items()}
        for key in paths:
            if key != "A":
                emit({"summary": True, "what": what, "path": key, "a_ms": round(mean["A"], 5),
                      "b_ms": round(mean[key], 5), "b_over_a": round(mean[key] / mean["A"], 4),
                      "tiles_over_a": round(shares[key], 4), "a_spread": round(spread["A"], 4),
                      "b_spread": round(spread[key], 4), **extra})

    configs = {"B1": S, "B2": 512, "B3": 64}  # document length
    for name, Hq, Hkv, D in (("llama3_8b", 32, 8, 128), ("llama_1b", 32, 8, 64)):
        torch.manual_seed(0)
        x = torch.randn(S, (Hq + 2 * Hkv) * D, device=dev).bfloat16()
        g = x.view(1, S, Hq + 2 * Hkv, D)
        q, k, v = g.narrow(2, 0, Hq), g.narrow(2, Hq, Hkv), g.narrow(2, Hq + Hkv, Hkv)
        do = torch.randn(1, S, Hq, D, device=dev).bfloat16()
        dqkv = torch.empty_like(x)
        sc = 1.0 / math.sqrt(D)
        fwd, bwd, sh_f, sh_b = {}, {}, {}, {}
        for key, n in [("A", None)] + list(configs.items()):
            kw = {}
            if n is not None:
                idx = torch.arange(S)
                lo, hi = doc_bounds((idx // n * n)[None])
                sh_f[key], sh_b[key] = tile_shares(lo[0].tolist(), hi[0].tolist(), S, D)
                kw = {"doc_lo": lo.to(dev), "doc_hi": hi.to(dev)}
            o, lse = C.flash_fwd(q, k, v, True, None, sc, **kw)
            fwd[key] = lambda kw=kw: C.flash_fwd(q, k, v, True, None, sc, **kw)
            bwd[key] = lambda kw=kw, o=o, lse=lse: C.flash_bwd(do, q, k, v, o, lse, True, None, sc, dqkv, None, **kw)
        shape = {"shape": name, "B": 1, "S": S, "Hq": Hq, "Hkv": Hkv, "D": D}
        compare("attention_fwd", fwd, shape, sh_f)
        compare("attention_bwd", bwd, shape, sh_b)
        del x, g, q, k, v, do, dqkv, fwd, bwd
        torch.cuda.empty_cache()
    f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
