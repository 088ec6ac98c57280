"""One decode step of one Llama layer plus the LM head: what the tree could do before the decode kernels, and with them.

    A   the training kernels at M = B: ``gemm.linear_fwd`` (what ``ops.nn.linear`` runs) for the QKV, O, gate|up, down
        and LM-head products, and ``attention(q [B, 1, Hq, D], cache, kv_lens=)`` on a token-major cache -- on the
        flash forward when ``flash_plan`` takes the shape, else the reference (the ``attention_route`` field says which)
    B   ``linear_skinny`` for the five products, ``kv_append`` and ``decode_attention``

for ``llama_1b`` and Llama-3-8B layers, B in {1, 8, 16}, context 2,048. The norms, the rotary embedding and the SwiGLU
are the same kernels on both sides and are left out. A and B alternate in one process; a sample is at least
``--min-sec`` of device time between device events, ``--samples`` samples each. Every kernel is also timed alone (one
sample of ``--kernel-sec``); the skinny GEMM's rate is its weight bytes over its time, as a fraction of the 6.25 TB/s
read-1-write-1 figure of ``profiles/r02_stream_bw_patterns_v2.jsonl``. One JSON line per sample and a summary per shape
go to ``--out``.

    python benchmarks/decode_step.py [--samples 3] [--min-sec 1.0] [--out FILE]
    python benchmarks/decode_step.py --e2e [--out FILE]   # python -m k8s_amd.generate on llama_1b --random-init:
                                                          # 128 prompt tokens, 256 new ones, rows 1 and 16
"""
from __future__ import annotations

import argparse
import json
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STREAM_TBS = 6.25
SHAPES = {  # hidden, heads, kv heads, head dim, intermediate, vocab
    "llama_1b": (2048, 32, 8, 64, 8192, 128256),
    "llama3_8b": (4096, 32, 8, 128, 14336, 128256),
}


def e2e(a, emit) -> int:
    import numpy as np

    for rows in (1, 16):
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "prompts.npy")
            np.save(path, np.random.default_rng(rows).integers(0, 128256, size=(rows, 128), dtype=np.int64))
            cmd = [sys.executable, "-m", "k8s_amd.generate", "--model", "llama_1b", "--random-init", "--prompts-npy",
                   path, "--max-new-tokens", "256", "--device", "cuda"]
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT))
        if p.returncode != 0:
            print(p.stderr[-2000:], file=sys.stderr)
            return 1
        done = [json.loads(line) for line in p.stdout.splitlines() if line.startswith('{"event": "done"')][-1]
        emit({"what": "e2e", "model": "llama_1b", "rows": rows, "prompt_tokens": 128, "new_tokens": 256,
              "prefill_ms": done["prefill_ms"], "decode_tokens_per_sec": done["decode_tokens_per_sec"],
              "gemm_fallbacks": done["gemm_fallbacks"], "linear_off_skinny": done["linear_off_skinny"]})
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--min-sec", type=float, default=1.0)
    ap.add_argument("--kernel-sec", type=float, default=0.2)
    ap.add_argument("--context", type=int, default=2048)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_ab.jsonl"))
    a = ap.parse_args(argv)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "a" if a.e2e else "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    if a.e2e:
        rc = e2e(a, emit)
        f.close()
        return rc

    import torch

    from k8s_amd.ops import decode as KD
    from k8s_amd.ops import gemm
    from k8s_amd.ops._ext import load
    from k8s_amd.ops.attention import _flash_ok, _plan, attention

    dev = torch.device("cuda", 0)
    C = load()
    ctx = a.context

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters  # ms per call

    def sample(fn, iters, min_sec):
        t = timed(fn, iters)
        while t * iters < min_sec * 1e3:  # a sample shorter than asked for is taken again
            iters = math.ceil(iters * 1.2)
            t = timed(fn, iters)
        return t, iters

    def warm(fn, min_sec):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        return max(3, math.ceil(1.1 * min_sec * 1e3 / timed(fn, 3)))

    for name, (H, Hq, Hkv, D, F, V) in SHAPES.items():
        torch.manual_seed(0)
        W = (Hq + 2 * Hkv) * D
        weights = {"qkv": (W, H), "o": (H, Hq * D), "gate_up": (2 * F, H), "down": (H, F), "lm_head": (V, H)}
        w = {k: (torch.randn(n, kk, device=dev) * 0.02).bfloat16() for k, (n, kk) in weights.items()}
        for B in (1, 8, 16):
            x = {k: torch.randn(B, kk, device=dev).bfloat16() for k, (n, kk) in weights.items()}
            lens_host = torch.full((B,), ctx, dtype=torch.int32)
            lens = lens_host.to(dev)
            start_host = lens_host - 1
            start = start_host.to(dev)
            qkv = torch.randn(B, W, device=dev).bfloat16()
            q = qkv[:, : Hq * D].view(B, Hq, D)
            ck = torch.randn(B, Hkv, ctx, D, device=dev).bfloat16()
            cv = torch.randn(B, Hkv, ctx, D, device=dev).bfloat16()
            # A's cache: token-major, the layout ops.attention takes
            ak, av = ck.permute(0, 2, 1, 3).contiguous(), cv.permute(0, 2, 1, 3).contiguous()
            aq = q.reshape(B, 1, Hq, D)
            sc = 1.0 / math.sqrt(D)
            flash = bool(_flash_ok(aq, ak, av) and _plan("plain", D, B, 1, ctx, Hq, Hkv, False, True,
                                                         max(t.stride(1) for t in (aq, ak, av)))["ok"])
            kern_a = {k: (lambda k=k: gemm.linear_fwd(x[k], w[k], None)) for k in weights}
            kern_a["attention"] = lambda: attention(aq, ak, av, kv_lens=lens, scale=sc)
            kern_b = {k: (lambda k=k: C.linear_skinny(x[k], w[k])) for k in weights}
            kern_b["kv_append"] = lambda: C.kv_append(qkv, ck, cv, start, start_host, 1, Hq)
            kern_b["attention"] = lambda: C.decode_attention(q, ck, cv, lens, lens_host, sc)
            with torch.no_grad():
                # the two sides compute the same thing
                for k in weights:
                    ya, yb = kern_a[k]()[0].float(), kern_b[k]().float()
                    assert float((ya - yb).abs().max()) <= 2e-2 * max(1.0, float(ya.abs().max())), k
                oa, ob = kern_a["attention"]().reshape(B, -1).float(), kern_b["attention"]().float()
                assert float((oa - ob).abs().max()) <= 2e-2 * max(1.0, float(oa.abs().max()))
                shape = {"shape": name, "B": B, "context": ctx, "attention_route": "flash_fwd" if flash else
                         "reference"}
                per = {}
                for side, kerns in (("A", kern_a), ("B", kern_b)):
                    for k, fn in kerns.items():
                        t, it = sample(fn, warm(fn, a.kernel_sec), a.kernel_sec)
                        per[side + "." + k] = t
                        rec = {"what": "kernel", "path": side, "kernel": k, "iters": it, "ms": round(t, 5), **shape}
                        if k in weights:
                            gbs = weights[k][0] * weights[k][1] * 2 / (t * 1e-3) / 1e9
                            rec.update(weight_gbs=round(gbs, 1), of_stream=round(gbs / (STREAM_TBS * 1e3), 4))
                        emit(rec)
                steps = {"A": lambda: [fn() for fn in kern_a.values()], "B": lambda: [fn() for fn in kern_b.values()]}
                iters = {k: warm(fn, a.min_sec) for k, fn in steps.items()}
                ms = {"A": [], "B": []}
                for s in range(a.samples):
                    for k, fn in steps.items():
                        t, iters[k] = sample(fn, iters[k], a.min_sec)
                        ms[k].append(t)
                        emit({"what": "step", "path": k, "sample": s, "iters": iters[k], "ms": round(t, 5), **shape})
            mean = {k: sum(v) / len(v) for k, v in ms.items()}
            spread = {k: (max(v) - min(v)) / mean[k] for k, v in ms.items()}
            wbytes = sum(n * kk * 2 for n, kk in weights.values())
            b_lin = sum(per["B." + k] for k in weights)
            emit({"summary": True, "what": "step", "a_ms": round(mean["A"], 5), "b_ms": round(mean["B"], 5),
                  "b_over_a": round(mean["B"] / mean["A"], 4), "a_spread": round(spread["A"], 4),
                  "b_spread": round(spread["B"], 4), "b_beats_a_by_more_than_a_spread":
                  bool(mean["A"] - mean["B"] > (max(ms["A"]) - min(ms["A"]))),
                  "skinny_weight_gbs": round(wbytes / (b_lin * 1e-3) / 1e9, 1),
                  "skinny_of_stream": round(wbytes / (b_lin * 1e-3) / 1e9 / (STREAM_TBS * 1e3), 4), **shape})
            del x, qkv, q, ck, cv, ak, av, aq
            torch.cuda.empty_cache()
        del w
        torch.cuda.empty_cache()
    f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
