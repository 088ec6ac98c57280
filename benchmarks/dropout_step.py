"""What dropout costs: BERT-base pretraining with and without it, and the kernels that carry it.

    A  dropout 0      the plain kernels (the same launches as before the feature)
    B  dropout 0.1    the DROP forms: mask bits regenerated from (seed, step, site, row, col), nothing stored

(a) the whole training step of ``bert_base`` (forward, backward, Adam) at ``--batch`` x ``--seq``;
(b) per kernel at BERT's shapes: attention forward + backward (packed QKV gradient) at B x 12 heads x S -- the
    one-block backward at S <= 128, the three-kernel backward above (S a multiple of 64) -- and add & LayerNorm forward
    + backward at [B * S, 768] -- each without and with dropout.

Both paths run in one process, alternating A / B per sample; a sample is at least ``--min-sec`` of device time measured
with device events. One JSON line per sample and a summary line per comparison (ms, B / A, each path's own
sample-to-sample spread) go to ``--out``.

    python benchmarks/dropout_step.py [--batch 1024] [--seq 128] [--samples 3] [--only step|kernels] [--out FILE]
                                      [--tag NAME]

``--only`` appends to ``--out``, and ``--tag`` marks every record of the run, so runs of two builds (this tree and the
one it is compared with) can share one file.
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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--min-sec", type=float, default=1.0)
    ap.add_argument("--only", choices=["step", "kernels"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_ab.jsonl"))
    ap.add_argument("--tag", default=None)
    a = ap.parse_args(argv)

    import torch

    import k8s_amd.ops.attention as A
    from k8s_amd.models.registry import build
    from k8s_amd.ops import gemm as G
    from k8s_amd.ops import nn as K
    from k8s_amd.ops import reference as ref
    from k8s_amd.ops._ext import load
    from k8s_amd.ops.optim import FusedAdam
    from k8s_amd.parallel.ddp import GradReducer

    dev = torch.device("cuda", 0)
    C = load()

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters  # ms per call

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "a" if a.only else "w")

    def emit(rec):
        if a.tag:
            rec = {"tag": a.tag, **rec}
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    def compare(what, paths, extra):
        """paths = {"A": fn, "B": fn}: alternating samples of at least --min-sec, then a summary line."""
        iters = {}
        for key, fn in paths.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[key] = max(3, math.ceil(1.1 * a.min_sec * 1e3 / timed(fn, 3)))
        ms = {"A": [], "B": []}
        for s in range(a.samples):
            for key, fn in paths.items():
                t = timed(fn, iters[key])
                while t * iters[key] < a.min_sec * 1e3:  # a sample shorter than --min-sec is taken again
                    iters[key] = math.ceil(iters[key] * 1.2)
                    t = timed(fn, iters[key])
                ms[key].append(t)
                emit({"what": what, "path": key, "dropout": 0.0 if key == "A" else a.p, "sample": s,
                      "iters": iters[key], "ms": round(t, 5), **extra})
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        emit({"summary": True, "what": what, "a_ms": round(mean["A"], 5), "b_ms": round(mean["B"], 5),
              "b_over_a": round(mean["B"] / mean["A"], 4), "b_minus_a_us": round((mean["B"] - mean["A"]) * 1e3, 2),
              "a_spread": round((max(ms["A"]) - min(ms["A"])) / mean["A"], 4),
              "b_spread": round((max(ms["B"]) - min(ms["B"])) / mean["B"], 4), **extra})

    B, S, H, D, hid = a.batch, a.seq, 12, 64, 768
    thr, scale = ref.drop_params(a.p)
    st = K.DropoutState(1, dev)

    if a.only in (None, "kernels"):
        # ---- attention forward + backward on the packed QKV layout
        torch.manual_seed(0)
        x = torch.randn(B * S, 3 * H * D, device=dev).bfloat16()
        g = x.view(B, S, 3 * H, D)
        q, k, v = g.narrow(2, 0, H), g.narrow(2, H, H), g.narrow(2, 2 * H, H)
        lens = torch.full((B,), S, device=dev, dtype=torch.int32)
        do = torch.randn(B, S, H, D, device=dev).bfloat16()
        dqkv = torch.empty_like(x)
        sc = 1.0 / math.sqrt(D)

        def attn(drop):
            kw = {"drop_state": st.tensor, "drop_thr": thr, "drop_scale": scale, "drop_site": 1} if drop else {}

            def fwd():
                return C.flash_fwd(q, k, v, False, lens, sc, **kw)

            o, lse = fwd()

            def bwd():
                C.flash_bwd(do, q, k, v, o, lse, False, lens, sc, dqkv, None, **kw)

            return fwd, bwd

        (fa, ba), (fb, bb) = attn(False), attn(True)
        shape = {"B": B, "H": H, "S": S, "D": D}
        compare("attention_fwd", {"A": fa, "B": fb}, shape)
        compare("attention_bwd", {"A": ba, "B": bb}, shape)
        del x, g, q, k, v, do, dqkv

        # ---- add & LayerNorm forward + backward (with the BiasLink column sums)
        R = B * S
        xa = torch.randn(R, hid, device=dev).bfloat16()
        r = torch.randn(R, hid, device=dev).bfloat16()
        gm, bt = torch.rand(hid, device=dev) + 0.5, torch.randn(hid, device=dev)
        dy = torch.randn(R, hid, device=dev).bfloat16()
        dg, db, dsum = (torch.empty(hid, device=dev) for _ in range(3))

        def norm(drop):
            kw = (st.tensor, thr, scale, 2) if drop else ()

            def fwd():
                return C.norm_fwd(xa, r, gm, bt, 1e-12, False, *kw)

            _, mean, rstd, xs = fwd()

            def bwd():
                if drop:
                    C.norm_bwd_dropout(dy, xs, gm, mean, rstd, None, dg, db, dsum, *kw)
                else:
                    C.norm_bwd(dy, xs, gm, mean, rstd, None, dg, db, False, dsum=dsum)

            return fwd, bwd

        (fa, ba), (fb, bb) = norm(False), norm(True)
        shape = {"R": R, "D": hid}
        compare("add_layer_norm_fwd", {"A": fa, "B": fb}, shape)
        compare("add_layer_norm_bwd", {"A": ba, "B": bb}, shape)
        del xa, r, dy
        torch.cuda.empty_cache()

    if a.only in (None, "step"):
        # ---- the whole training step
        def step_of(dropout):
            w = build("bert_base", dev, B, seq=S, seed=0, dropout=dropout)
            opt = FusedAdam(w.store, lr=1e-5, weight_decay=0.01, max_grad_norm=1.0)
            red = GradReducer(w.store)
            batch = w.batch(0)

            def step():
                red.begin_step()
                loss = w.loss(batch)
                loss.backward()
                red.finish()
                opt.step(grad_scale=red.grad_scale)

            return step

        compare("bert_base_step", {"A": step_of(None), "B": step_of(a.p)}, {"batch": B, "seq": S, "tokens": B * S})
        # counted after the timed steps: both must be empty / zero at the fused shapes (seq <= 128 or a multiple of 64)
        emit({"what": "bert_base_step_fallbacks", "gemm_fallbacks": dict(G.FALLBACKS),
              "dropout_fallbacks": A.DROPOUT_FALLBACKS})
    f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
