"""``python -m k8s_amd.generate``: sample tokens from a Llama checkpoint.

    python -m k8s_amd.generate --model llama_tiny --ckpt-dir DIR --prompt-ids 1,2,3 --prompt-ids 7,8 --max-new-tokens 16

Restores the newest ``model.ckpt-N`` of ``--ckpt-dir`` (what the trainer's ``--ckpt-dir`` writes; ``--random-init``
runs the initialised weights instead), prefills the prompts into a KV cache and decodes token by token
(``LlamaForCausalLM.generate``). Prompts are token ids: ``--prompt-ids`` (repeatable, one batch row each) or
``--prompts-npy`` (an integer array [B, S], or an object array of rows). Output: one JSON line per row, ``{"event":
"generate", "row", "prompt_len", "tokens"}``, then a ``done`` line with ``prefill_ms``, ``decode_tokens_per_sec``,
``gemm_fallbacks`` and ``linear_off_skinny`` (``ops.decode.linear`` calls that left the skinny kernel). A configuration
error exits 1 with one sentence on stderr, before the model is built.
"""
from __future__ import annotations

import argparse
import json
import sys

LLAMA_MODELS = ("llama3_8b", "llama_1b", "llama_tiny")
MAX_ROWS = 16


class ConfigError(ValueError):
    pass


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m k8s_amd.generate", description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="llama_tiny")
    ap.add_argument("--ckpt-dir", default=None)
    ap.add_argument("--random-init", action="store_true", help="run the initialised weights when there is no checkpoint")
    ap.add_argument("--prompt-ids", action="append", default=[], help="comma-separated token ids; one batch row each")
    ap.add_argument("--prompts-npy", default=None, help="a .npy file of token ids, one row per prompt")
    ap.add_argument("--max-new-tokens", type=int, default=16)
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--top-k", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--eos-id", type=int, default=None)
    ap.add_argument("--max-len", type=int, default=None, help="cache positions per row (default: prompt + new tokens)")
    ap.add_argument("--device", default="auto", choices=["auto", "cuda", "cpu"])
    ap.add_argument("--init-seed", type=int, default=0, help="seed of --random-init's weights")
    return ap.parse_args(argv)


def read_prompts(a):
    rows = []
    for text in a.prompt_ids:
        try:
            rows.append([int(t) for t in text.split(",") if t.strip() != ""])
        except ValueError:
            raise ConfigError("--prompt-ids takes comma-separated integers, got %r" % text)
    if a.prompts_npy:
        import numpy as np

        try:
            arr = np.load(a.prompts_npy, allow_pickle=False)
        except (OSError, ValueError) as e:
            raise ConfigError("--prompts-npy %s cannot be read: %s" % (a.prompts_npy, e))
        if arr.ndim != 2 or arr.dtype.kind not in "iu":
            raise ConfigError("--prompts-npy must hold an integer array [rows, tokens], got %s %s"
                              % (arr.dtype, list(arr.shape)))
        rows += [[int(t) for t in r] for r in arr]
    return rows


def check_config(a, prompts):
    """Every configuration error, as one sentence, before the model is built. Returns (config, checkpoint or None)."""
    from k8s_amd.models.registry import MODELS, token_config
    from k8s_amd.utils import checkpoint as ckpt

    if a.model not in MODELS:
        raise ConfigError("unknown model %r (choose from %s)" % (a.model, ", ".join(LLAMA_MODELS)))
    if a.model not in LLAMA_MODELS:
        raise ConfigError("generation is implemented for the Llama models only, not %s" % a.model)
    c = token_config(a.model)
    if not prompts or any(len(p) < 1 for p in prompts):
        raise ConfigError("give at least one prompt of at least one token (--prompt-ids or --prompts-npy)")
    if len(prompts) > MAX_ROWS:
        raise ConfigError("%d prompts exceed the %d rows one generation batch takes" % (len(prompts), MAX_ROWS))
    for b, p in enumerate(prompts):
        for t in p:
            if not 0 <= t < c.vocab_size:
                raise ConfigError("prompt %d holds token id %d outside %s's vocabulary [0, %d)"
                                  % (b, t, a.model, c.vocab_size))
    if a.max_new_tokens < 1:
        raise ConfigError("--max-new-tokens must be positive")
    if a.temperature < 0:
        raise ConfigError("--temperature must not be negative")
    if a.temperature != 0 and not 1 <= a.top_k <= 64:
        raise ConfigError("--top-k must be in 1..64 with a nonzero temperature, got %d" % a.top_k)
    if a.eos_id is not None and not 0 <= a.eos_id < c.vocab_size:
        raise ConfigError("--eos-id %d is outside %s's vocabulary [0, %d)" % (a.eos_id, a.model, c.vocab_size))
    need = max(len(p) for p in prompts) + a.max_new_tokens
    if a.max_len is not None and need > a.max_len:
        raise ConfigError("prompt plus --max-new-tokens = %d tokens exceed --max-len %d" % (need, a.max_len))
    if need > c.max_position:
        raise ConfigError("prompt plus --max-new-tokens = %d tokens exceed %s's max_position = %d"
                          % (need, a.model, c.max_position))
    base = ckpt.latest_checkpoint(a.ckpt_dir) if a.ckpt_dir else None
    if base is None and not a.random_init:
        raise ConfigError("no checkpoint in --ckpt-dir %s (pass --random-init to run the initialised weights)"
                          % (a.ckpt_dir,))
    return c, base


def main(argv=None) -> int:
    a = parse_args(argv)
    try:
        prompts = read_prompts(a)
        _, base = check_config(a, prompts)
    except ConfigError as e:
        print("error: %s" % e, file=sys.stderr, flush=True)
        return 1
    import torch

    if a.device == "cuda" and not torch.cuda.is_available():
        print("error: --device cuda but no GPU is visible", file=sys.stderr, flush=True)
        return 1
    dev = "cuda" if a.device == "cuda" or (a.device == "auto" and torch.cuda.is_available()) else "cpu"

    from k8s_amd.models.registry import build
    from k8s_amd.ops import decode as KD
    from k8s_amd.ops import gemm
    from k8s_amd.utils import checkpoint as ckpt

    w = build(a.model, dev, batch=len(prompts), seed=a.init_seed)
    step = None
    if base is not None:
        step, tensors, meta = ckpt.load(base)
        if meta.get("model") not in (None, a.model):
            print("error: checkpoint %s holds %s, not %s" % (base, meta.get("model"), a.model), file=sys.stderr,
                  flush=True)
            return 1
        w.store.load_state_dict({k[len("params/"):]: v for k, v in tensors.items() if k.startswith("params/")})
        w.store.refresh_lowp()
    print(json.dumps({"event": "start", "model": a.model, "device": dev, "checkpoint": base, "step": step,
                      "rows": len(prompts)}), flush=True)
    gemm.FALLBACKS.clear()
    KD.reset_counters()
    out = w.model.generate(prompts, a.max_new_tokens, a.temperature, a.top_k, a.seed, a.eos_id, a.max_len)
    for b, toks in enumerate(out):
        print(json.dumps({"event": "generate", "row": b, "prompt_len": len(prompts[b]), "tokens": toks}), flush=True)
    st = w.model.last_generate
    print(json.dumps({"event": "done", "prefill_ms": round(st["prefill_ms"], 3),
                      "decode_tokens_per_sec": round(st["decode_tokens_per_sec"], 2),
                      "decode_steps": st["decode_steps"], "gemm_fallbacks": dict(gemm.FALLBACKS),
                      "linear_off_skinny": KD.LINEAR_OTHER, "linear_skinny": KD.LINEAR_SKINNY}), flush=True)
    if w.close is not None:
        w.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
