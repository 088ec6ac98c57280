"""Llama-3 decoder (8B and small test configs) on the k8s_amd op set.

BASELINE config 4: "Llama-3 8B TfJob 8 WORKER ring all-reduce (no PS), bf16,
CDNA4 MFMA GEMM path". Architecture = Llama-3-8B: vocab 128256, hidden 4096,
32 layers, 32 query heads / 8 KV heads (GQA), head dim 128, SwiGLU FFN 14336,
RMSNorm eps 1e-5, RoPE theta 500000, untied embeddings (8.03 B parameters).

MI355X sizing: bf16 weights 16 GB + fp32 master 32 GB + fp32
grads 32 GB + Adam 64 GB fit one 288 GB GPU with room for activations, so the
8-GPU config is pure data parallel with a ring all-reduce of the flat gradient
buffer (``parallel/ddp.py``) -- no tensor/pipeline parallelism needed.

Per layer: RMSNorm (fused residual add) -> fused QKV GEMM [T, 6144] with RoPE on
q/k in its epilogue -> causal GQA flash attention -> O GEMM -> RMSNorm (+residual) -> fused
gate|up GEMM [T, 28672] -> SwiGLU -> down GEMM.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass

import torch
import torch.nn as nn

from k8s_amd.ops import decode as KD
from k8s_amd.ops import nn as K
from k8s_amd.ops import sampling
from k8s_amd.ops.attention import attention_qkv
from k8s_amd.parallel.flat import ParamStore, init_const, init_normal


@dataclass
class LlamaConfig:
    vocab_size: int = 128256
    hidden: int = 4096
    layers: int = 32
    heads: int = 32
    kv_heads: int = 8
    intermediate: int = 14336
    max_position: int = 8192
    rope_theta: float = 500000.0
    eps: float = 1e-5
    init_std: float = 0.02

    @property
    def head_dim(self) -> int:
        return self.hidden // self.heads


LLAMA3_8B = LlamaConfig()
LLAMA_TINY = LlamaConfig(vocab_size=512, hidden=256, layers=2, heads=4, kv_heads=2, intermediate=512,
                         max_position=256)
# a ~1B-parameter shape for quick single-GPU checks of the same kernels
LLAMA_1B = LlamaConfig(vocab_size=128256, hidden=2048, layers=16, heads=32, kv_heads=8, intermediate=8192)


class LlamaLayer(nn.Module):
    def __init__(self, store: ParamStore, name: str, c: LlamaConfig):
        super().__init__()
        self.c = c
        h, d = c.hidden, c.head_dim
        std = init_normal(c.init_std)
        out_std = init_normal(c.init_std / math.sqrt(2 * c.layers))
        self.attn_norm = store.new(name + ".input_layernorm.weight", (h,), init_const(1), decay=False, lowp=False)
        self.qkv = store.new(name + ".self_attn.qkv_proj.weight", ((c.heads + 2 * c.kv_heads) * d, h), std)
        self.o = store.new(name + ".self_attn.o_proj.weight", (h, c.heads * d), out_std)
        self.mlp_norm = store.new(name + ".post_attention_layernorm.weight", (h,), init_const(1), decay=False,
                                  lowp=False)
        # rows: blocks of 64 gate rows then the matching 64 up rows (ops.nn.linear_swiglu), so every wave tile of the
        # gate|up GEMM holds matching gate / up columns and its epilogue applies the SwiGLU; halves if F % 64 != 0
        self.gate_up = store.new(name + ".mlp.gate_up_proj.weight", (2 * c.intermediate, h), std)
        self.swiglu_blk = 64 if c.intermediate % 64 == 0 else 0
        self.down = store.new(name + ".mlp.down_proj.weight", (h, c.intermediate), out_std)

    def forward(self, x, res, B, S, pos, table, doc=None):
        """x: this layer's input stream delta, res: running residual (None for the first layer).
        Returns (delta, residual) so every residual add is fused into the next RMSNorm. ``doc`` = (lo, hi): the
        document-boundary mask of ``ops.attention`` (``pos`` then restarts at every document)."""
        c = self.c
        d = c.head_dim
        if res is None:
            res = x
            hn = K.rms_norm(x, self.attn_norm, c.eps)
        else:
            hn, res = K.rms_norm(x, self.attn_norm, c.eps, residual=res)
        # the q / k rotary embedding in the QKV GEMM's epilogue where the kernel takes the shape (else in place below)
        qkv, rotated = K.linear_rope(hn, self.qkv, pos, table, (c.heads + c.kv_heads) * d)
        # causal GQA flash attention and the packed QKV gradient in one op (no split/cat/copies)
        kw = {} if doc is None else {"doc": doc}
        o = attention_qkv(qkv, B, S, c.heads, c.kv_heads, d, causal=True, rope=(pos, table),
                          rope_in_place=True,  # qkv: this linear's output, read by nothing else
                          rope_applied=rotated, **kw)
        a = K.linear(o.reshape(B * S, c.heads * d), self.o)
        hn, res = K.rms_norm(a, self.mlp_norm, c.eps, residual=res)
        sl = K.SwiGLULink(self.swiglu_blk)  # the SwiGLU backward inside the down projection's data gradient
        # gate|up projection + SwiGLU: one GEMM with the SwiGLU in its epilogue where the kernel takes the shape
        f = K.linear(K.linear_swiglu(hn, self.gate_up, link=sl, blk=self.swiglu_blk), self.down, swiglu_in=sl)
        return f, res

    def prefill(self, x, res, B, S, pos, table, cache_k, cache_v, start, start_host):
        """``forward`` without autograd state that also appends the rotated k / v of all S tokens to the caches."""
        c = self.c
        d = c.head_dim
        if res is None:
            res = x
            hn = K.rms_norm(x, self.attn_norm, c.eps)
        else:
            hn, res = K.rms_norm(x, self.attn_norm, c.eps, residual=res)
        rot = (c.heads + c.kv_heads) * d
        qkv, rotated = K.linear_rope(hn, self.qkv, pos, table, rot)
        if not rotated:  # (the cache holds rotated keys, so rotate the packed output itself, then attend without rope)
            qkv = KD.rope_(qkv.contiguous(), rot, pos, table)
        KD.kv_append(qkv, cache_k, cache_v, start, start_host, S, c.heads)
        o = attention_qkv(qkv, B, S, c.heads, c.kv_heads, d, causal=True)
        a = K.linear(o.reshape(B * S, c.heads * d), self.o)
        hn, res = K.rms_norm(a, self.mlp_norm, c.eps, residual=res)
        return K.linear(K.linear_swiglu(hn, self.gate_up, blk=self.swiglu_blk), self.down), res

    def decode(self, x, res, pos, table, cache_k, cache_v, lens, lens_host, new_lens, new_lens_host):
        """One token per row: x [B, hidden]; the row's k / v go to cache position ``lens`` and it attends to the
        ``new_lens = lens + 1`` positions written so far."""
        c = self.c
        d = c.head_dim
        if res is None:
            res = x
            hn = K.rms_norm(x, self.attn_norm, c.eps)
        else:
            hn, res = K.rms_norm(x, self.attn_norm, c.eps, residual=res)
        qkv = KD.rope_(KD.linear(hn, self.qkv), (c.heads + c.kv_heads) * d, pos, table)
        KD.kv_append(qkv, cache_k, cache_v, lens, lens_host, 1, c.heads)
        q = qkv[:, : c.heads * d].view(x.shape[0], c.heads, d)  # (a strided view: no copy)
        o = KD.decode_attention(q, cache_k, cache_v, new_lens, new_lens_host, 1.0 / math.sqrt(d))
        hn, res = K.rms_norm(KD.linear(o, self.o), self.mlp_norm, c.eps, residual=res)
        return KD.linear(K.swiglu(KD.linear(hn, self.gate_up), blk=self.swiglu_blk), self.down), res


class KVCache:
    """The per-layer key / value caches of ``batch`` sequences of up to ``max_len`` tokens ([batch, kv_heads, max_len,
    head_dim] each, uninitialised: nothing reads a position before it is written), the sequences' lengths on the
    device (``lens``, int32) and their host mirror (``lens_host``), which is what every check reads."""

    def __init__(self, c: LlamaConfig, batch: int, max_len: int, device, dtype=torch.bfloat16):
        if batch < 1 or max_len < 1:
            raise ValueError("KVCache: batch and max_len must be positive")
        self.c, self.batch, self.max_len, self.dtype = c, int(batch), int(max_len), dtype
        self.device = torch.device(device)
        shape = (self.batch, c.kv_heads, self.max_len, c.head_dim)
        self.k = [torch.empty(shape, device=self.device, dtype=dtype) for _ in range(c.layers)]
        self.v = [torch.empty(shape, device=self.device, dtype=dtype) for _ in range(c.layers)]
        self.lens = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self.lens_host = torch.zeros(self.batch, dtype=torch.int32)

    def set_lens(self, lens_host) -> None:
        self.lens_host = torch.as_tensor(lens_host, dtype=torch.int32).reshape(-1).cpu().contiguous().clone()
        self.lens.copy_(self.lens_host)


class LlamaForCausalLM(nn.Module):
    def __init__(self, store: ParamStore, c: LlamaConfig = LLAMA3_8B):
        super().__init__()
        self.store, self.c = store, c
        std = init_normal(c.init_std)
        self.embed = store.new("model.embed_tokens.weight", (c.vocab_size, c.hidden), std)
        self.layers = nn.ModuleList([LlamaLayer(store, "model.layers.%d" % i, c) for i in range(c.layers)])
        self.norm = store.new("model.norm.weight", (c.hidden,), init_const(1), decay=False, lowp=False)
        self.lm_head = store.new("lm_head.weight", (c.vocab_size, c.hidden), std)
        self.table = None

    def finalize(self, device, **kw):
        self.store.finalize(device, **kw)
        self.table = K.rope_table(self.c.max_position, self.c.head_dim, self.c.rope_theta, device)
        return self.to(device)

    def forward(self, input_ids, labels, doc_lo=None, doc_hi=None, pos=None, dtype=torch.bfloat16):
        """``doc_lo``, ``doc_hi``, ``pos`` (int32 [B, S], all three or none; ``ops.data.causal_doc_batch``): rows that
        pack several documents -- attention stays inside each token's document and ``pos``, restarting at every
        document, replaces 0 .. S - 1."""
        B, S = input_ids.shape
        c = self.c
        doc = None
        if doc_lo is None and doc_hi is None and pos is None:
            pos = torch.arange(S, device=input_ids.device, dtype=torch.int32).repeat(B)
        elif doc_lo is None or doc_hi is None or pos is None:
            raise ValueError("doc_lo, doc_hi and pos go together")
        else:
            doc = (doc_lo, doc_hi)
            pos = pos.to(torch.int32).reshape(-1).contiguous()
        x = K.embedding_sum([(input_ids, self.embed)], S, dtype).reshape(B * S, c.hidden)
        res = None
        for layer in self.layers:
            x, res = layer(x, res, B, S, pos, self.table, doc)
        hn, _ = K.rms_norm(x, self.norm, c.eps, residual=res)
        logits = K.linear(hn, self.lm_head)
        return K.cross_entropy(logits, labels.reshape(-1))

    # ------------------------------------------------------------------------------------------------ generation
    @torch.no_grad()
    def prefill(self, ids, lens, cache: KVCache, all_logits: bool = False):
        """Run the prompts ``ids`` [B, S] (right-padded; row b holds ``lens[b]`` real tokens) through the model, fill
        ``cache`` and set its lengths to ``lens``. Returns the logits of every row's last real token [B, V], or with
        ``all_logits`` of every position [B, S, V]. Attention is causal, so a pad token never reaches a real one, and
        later appends overwrite the pad positions."""
        B, S = ids.shape
        c = self.c
        lens_host = torch.as_tensor(lens, dtype=torch.int32).reshape(-1).cpu()
        if B != cache.batch or lens_host.numel() != B:
            raise ValueError("prefill: %d prompts and %d lengths for a cache of %d rows" % (B, lens_host.numel(),
                                                                                        cache.batch))
        if S > cache.max_len or S > c.max_position:
            raise ValueError("prefill: %d prompt tokens exceed the cache's max_len = %d or the model's max_position = "
                             "%d" % (S, cache.max_len, c.max_position))
        if int(lens_host.min()) < 1 or int(lens_host.max()) > S:
            raise ValueError("prefill: every prompt length must be in [1, S = %d]" % S)
        dev = ids.device
        pos = torch.arange(S, device=dev, dtype=torch.int32).repeat(B)
        cache.set_lens(torch.zeros(B, dtype=torch.int32))
        x = K.embedding_sum([(ids, self.embed)], S, cache.dtype).reshape(B * S, c.hidden)
        res = None
        for i, layer in enumerate(self.layers):
            x, res = layer.prefill(x, res, B, S, pos, self.table, cache.k[i], cache.v[i], cache.lens, cache.lens_host)
        cache.set_lens(lens_host)
        if not all_logits:  # the LM head reads B rows, not B * S
            last = torch.arange(B, device=dev) * S + (cache.lens.long() - 1)
            x, res = x[last].contiguous(), res[last].contiguous()
        hn, _ = K.rms_norm(x, self.norm, c.eps, residual=res)
        logits = K.linear(hn, self.lm_head)
        return logits.reshape(B, S, c.vocab_size) if all_logits else logits

    @torch.no_grad()
    def decode_step(self, tokens, cache: KVCache):
        """Append one token per row (``tokens`` int64 [B]) and return the next-token logits [B, V]."""
        c = self.c
        B = tokens.shape[0]
        if B != cache.batch:
            raise ValueError("decode_step: %d tokens for a cache of %d rows" % (B, cache.batch))
        longest = int(cache.lens_host.max())
        if int(cache.lens_host.min()) < 1:
            raise ValueError("decode_step: a row of the cache is empty (run prefill first)")
        if longest + 1 > cache.max_len or longest + 1 > c.max_position:
            raise ValueError("decode_step: a row of %d tokens would pass the cache's max_len = %d or the model's "
                             "max_position = %d" % (longest + 1, cache.max_len, c.max_position))
        new_host = cache.lens_host + 1
        new_lens = cache.lens + 1
        x = K.embedding_sum([(tokens.reshape(B, 1), self.embed)], 1, cache.dtype).reshape(B, c.hidden)
        res = None
        for i, layer in enumerate(self.layers):
            x, res = layer.decode(x, res, cache.lens, self.table, cache.k[i], cache.v[i], cache.lens, cache.lens_host,
                                  new_lens, new_host)
        cache.lens, cache.lens_host = new_lens, new_host
        hn, _ = K.rms_norm(x, self.norm, c.eps, residual=res)
        return KD.linear(hn, self.lm_head)

    @torch.no_grad()
    def generate(self, prompts, max_new_tokens: int, temperature: float = 0.0, top_k: int = 40, seed: int = 0,
                 eos_id=None, max_len=None, dtype=None):
        """Continue ``prompts`` (a list of token-id lists, one batch row each) by up to ``max_new_tokens`` tokens.
        Returns a list of token lists. Generated token t of row b is ``ops.sampling.sample`` at (seed, step = t,
        row = b). After ``eos_id`` a row emits ``eos_id``; the loop ends when every row has. ``self.last_generate``
        holds the timings of the call (``prefill_ms``, ``decode_tokens_per_sec``, ``decode_steps``)."""
        c = self.c
        B = len(prompts)
        lens = [len(p) for p in prompts]
        if B < 1 or min(lens) < 1:
            raise ValueError("generate: needs at least one prompt, each of at least one token")
        if max_new_tokens < 1:
            raise ValueError("generate: max_new_tokens must be positive")
        S = max(lens)
        max_len = int(max_len or S + max_new_tokens)
        if S + max_new_tokens > max_len or S + max_new_tokens > c.max_position:
            raise ValueError("generate: prompt (%d) plus max_new_tokens (%d) pass max_len = %d or the model's "
                             "max_position = %d" % (S, max_new_tokens, max_len, c.max_position))
        dev = self.embed.master.device
        if dtype is None:
            dtype = torch.bfloat16 if dev.type == "cuda" else torch.float32
        ids = torch.zeros(B, S, dtype=torch.int64)
        for b, p in enumerate(prompts):
            ids[b, : lens[b]] = torch.as_tensor(p, dtype=torch.int64)
        cache = KVCache(c, B, max_len, dev, dtype)
        sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
        t0 = time.perf_counter()
        logits = self.prefill(ids.to(dev), lens, cache)
        sync()
        t1 = time.perf_counter()
        out = [[] for _ in range(B)]
        done = torch.zeros(B, dtype=torch.bool)
        steps = 0
        for t in range(max_new_tokens):
            tok = sampling.sample(logits, temperature, top_k, seed, t).cpu()
            if eos_id is not None:
                tok = torch.where(done, torch.full_like(tok, eos_id), tok)
                done = done | (tok == eos_id)
            for b in range(B):
                out[b].append(int(tok[b]))
            if t + 1 == max_new_tokens or bool(done.all()):
                break
            logits = self.decode_step(tok.to(dev), cache)
            steps += 1
        sync()
        t2 = time.perf_counter()
        self.last_generate = {"prefill_ms": (t1 - t0) * 1e3, "decode_steps": steps,
                              "decode_tokens_per_sec": B * steps / (t2 - t1) if steps and t2 > t1 else 0.0}
        return out


def synthetic_batch(c: LlamaConfig, batch: int, seq: int, device, generator=None):
    ids = torch.randint(0, c.vocab_size, (batch, seq + 1), device=device, generator=generator)
    return ids[:, :-1].contiguous(), ids[:, 1:].contiguous()
