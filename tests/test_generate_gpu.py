"""Generation on the GPU (K16): the skinny-M GEMM, the cache append and the split-key decode attention of
``csrc/kernels/decode.hip`` against their torch definitions, then ``llama_tiny``'s prefill / decode_step / generate
against the fp32 CPU model."""
import math

import pytest
import torch

from k8s_amd.ops import decode as KD
from k8s_amd.ops import reference as ref
from k8s_amd.ops.attention import attention_reference

pytestmark = pytest.mark.gpu


def _close(a, b, tol, what):  # tests/test_attention_gpu.py's measure
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    print("%s: max err %g (scale %g, bound %g)" % (what, err, scale, tol * max(1.0, scale)))
    assert err <= tol * max(1.0, scale), "%s: max err %g (scale %g)" % (what, err, scale)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ linear_skinny
SKINNY = [(1, 512, 256), (5, 528, 768), (16, 512, 14336), (3, 48, 4096)]


@pytest.mark.parametrize("M,N,K", SKINNY)
def test_linear_skinny_per_element_vs_fp64(cuda, M, N, K):
    """|y - fp64| <= 2^-8 |y| + K 2^-24 sum_k |x_k w_k|: one bf16 rounding plus the worst-case fp32 accumulation."""
    from k8s_amd.ops._ext import load

    g = torch.Generator().manual_seed(M * 1000 + N + K)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    kc, nsplit = load().linear_skinny_plan(N, K)
    y = KD.linear_skinny(x.to(cuda), w.to(cuda))
    y2 = KD.linear_skinny(x.to(cuda), w.to(cuda))
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    exact = x.double() @ w.double().t()
    mag = x.double().abs() @ w.double().abs().t()
    bound = 2.0 ** -8 * exact.abs() + K * 2.0 ** -24 * mag
    err = (y.cpu().double() - exact).abs()
    print("skinny %dx%dx%d: k chunk %d x %d, worst err / bound %.4f" % (M, N, K, kc, nsplit,
                                                                         float((err / bound.clamp_min(1e-30)).max())))
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-30)).max())
    assert torch.equal(_bits(y), _bits(y2))  # bitwise repeatable
    assert float(y.float().abs().max()) > 0


def test_linear_skinny_covers_one_chunk_and_many(cuda):
    from k8s_amd.ops._ext import load

    splits = [load().linear_skinny_plan(N, K)[1] for _, N, K in SKINNY]
    assert min(splits) == 1 and max(splits) > 1, splits


@pytest.mark.parametrize("N,K", [(512, 256), (512, 14336), (48, 4096)])
def test_linear_skinny_row_does_not_depend_on_m(cuda, N, K):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(16, K, generator=g).bfloat16().to(cuda)
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16().to(cuda)
    y16 = KD.linear_skinny(x, w)
    y1 = KD.linear_skinny(x[:1].contiguous(), w)
    y7 = KD.linear_skinny(x[:7].contiguous(), w)
    assert torch.equal(_bits(y1[0]), _bits(y16[0]))
    assert torch.equal(_bits(y7), _bits(y16[:7]))


def test_linear_skinny_contract_and_fallback(cuda):
    from k8s_amd.models.registry import build
    from k8s_amd.ops._ext import load

    C = load()
    before = C.decode_launches()
    x = torch.randn(17, 256, device=cuda).bfloat16()
    w = torch.randn(512, 256, device=cuda).bfloat16()
    for bad_x, bad_w in ((x, w),                                  # M = 17
                         (x[:4, :96].contiguous(), w[:, :96].contiguous()),   # K % 64
                         (x[:4].contiguous(), w[:40].contiguous()),           # N % 16
                         (x[:4].contiguous(), w[:, :128].contiguous()),       # K mismatch
                         (x[:4].float(), w)):
        with pytest.raises(RuntimeError):
            C.linear_skinny(bad_x, bad_w)
    assert C.decode_launches() == before
    # ops.decode.linear: outside the contract the product goes through ops.nn.linear and is counted
    m = build("llama_tiny", cuda, batch=1, seed=1).model
    KD.reset_counters()
    pw = m.layers[0].qkv
    x17 = torch.randn(17, pw.shape[1], device=cuda).bfloat16()
    with torch.no_grad():
        y = KD.linear(x17, pw)
        assert (KD.LINEAR_SKINNY, KD.LINEAR_OTHER) == (0, 1)
        y4 = KD.linear(x17[:4].contiguous(), pw)
    assert (KD.LINEAR_SKINNY, KD.LINEAR_OTHER) == (1, 1)
    _close(y[:4], y4, 2e-2, "fallback vs skinny")
    KD.reset_counters()


# ------------------------------------------------------------------------------------------------ kv_append
@pytest.mark.parametrize("S", [1, 40])
def test_kv_append_is_the_index_copy(cuda, S):
    B, Hq, Hkv, D, Smax = 3, 4, 2, 64, 96
    g = torch.Generator().manual_seed(S)
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, generator=g).bfloat16()
    start = torch.tensor([0, 56, 17], dtype=torch.int32)
    sent_k = torch.full((B, Hkv, Smax, D), 7.0).bfloat16()
    sent_v = torch.full((B, Hkv, Smax, D), -3.0).bfloat16()
    want_k, want_v = sent_k.clone(), sent_v.clone()
    ref.kv_append(qkv, want_k, want_v, start, S, Hq)
    # the definition moved what it should and nothing else
    for b in range(B):
        lo = int(start[b])
        assert bool((want_k[b, :, :lo] == 7.0).all()) and bool((want_k[b, :, lo + S:] == 7.0).all())
        assert torch.equal(want_v[b, 1, lo:lo + S], qkv.view(B, S, -1, D)[b, :, Hq + Hkv + 1])
    got_k, got_v = sent_k.to(cuda), sent_v.to(cuda)
    KD.kv_append(qkv.to(cuda), got_k, got_v, start.to(cuda), start, S, Hq)
    assert torch.equal(_bits(got_k.cpu()), _bits(want_k)) and torch.equal(_bits(got_v.cpu()), _bits(want_v))


def test_kv_append_rejects_before_any_launch(cuda):
    from k8s_amd.ops._ext import load

    C = load()
    B, Hq, Hkv, D, Smax, S = 3, 4, 2, 64, 96, 40
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, device=cuda).bfloat16()
    ck = torch.full((B, Hkv, Smax, D), 7.0, device=cuda).bfloat16()
    cv = torch.full((B, Hkv, Smax, D), -3.0, device=cuda).bfloat16()
    before = C.decode_launches()
    for bad in ([0, 57, 17], [0, -1, 17]):
        start = torch.tensor(bad, dtype=torch.int32)
        with pytest.raises(RuntimeError):
            KD.kv_append(qkv, ck, cv, start.to(cuda), start, S, Hq)
    ok = torch.tensor([0, 1, 2], dtype=torch.int32)
    with pytest.raises(RuntimeError):  # a mirror on the device, a cache of another shape
        KD.kv_append(qkv, ck, cv, ok.to(cuda), ok.to(cuda), S, Hq)
    with pytest.raises(RuntimeError):
        KD.kv_append(qkv, ck, cv[:, :, :50].contiguous(), ok.to(cuda), ok, S, Hq)
    assert C.decode_launches() == before
    assert bool((ck == 7.0).all()) and bool((cv == -3.0).all())


# ------------------------------------------------------------------------------------------------ decode_attention
LENS = [[1, 63, 64], [65, 257, 320], [320, 1, 257], [64, 65, 63]]
ATTN = [(D, Hq, Hkv) for D in (64, 128) for Hq, Hkv in ((4, 2), (8, 8), (32, 8), (16, 1))]  # groups of 2, 1, 4 and 16


def _attn_inputs(D, Hq, Hkv, lens, B=3, Smax=320):
    g = torch.Generator().manual_seed(D + Hq + sum(lens))
    q = torch.randn(B, Hq, D, generator=g).bfloat16()
    k = torch.randn(B, Hkv, Smax, D, generator=g).bfloat16()
    v = torch.randn(B, Hkv, Smax, D, generator=g).bfloat16()
    return q, k, v, torch.tensor(lens, dtype=torch.int32)


@pytest.mark.parametrize("D,Hq,Hkv", ATTN)
def test_decode_attention_vs_reference(cuda, D, Hq, Hkv):
    scale = 1.0 / math.sqrt(D)
    for lens in LENS:
        q, k, v, ln = _attn_inputs(D, Hq, Hkv, lens)
        want = attention_reference(q[:, None].float(), k.permute(0, 2, 1, 3).float(), v.permute(0, 2, 1, 3).float(),
                                   False, ln, scale).reshape(3, Hq * D)
        qc, kc, vc = q.to(cuda), k.to(cuda), v.to(cuda)
        got = KD.decode_attention(qc, kc, vc, ln.to(cuda), ln, scale)
        assert got.shape == (3, Hq * D) and got.dtype == torch.bfloat16
        _close(got.cpu(), want, 2e-2, "decode attention D %d heads %d/%d lens %s" % (D, Hq, Hkv, lens))
        # two runs, bitwise
        assert torch.equal(_bits(got), _bits(KD.decode_attention(qc, kc, vc, ln.to(cuda), ln, scale)))
        # NaN past lens changes nothing
        kn, vn = k.clone(), v.clone()
        for b in range(3):
            kn[b, :, lens[b]:] = float("nan")
            vn[b, :, lens[b]:] = float("nan")
        nan = KD.decode_attention(qc, kn.to(cuda), vn.to(cuda), ln.to(cuda), ln, scale)
        assert torch.equal(_bits(got), _bits(nan))
        # every sequence alone gives the bits it gives in the batch (q as a strided view of a wider row, too)
        for b in range(3):
            wide = torch.zeros(1, Hq * D + 64, device=cuda, dtype=torch.bfloat16)
            wide[:, : Hq * D] = qc[b].reshape(1, -1)
            one = KD.decode_attention(wide[:, : Hq * D].view(1, Hq, D), kc[b:b + 1].contiguous(),
                                      vc[b:b + 1].contiguous(), ln[b:b + 1].to(cuda), ln[b:b + 1].contiguous(), scale)
            assert torch.equal(_bits(one[0]), _bits(got[b])), (lens, b)


def test_decode_attention_rejects_before_any_launch(cuda):
    from k8s_amd.ops._ext import load

    C = load()
    q, k, v, ln = _attn_inputs(64, 4, 2, [1, 63, 64])
    qc, kc, vc = q.to(cuda), k.to(cuda), v.to(cuda)
    before = C.decode_launches()
    for bad in ([0, 5, 5], [5, 321, 5]):
        t = torch.tensor(bad, dtype=torch.int32)
        with pytest.raises(RuntimeError):
            KD.decode_attention(qc, kc, vc, t.to(cuda), t, 0.125)
    with pytest.raises(RuntimeError):  # a group of 17 queries
        KD.decode_attention(torch.zeros(3, 34, 64, device=cuda).bfloat16(), kc, vc, ln.to(cuda), ln, 0.125)
    with pytest.raises(RuntimeError):  # head dim 32
        KD.decode_attention(qc[..., :32].contiguous(), kc[..., :32].contiguous(), vc[..., :32].contiguous(),
                            ln.to(cuda), ln, 0.125)
    assert C.decode_launches() == before


# ------------------------------------------------------------------------------------------------ the model
PROMPT_LENS = (5, 9, 16)
STEPS = 12


@pytest.fixture(scope="module")
def tiny(cuda):
    """llama_tiny on the GPU (bf16) and on the CPU (fp32) with the same weights, and 3 token rows of 16 + 12 ids."""
    from k8s_amd.models.registry import build

    g = build("llama_tiny", cuda, batch=3, seed=3).model
    c = build("llama_tiny", "cpu", batch=3, seed=3).model
    ids = torch.randint(0, 512, (3, max(PROMPT_LENS) + STEPS), generator=torch.Generator().manual_seed(21))
    return g, c, ids


def _teacher_forced(model, ids, dev, dtype, rows=(0, 1, 2)):
    """(prefill logits, [decode logits per step]) feeding the true next ids after prompts of PROMPT_LENS."""
    from k8s_amd.models.llama import KVCache

    rows = list(rows)
    lens = [PROMPT_LENS[r] for r in rows]
    S = max(lens)
    prompt = torch.zeros(len(rows), S, dtype=torch.int64)
    for i, r in enumerate(rows):
        prompt[i, : lens[i]] = ids[r, : lens[i]]
    cache = KVCache(model.c, len(rows), max(PROMPT_LENS) + STEPS, dev, dtype)
    first = model.prefill(prompt.to(dev), lens, cache)
    out = []
    for t in range(STEPS):
        tok = torch.stack([ids[r, lens[i] + t] for i, r in enumerate(rows)])
        out.append(model.decode_step(tok.to(dev), cache))
    return first, out


def _longer_prefix(model, ids, dev, dtype, t):
    """Last-row prefill logits over the prefixes of PROMPT_LENS[b] + t + 1 tokens."""
    from k8s_amd.models.llama import KVCache

    lens = [n + t + 1 for n in PROMPT_LENS]
    S = max(lens)
    prompt = torch.zeros(3, S, dtype=torch.int64)
    for b in range(3):
        prompt[b, : lens[b]] = ids[b, : lens[b]]
    return model.prefill(prompt.to(dev), lens, KVCache(model.c, 3, S, dev, dtype))


def test_llama_tiny_decode_matches_prefill_and_cpu_fp32(cuda, tiny):
    from k8s_amd.ops import gemm

    g, c, ids = tiny
    gemm.FALLBACKS.clear()
    KD.reset_counters()
    first_g, dec_g = _teacher_forced(g, ids, cuda, torch.bfloat16)
    first_c, dec_c = _teacher_forced(c, ids, "cpu", torch.float32)
    assert KD.LINEAR_OTHER == 0 and KD.LINEAR_SKINNY == STEPS * (4 * g.c.layers + 1)
    assert gemm.FALLBACKS == {}, gemm.FALLBACKS
    # against the fp32 CPU model: tests/test_doc_mask_gpu.py's tolerance for llama_tiny (3e-2 of max(1, scale))
    _close(first_g.cpu(), first_c, 3e-2, "prefill logits vs cpu fp32")
    for t in range(STEPS):
        _close(dec_g[t].cpu(), dec_c[t], 3e-2, "decode step %d logits vs cpu fp32" % t)
    # the teacher-forced property in bf16: a decode step's logits are the one-token-longer prefill's, to the same bound
    for t in (0, 5, STEPS - 1):
        _close(dec_g[t], _longer_prefix(g, ids, cuda, torch.bfloat16, t), 3e-2, "decode step %d vs prefill" % t)
    # row 1 alone: the decode kernels give a row the bits it has in the batch; the prefill's GEMMs tile M, so compare
    # within the bound
    _, alone = _teacher_forced(g, ids, cuda, torch.bfloat16, rows=(1,))
    for t in range(STEPS):
        _close(alone[t][0], dec_g[t][1], 3e-2, "row 1 alone, step %d" % t)


def test_llama_tiny_generate_is_repeatable(cuda, tiny):
    from k8s_amd.ops import gemm

    g, _, ids = tiny
    prompts = [ids[b, : PROMPT_LENS[b]].tolist() for b in range(3)]
    gemm.FALLBACKS.clear()
    KD.reset_counters()
    for temperature in (0.0, 0.8):
        a = g.generate(prompts, 10, temperature, 8, seed=4)
        b = g.generate(prompts, 10, temperature, 8, seed=4)
        assert a == b and all(len(r) == 10 and all(0 <= t < 512 for t in r) for r in a)
    assert gemm.FALLBACKS == {} and KD.LINEAR_OTHER == 0 and KD.LINEAR_SKINNY > 0
