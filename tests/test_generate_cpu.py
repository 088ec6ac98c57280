"""Generation on the CPU in fp32 (``llama_tiny``): prefill against the training forward, teacher-forced decode against
prefill, the kv_append / decode_attention definitions, sampling, and ``python -m k8s_amd.generate``."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from k8s_amd.models.llama import KVCache
from k8s_amd.ops import decode as KD
from k8s_amd.ops import nn as K
from k8s_amd.ops import reference as ref
from k8s_amd.ops import sampling
from k8s_amd.ops.attention import attention_reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT_LENS = (5, 9, 16)
STEPS = 12


@pytest.fixture(scope="module")
def tiny():
    from k8s_amd.models.registry import build

    model = build("llama_tiny", "cpu", batch=3, seed=3).model
    ids = torch.randint(0, 512, (3, max(PROMPT_LENS) + STEPS + 1), generator=torch.Generator().manual_seed(21))
    return model, ids


def _prompt(ids, lens):
    p = torch.zeros(len(lens), max(lens), dtype=torch.int64)
    for b, n in enumerate(lens):
        p[b, :n] = ids[b, :n]
    return p


# ------------------------------------------------------------------------------------------------ the model
def test_prefill_is_the_training_forward(tiny):
    model, ids = tiny
    B, S = 3, 24
    x, labels = ids[:, :S].contiguous(), ids[:, 1:S + 1].contiguous()
    with torch.no_grad():
        want = float(model(x, labels, dtype=torch.float32))
    logits = model.prefill(x, [S] * B, KVCache(model.c, B, S, "cpu", torch.float32), all_logits=True)
    assert logits.shape == (B, S, 512)
    got = float(K.cross_entropy(logits.reshape(B * S, -1), labels.reshape(-1)))
    assert abs(got - want) <= 1e-4 * abs(want), (got, want)
    # without all_logits: the rows at lens - 1 only
    last = model.prefill(x, [S, 7, 1], KVCache(model.c, B, S, "cpu", torch.float32))
    for b, n in enumerate((S, 7, 1)):
        err = float((last[b] - logits[b, n - 1]).abs().max())
        assert err <= 1e-4 * float(logits[b, n - 1].abs().max()), (b, err)


def test_teacher_forced_decode_is_the_longer_prefill(tiny):
    model, ids = tiny
    cache = KVCache(model.c, 3, max(PROMPT_LENS) + STEPS, "cpu", torch.float32)
    model.prefill(_prompt(ids, PROMPT_LENS), PROMPT_LENS, cache)
    alone = KVCache(model.c, 1, PROMPT_LENS[1] + STEPS, "cpu", torch.float32)
    model.prefill(ids[1:2, : PROMPT_LENS[1]], [PROMPT_LENS[1]], alone)
    for t in range(STEPS):
        tok = torch.stack([ids[b, PROMPT_LENS[b] + t] for b in range(3)])
        got = model.decode_step(tok, cache)
        assert cache.lens_host.tolist() == [n + t + 1 for n in PROMPT_LENS] == cache.lens.tolist()
        lens = [n + t + 1 for n in PROMPT_LENS]
        want = model.prefill(_prompt(ids, lens), lens, KVCache(model.c, 3, max(lens), "cpu", torch.float32))
        one = model.decode_step(tok[1:2], alone)
        for b in range(3):
            bound = 1e-4 * float(want[b].abs().max())
            assert float((got[b] - want[b]).abs().max()) <= bound, (t, b)
        assert float((one[0] - got[1]).abs().max()) <= 1e-4 * float(got[1].abs().max()), t


def test_decode_step_and_prefill_refuse_what_does_not_fit(tiny):
    model, ids = tiny
    cache = KVCache(model.c, 1, 6, "cpu", torch.float32)
    with pytest.raises(ValueError):
        model.decode_step(ids[:1, 0], cache)  # nothing prefilled
    model.prefill(ids[:1, :5], [5], cache)
    model.decode_step(ids[:1, 5], cache)
    with pytest.raises(ValueError):
        model.decode_step(ids[:1, 6], cache)  # a seventh token in a cache of six
    with pytest.raises(ValueError):
        model.prefill(ids[:1, :7], [7], cache)
    with pytest.raises(ValueError):
        model.prefill(ids[:1, :5], [0], cache)
    with pytest.raises(ValueError):
        model.generate([[1, 2, 3]], 300)  # past llama_tiny's max_position = 256


# ------------------------------------------------------------------------------------------------ the ops' definitions
def test_kv_append_is_an_index_copy():
    B, S, Hq, Hkv, D, Smax = 3, 5, 4, 2, 8, 12
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D)
    ck, cv = torch.full((B, Hkv, Smax, D), 7.0), torch.full((B, Hkv, Smax, D), -3.0)
    start = torch.tensor([0, 7, 3], dtype=torch.int32)
    KD.kv_append(qkv, ck, cv, start, start, S, Hq)
    g = qkv.view(B, S, Hq + 2 * Hkv, D)
    for b in range(B):
        lo = int(start[b])
        for h in range(Hkv):
            assert torch.equal(ck[b, h, lo:lo + S], g[b, :, Hq + h]) and torch.equal(cv[b, h, lo:lo + S],
                                                                                      g[b, :, Hq + Hkv + h])
        assert bool((ck[b, :, :lo] == 7).all()) and bool((ck[b, :, lo + S:] == 7).all())
        assert bool((cv[b, :, :lo] == -3).all()) and bool((cv[b, :, lo + S:] == -3).all())
    before = ck.clone()
    for bad in ([0, 8, 3], [-1, 0, 0]):
        with pytest.raises(RuntimeError):
            KD.kv_append(qkv, ck, cv, torch.tensor(bad, dtype=torch.int32), torch.tensor(bad, dtype=torch.int32), S, Hq)
    assert torch.equal(ck, before)


@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (8, 8, 16), (32, 8, 128)])
def test_decode_attention_is_the_reference_at_sq_1(Hq, Hkv, D):
    B, Smax = 3, 70
    g = torch.Generator().manual_seed(Hq + D)
    q = torch.randn(B, Hq, D, generator=g)
    k, v = torch.randn(B, Hkv, Smax, D, generator=g), torch.randn(B, Hkv, Smax, D, generator=g)
    lens = torch.tensor([1, 33, 70], dtype=torch.int32)
    scale = 1.0 / math.sqrt(D)
    want = attention_reference(q[:, None], k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3), False, lens, scale)
    got = KD.decode_attention(q, k, v, lens, lens, scale)
    assert got.shape == (B, Hq * D)
    assert float((got - want.reshape(B, Hq * D)).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    kn, vn = k.clone(), v.clone()
    for b in range(B):
        kn[b, :, int(lens[b]):] = float("nan")
        vn[b, :, int(lens[b]):] = float("nan")
    assert torch.equal(KD.decode_attention(q, kn, vn, lens, lens, scale), got)  # bitwise
    with pytest.raises(RuntimeError):
        bad = torch.tensor([1, 0, 70], dtype=torch.int32)
        KD.decode_attention(q, k, v, bad, bad, scale)


def test_counter_bits_is_what_dropout_keep_compares():
    state = (1234567, 9)
    rows, cols = torch.arange(5), torch.arange(7)
    bits = ref.counter_bits(state, 3, rows, cols)
    assert bits.shape == (5, 7) and int(bits.min()) >= 0 and int(bits.max()) < 2 ** 32
    for p in (0.1, 0.5, 0.9):
        thr, _ = ref.drop_params(p)
        assert torch.equal(ref.dropout_keep(state, 3, rows, cols, p), bits >= thr)


# ------------------------------------------------------------------------------------------------ sampling
def test_greedy_ties_go_to_the_lower_index():
    logits = torch.tensor([[0.0, 3.0, 3.0, 1.0], [2.0, 2.0, 2.0, 2.0], [-1.0, -5.0, -1.0, -0.5]])
    assert sampling.sample(logits, 0.0, 40, 0, 0).tolist() == [1, 0, 3]
    assert sampling.sample(logits.bfloat16(), 0.0, 40, 0, 0).tolist() == [1, 0, 3]
    vals, cols = sampling.candidates(torch.tensor([[1.0, 5.0, 5.0, 0.0, 5.0]]), 4)
    assert cols.tolist() == [[1, 2, 4, 0]]


def test_sampled_tokens_have_rank_below_top_k_and_repeat():
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(6, 300, generator=g)
    logits[:, 17] = logits[:, 211]  # ties
    labels = None
    for top_k in (1, 5, 64):
        a = [sampling.sample(logits, 0.7, top_k, 11, t) for t in range(64)]
        b = [sampling.sample(logits, 0.7, top_k, 11, t) for t in range(64)]
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        for tok in a:
            _, rank = ref.xent_eval(logits, tok)
            assert int(rank.max()) < top_k
        if top_k == 1:
            assert all(torch.equal(t, sampling.greedy(logits)) for t in a)
    a = torch.stack([sampling.sample(logits, 1.0, 8, 11, t) for t in range(64)])
    assert not torch.equal(a[0].expand_as(a), a)  # another step, another draw somewhere in 64
    other_seed = torch.stack([sampling.sample(logits, 1.0, 8, 12, t) for t in range(64)])
    assert not torch.equal(a, other_seed)
    # a row's draw depends on its index alone
    sub = sampling.sample(logits[2:4], 1.0, 8, 11, 5, rows=torch.tensor([2, 3]))
    assert torch.equal(sub, sampling.sample(logits, 1.0, 8, 11, 5)[2:4])
    for bad in (0, 65):
        with pytest.raises(ValueError):
            sampling.sample(logits, 1.0, bad, 0, 0)


def test_sampling_follows_the_cdf():
    """4,096 draws, top_k 8, T = 1: every token's fp64 CDF interval over the rank-ordered candidates, widened by 1e-3
    of the total, holds u * total; every candidate is drawn. The narrowest interval is 0.02 of the total or more."""
    top_k, V = 8, 32
    probs = torch.tensor([0.30, 0.22, 0.16, 0.11, 0.08, 0.06, 0.04, 0.03], dtype=torch.float64)
    logits = torch.full((V,), -20.0)
    where = torch.tensor([3, 30, 11, 0, 7, 19, 25, 14])
    logits[where] = probs.log().float()
    cand = logits[where].double().exp()
    total = float(cand.sum())
    edges = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(cand, 0)])
    assert float((cand / total).min()) >= 0.02
    rows = 16
    seen = set()
    for step in range(4096 // rows):
        tok = sampling.sample(logits.expand(rows, V), 1.0, top_k, 77, step)
        u = sampling.uniform(77, step, torch.arange(rows))
        for b in range(rows):
            j = int((where == int(tok[b])).nonzero()[0])
            seen.add(j)
            x = float(u[b]) * total
            assert float(edges[j]) - 1e-3 * total <= x <= float(edges[j + 1]) + 1e-3 * total, (step, b, j, x)
    assert seen == set(range(top_k))


def test_eos_freezes_a_row(tiny):
    model, ids = tiny
    prompts = [ids[b, : PROMPT_LENS[b]].tolist() for b in range(3)]
    free = model.generate(prompts, 8, 0.0)
    eos = free[1][2]  # row 1's third token becomes the end-of-sequence id
    out = model.generate(prompts, 8, 0.0, eos_id=eos)
    for b in range(3):
        n = free[b].index(eos) + 1 if eos in free[b] else 8
        assert out[b][:n] == free[b][:n] and all(t == eos for t in out[b][n:]), (b, free[b], out[b])
    assert out[1][2:] == [eos] * (len(out[1]) - 2)
    same = model.generate(prompts, 8, 0.9, 8, seed=3)
    assert same == model.generate(prompts, 8, 0.9, 8, seed=3)
    # every row finished: the loop stops early
    early = model.generate([prompts[1]], 8, 0.0, eos_id=eos)
    assert early == [free[1][:3]]


# ------------------------------------------------------------------------------------------------ the command
def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""
    env["OMP_NUM_THREADS"] = "2"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        env.pop(k, None)
    return env


def _run(module, args, timeout=240):
    p = subprocess.run([sys.executable, "-m", module, "--device", "cpu"] + args, env=_env(), capture_output=True,
                       text=True, timeout=timeout)
    return p, [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]


ERRORS = [
    (["--model", "llama_tiny", "--ckpt-dir", "EMPTY", "--prompt-ids", "1,2"], "checkpoint"),
    (["--model", "llama_tiny", "--prompt-ids", "1,2"], "checkpoint"),
    (["--model", "bert_tiny", "--random-init", "--prompt-ids", "1,2"], "Llama"),
    (["--model", "llama_tiny", "--random-init", "--prompt-ids", "1,512"], "vocabulary"),
    (["--model", "llama_tiny", "--random-init", "--prompt-ids", "1,-2"], "vocabulary"),
    (["--model", "llama_tiny", "--random-init"] + ["--prompt-ids", "1"] * 17, "rows"),
    (["--model", "llama_tiny", "--random-init", "--prompt-ids", "1", "--temperature", "0.5", "--top-k", "65"], "--top-k"),
    (["--model", "llama_tiny", "--random-init", "--prompt-ids", "1", "--temperature", "0.5", "--top-k", "0"], "--top-k"),
    (["--model", "llama_tiny", "--random-init", "--prompt-ids", "1,2,3", "--max-new-tokens", "6", "--max-len", "8"],
     "--max-len"),
    (["--model", "llama_tiny", "--random-init", "--prompt-ids", "1,2,3", "--max-new-tokens", "254"], "max_position"),
]


@pytest.mark.parametrize("args,word", ERRORS)
def test_generate_configuration_error_exits_1_with_one_sentence(tmp_path, args, word):
    p, events = _run("k8s_amd.generate", [str(tmp_path) if a == "EMPTY" else a for a in args])
    assert p.returncode == 1, p.stdout[-1500:] + p.stderr[-1500:]
    errors = [line for line in p.stderr.splitlines() if line.startswith("error: ")]
    assert len(errors) == 1 and word in errors[0] and "Traceback" not in p.stderr, p.stderr[-1500:]
    assert not events  # before the model is built


def test_generate_command_prints_what_generate_gives_on_the_checkpoint(tmp_path):
    from k8s_amd.models.registry import build
    from k8s_amd.utils import checkpoint as ckpt

    ck = str(tmp_path / "ckpt")
    p, _ = _run("k8s_amd.trainer", ["--model", "llama_tiny", "--batch", "2", "--steps", "3", "--ckpt-dir", ck])
    assert p.returncode == 0, p.stderr[-1500:]
    args = ["--model", "llama_tiny", "--ckpt-dir", ck, "--prompt-ids", "5,6,7,8,9", "--prompt-ids", "100,3",
            "--max-new-tokens", "6"]
    for extra in ([], ["--temperature", "0.7", "--top-k", "5", "--seed", "9"]):
        p, ev = _run("k8s_amd.generate", args + extra)
        assert p.returncode == 0, p.stderr[-1500:]
        rows = [e for e in ev if e["event"] == "generate"]
        done = [e for e in ev if e["event"] == "done"]
        assert [e["row"] for e in rows] == [0, 1] and [e["prompt_len"] for e in rows] == [5, 2]
        assert len(done) == 1 and done[0]["gemm_fallbacks"] == {} and done[0]["linear_off_skinny"] == 0
        assert done[0]["prefill_ms"] > 0 and done[0]["decode_tokens_per_sec"] > 0
        w = build("llama_tiny", "cpu", batch=2, seed=5)  # another initialisation: the tokens come from the checkpoint
        _, tensors, _ = ckpt.load(ckpt.latest_checkpoint(ck))
        w.store.load_state_dict({k[len("params/"):]: v for k, v in tensors.items() if k.startswith("params/")})
        w.store.refresh_lowp()
        want = w.model.generate([[5, 6, 7, 8, 9], [100, 3]], 6, 0.7 if extra else 0.0, 5 if extra else 40,
                                seed=9 if extra else 0)
        assert [e["tokens"] for e in rows] == want


def test_generate_example_manifest_validates():
    from k8s_amd import _operator as op
    from k8s_amd.fakeapi.cluster import load_manifests

    (d,) = load_manifests(os.path.join(REPO, "examples", "tf_job_llama_generate.yaml"))
    spec, err = op.set_defaults(json.dumps(d["spec"]))
    assert err == "" and op.validate(spec) == ""
    (rs,) = json.loads(spec)["replicaSpecs"]
    assert rs["replicas"] == 1
    c = rs["template"]["spec"]["containers"][0]
    assert c["command"] == ["python", "-m", "k8s_amd.generate"] and "--ckpt-dir" in c["args"]
    (train,) = load_manifests(os.path.join(REPO, "examples", "tf_job_llama_tokens_docmask.yaml"))
    targs = train["spec"]["replicaSpecs"][0]["template"]["spec"]["containers"][0]["args"]
    assert c["args"][c["args"].index("--ckpt-dir") + 1] == targs[targs.index("--ckpt-dir") + 1]
    assert c["args"][c["args"].index("--model") + 1] == targs[targs.index("--model") + 1]
