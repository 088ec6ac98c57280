"""Gradient accumulation, CPU tier: the oracles against the definition, large-batch equivalence on llama_tiny, two
gloo ranks under both data-parallel strategies, the trainer end to end (``--accum-steps``), and the example manifest."""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from k8s_amd.fakeapi.server import free_port
from k8s_amd.ops import reference as ref
from k8s_amd.ops.optim import FusedLAMB
from k8s_amd.parallel.accum import GradAccumulator
from k8s_amd.parallel.ddp import GradReducer
from k8s_amd.parallel.flat import ALIGN, ParamStore, init_normal
from k8s_amd.parallel.ps import ShardedParameterService

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- oracles
@pytest.mark.parametrize("total,lo,hi", [(64, 0, 64), (192, 64, 192), (192, 64, 128), (320, 128, 128)])
def test_oracles_follow_the_definition(total, lo, hi):
    gen = torch.Generator().manual_seed(total + lo)
    g0, a0 = torch.randn(total, generator=gen), torch.randn(total, generator=gen)
    for first in (True, False):
        acc = torch.full((total,), float("nan")) if first else a0.clone()
        keep = acc.clone()
        ref.grad_accumulate(acc, g0, lo, hi, first)
        for i in range(total):
            if lo <= i < hi:
                assert acc[i].item() == (g0[i].item() if first else (a0[i] + g0[i]).item())
            else:
                assert acc[i].item() == keep[i].item() or (first and acc[i] != acc[i])
    g = g0.clone()
    out_bf = torch.full((hi - lo + 64,), -1024.0, dtype=torch.bfloat16)
    ref.grad_fold(g, a0, lo, hi, out_bf)
    want = g0 + a0
    assert torch.equal(g[lo:hi], want[lo:hi]) and torch.equal(g[:lo], g0[:lo]) and torch.equal(g[hi:], g0[hi:])
    assert torch.equal(out_bf[:hi - lo], want[lo:hi].bfloat16()) and bool((out_bf[hi - lo:] == -1024.0).all())
    g = g0.clone()
    ref.grad_fold(g, a0, lo, hi)
    assert torch.equal(g[lo:hi], want[lo:hi])


def test_oracle_rounds_to_nearest_even_and_checks_its_arguments():
    g = torch.zeros(64)
    acc = torch.zeros(64)
    g[0], acc[0] = 1.0, 2.0 ** -8  # exactly between two bf16 values: ties to even (1.0)
    g[1], acc[1] = 1.0 + 2.0 ** -7, 2.0 ** -8  # between 1.0078125 and 1.015625: ties to even (1.015625)
    out = torch.zeros(64, dtype=torch.bfloat16)
    ref.grad_fold(g, acc, 0, 64, out)
    assert out[0].item() == 1.0 and out[1].item() == 1.015625
    for bad in (lambda: ref.grad_accumulate(acc, g, 32, 64, False), lambda: ref.grad_accumulate(acc, g, 0, 128, True),
                lambda: ref.grad_fold(g.bfloat16(), acc, 0, 64), lambda: ref.grad_fold(g, acc[:32], 0, 32),
                lambda: ref.grad_fold(g, acc, 0, 64, torch.zeros(32, dtype=torch.bfloat16)),
                lambda: ref.grad_fold(g, acc, 0, 64, torch.zeros(64))):
        with pytest.raises(ValueError):
            bad()


def test_accumulator_protocol():
    st = ParamStore()
    p = st.new("w", (100,), init_normal(0.1))
    st.finalize("cpu")
    with pytest.raises(ValueError):
        GradAccumulator(st, 0)
    one = GradAccumulator(st, 1)
    assert not one.active and one.scale == 1.0 and one.buf is None
    with pytest.raises(RuntimeError):
        one.accumulate(first=True)
    acc = GradAccumulator(st, 3)
    assert acc.buf is None and acc.scale == 1.0 / 3
    red = GradReducer(st, enabled=False, accumulator=acc)
    with pytest.raises(RuntimeError):
        acc.accumulate(first=False)  # the first micro-batch must start the sum
    gs = [torch.full((100,), float(v)) for v in (1, 10, 100)]
    for k, g in enumerate(gs):
        red.begin_step(sync=(k == 2))
        st.deposit(p, g)
        if k < 2:
            acc.accumulate(first=(k == 0))
    with pytest.raises(RuntimeError):
        acc.accumulate(first=False)  # steps - 1 micro-batches are in: the next one is the final one
    red.finish()
    assert bool((p.grad == 111.0).all()) and bool((st.grad[100:] == 0).all())
    with pytest.raises(AssertionError):
        acc.fold(0, st.total)  # nothing accumulated for the next step yet
    assert acc.buf.data_ptr() != st.grad.data_ptr() and acc.buf.shape == st.grad.shape
    st2 = ParamStore()
    st2.new("w", (100,), init_normal(0.1))
    st2.finalize("cpu", grad_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        GradAccumulator(st2, 2)
    with pytest.raises(ValueError):
        GradReducer(st2, enabled=False, accumulator=acc)  # another store's accumulator


# --------------------------------------------------------------------------- large-batch equivalence
def test_llama_tiny_two_micro_batches_equal_the_large_batch():
    """One batch of 8 split into 2 x 4 (equal token counts, so the mean of the two mean losses is the batch-8 mean
    loss): the accumulated gradient times ``scale`` against the batch-8 gradient, per slot, as a relative error of
    norms. Tolerance: the rule of the project's gradient-vs-twin test of this model
    (tests/test_transformer_grads_gpu.py: err <= 2 x bf16 noise floor + 0.03) with the floor at 0, the fp32 CPU path
    having no bf16 noise: 0.03. The two halves' own gradients must differ by more than that, or the test would pass
    with either half alone."""
    from k8s_amd.models.llama import LLAMA_TINY, LlamaForCausalLM, synthetic_batch

    tol = 0.03

    def model():
        st = ParamStore()
        return LlamaForCausalLM(st, LLAMA_TINY).finalize("cpu", seed=7), st

    gen = torch.Generator().manual_seed(3)
    ids, labels = synthetic_batch(LLAMA_TINY, 8, 32, "cpu", generator=gen)
    assert int((labels[:4] != -100).sum()) == int((labels[4:] != -100).sum()) > 0
    m, st = model()
    st.begin_step()
    m(ids, labels, dtype=torch.float32).backward()
    st.zero_unwritten()
    big = st.grad.clone()

    m, st = model()
    acc = GradAccumulator(st, 2)
    red = GradReducer(st, enabled=False, accumulator=acc)
    halves = []
    for k in range(2):
        red.begin_step(sync=(k == 1))
        m(ids[4 * k:4 * k + 4], labels[4 * k:4 * k + 4], dtype=torch.float32).backward()
        st.zero_unwritten()
        halves.append(st.grad.clone())
        if k == 0:
            acc.accumulate(first=True)
    red.finish()
    assert torch.equal(st.grad, halves[1] + halves[0])
    got = st.grad * red.grad_scale
    checked = 0
    for p in st.params:
        sl = slice(p.offset, p.offset + p.numel)
        n = big[sl].norm().item()
        if n == 0:
            continue
        checked += 1
        assert (halves[0][sl] - halves[1][sl]).norm().item() / n > tol, p.name  # not vacuous
        assert (got[sl] - big[sl]).norm().item() / n <= tol, p.name
    assert checked >= len(st.params) - 1


# --------------------------------------------------------------------------- two ranks on gloo
SHAPES = [(64, 33), (129,), (7, 5, 3), (256,), (16, 16), (1000,), (300,)]
STEPS, MICRO = 3, 2


def _store(world):
    st = ParamStore()
    params = [st.new("p%d" % i, s, init_normal(0.5), decay=(i % 2 == 0), lowp=(i % 3 != 2))
              for i, s in enumerate(SHAPES)]
    st.finalize("cpu", pad_to=world * ALIGN, seed=5)
    return st, params


def _grads(rank, micro):
    g = torch.Generator().manual_seed(1000 * micro + 17 * rank + 3)
    return [torch.randn(s, generator=g) * (1.0 + rank) for s in SHAPES]


def _opt(st):
    return FusedLAMB(st, lr=0.01, weight_decay=0.01, max_grad_norm=10.0)


def _worker(rank, world, port, strategy, comm, out_dir):
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    st, params = _store(world)
    opt = _opt(st)
    acc = GradAccumulator(st, MICRO)
    dtype = torch.bfloat16 if comm == "bf16" else torch.float32
    launches = []  # (sync flag of the micro-batch, fold) of every collective launch
    if strategy == "ps":
        t = ShardedParameterService(st, opt, bucket_mb=0.002, comm_dtype=dtype, accumulator=acc)
        inner = t._push
        t._push = lambda b, fold=False: (launches.append((t.sync, fold)), inner(b, fold))[1]
        finish = t.step
    else:
        t = GradReducer(st, bucket_mb=0.002, comm_dtype=dtype, accumulator=acc)
        inner = t._launch
        t._launch = lambda b, fold=False: (launches.append((t.sync, fold)), inner(b, fold))[1]

        def finish():
            t.finish()
            opt.step(grad_scale=t.grad_scale)
    check = t.self_check()  # step 0, without folding
    n_check = len(launches)
    assert t.grad_scale == 1.0 / (world * MICRO)
    per_micro = []
    for step in range(STEPS):
        for k in range(MICRO):
            t.begin_step(sync=(k == MICRO - 1))
            before = len(launches)
            for p, g in reversed(list(zip(params, _grads(rank, step * MICRO + k)))):
                st.deposit(p, g)
            if k < MICRO - 1:
                acc.accumulate(first=(k == 0))
                per_micro.append(len(launches) - before)
        finish()
    if strategy == "ps":
        t.sync_master()
    torch.save({"master": st.master.clone(), "check": check, "n_check": n_check, "launches": launches,
                "non_final": per_micro, "buckets": len(t.buckets)},
               os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def _run(strategy, comm, world=2):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(world, free_port(), strategy, comm, d), nprocs=world)
        return [torch.load(os.path.join(d, "rank%d.pt" % r), weights_only=False) for r in range(world)]


_single = {}


def _single_process(world=2):
    """One process accumulating the world x MICRO micro-batches of every step in rank-major order."""
    if "master" not in _single:
        st, params = _store(world)
        opt = _opt(st)
        acc = GradAccumulator(st, world * MICRO)
        red = GradReducer(st, enabled=False, accumulator=acc)
        for step in range(STEPS):
            order = [(r, k) for r in range(world) for k in range(MICRO)]
            for i, (r, k) in enumerate(order):
                last = i == len(order) - 1
                red.begin_step(sync=last)
                for p, g in reversed(list(zip(params, _grads(r, step * MICRO + k)))):
                    st.deposit(p, g)
                if not last:
                    acc.accumulate(first=(i == 0))
            red.finish()
            opt.step(grad_scale=red.grad_scale)
        _single["master"] = st.master.clone()
    return _single["master"]


@pytest.mark.parametrize("strategy,comm", [("allreduce", "fp32"), ("allreduce", "bf16"), ("ps", "fp32")])
def test_two_ranks_accumulate(strategy, comm):
    a, b = _run(strategy, comm)
    assert a["check"]["ok"] and b["check"]["ok"], a["check"]
    assert torch.equal(a["master"], b["master"])  # the replicas stay identical
    for r in (a, b):
        assert r["buckets"] > 3
        assert r["non_final"] == [0] * (STEPS * (MICRO - 1))  # non-final micro-batches launch no collective
        assert r["launches"][:r["n_check"]] == [(True, False)] * r["n_check"]  # the self-check does not fold
        # every optimizer step: each bucket once, in the final micro-batch, folded
        assert r["launches"][r["n_check"]:] == [(True, True)] * (STEPS * r["buckets"])
    single = _single_process()
    assert not torch.equal(single, _store(2)[0].master)
    if comm == "fp32":  # the tolerance of the all-reduce vs sharded-service agreement tests (summation order only)
        torch.testing.assert_close(a["master"], single, rtol=1e-5, atol=1e-6)
    else:  # sanity only: the bf16 transport rounds each rank's contribution once (2^-8 relative)
        assert (a["master"] - single).abs().max().item() < 0.05


# --------------------------------------------------------------------------- trainer end to end
def _events(logdir):
    with open(os.path.join(logdir, "metrics.jsonl")) as f:
        return [json.loads(line) for line in f if line.strip()]


def _trainer(args, env):
    return subprocess.run([sys.executable, "-m", "k8s_amd.trainer", "--device", "cpu", "--model", "bert_tiny"] + args,
                          env=env, capture_output=True, text=True, timeout=300)


def _env():
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("TF_CONFIG", "RANK", "WORLD_SIZE"):
        env.pop(k, None)
    return env


def test_trainer_accum_steps_resume_reports_the_same_losses():
    env = _env()
    common = ["--accum-steps", "2", "--steps", "6", "--fresh-batches", "--dropout", "0.1", "--ckpt-every", "3",
              "--log-every", "1"]
    with tempfile.TemporaryDirectory() as d:
        full, part = os.path.join(d, "full"), os.path.join(d, "part")
        r = _trainer(common + ["--logdir", full, "--ckpt-dir", os.path.join(d, "ck_full")], env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        args = common + ["--logdir", part, "--ckpt-dir", os.path.join(d, "ck_part"), "--fail-at-step", "3"]
        r = _trainer(args, env)
        assert r.returncode == 138, r.stdout[-2000:] + r.stderr[-2000:]  # the injected, retryable failure
        n_first = len(_events(part))
        r = _trainer(args, env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        ev_full, ev_part = _events(full), _events(part)
    start = [e for e in ev_full if e.get("event") == "start"][0]
    assert start["accum_steps"] == 2 and start["batch"] == 4 and start["world"] == 1 and start["global_batch"] == 8
    loss = lambda evs: {e["step"]: e["loss"] for e in evs if e.get("event") in ("step0", "step")}  # noqa: E731
    whole = loss(ev_full)
    assert sorted(whole) == [0, 1, 2, 3, 4, 5]
    assert sorted(loss(ev_part[:n_first])) == [0, 1, 2]
    resumed = ev_part[n_first:]
    assert [e["step"] for e in resumed if e.get("event") == "restored"] == [2]
    again = loss(resumed)
    assert sorted(again) == [3, 4, 5]
    assert {s: whole[s] for s in (3, 4, 5)} == again  # the dropout step and the batch index after the resume
    assert {s: whole[s] for s in (0, 1, 2)} == loss(ev_part[:n_first])
    assert len(set(whole.values())) == 6
    # the rate counts both micro-batches: 2 x 4 sequences x 32 tokens per step
    steps = [e for e in ev_full if e.get("event") in ("step0", "step")]
    for prev, e in zip(steps[1:], steps[2:]):  # (step 2 -> 3 holds a checkpoint save in both measures)
        expect = 2 * 4 * 32 / (e["time"] - prev["time"])
        assert 0.7 < e["tokens_per_sec"] / expect < 1.4, (e, expect)


def test_trainer_accum_steps_one_is_the_plain_step():
    """``--accum-steps 1`` is the run without the flag: the same losses."""
    env = _env()
    base = ["--steps", "3", "--fresh-batches", "--log-every", "1"]
    with tempfile.TemporaryDirectory() as d:
        out = []
        for i, extra in enumerate(([], ["--accum-steps", "1"])):
            logdir = os.path.join(d, "log%d" % i)
            r = _trainer(base + extra + ["--logdir", logdir], env)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            out.append([(e["step"], e["loss"]) for e in _events(logdir) if e.get("event") in ("step0", "step")])
    assert out[0] == out[1] and len(out[0]) == 3


@pytest.mark.parametrize("extra", [["--accum-steps", "0"], ["--accum-steps", "2", "--graph"]])
def test_trainer_accum_steps_configuration_errors(extra):
    r = _trainer(["--steps", "1"] + extra, _env())
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert "--accum-steps" in r.stderr


def test_accum_example_manifest_validates():
    from k8s_amd import _operator as op
    from k8s_amd.fakeapi.cluster import REPO, load_manifests

    (d,) = load_manifests(os.path.join(REPO, "examples", "tf_job_bert_lamb_accum_1gpu.yaml"))
    spec, err = op.set_defaults(json.dumps(d["spec"]))
    assert err == "" and op.validate(spec) == ""
    (rs,) = d["spec"]["replicaSpecs"]
    assert rs["tfReplicaType"] == "MASTER" and rs["replicas"] == 1
    args = rs["template"]["spec"]["containers"][0]["args"]
    opt = dict(zip(args[::2], args[1::2]))
    assert opt["--batch"] == "1024" and opt["--accum-steps"] == "8" and opt["--optimizer"] == "lamb"
    (ref8,) = [m for m in load_manifests(os.path.join(REPO, "examples", "tf_job_bert_lamb_dp8.yaml"))]
    args8 = ref8["spec"]["replicaSpecs"][0]["template"]["spec"]["containers"][0]["args"]
    opt8 = dict(zip(args8[::2], args8[1::2]))
    for k in ("--warmup-steps", "--lr-schedule", "--lr-power", "--lr-end", "--lr", "--steps", "--weight-decay"):
        assert opt[k] == opt8[k], k
    from k8s_amd.trainer.runner import parse

    a = parse(args)
    assert a.accum_steps == 8 and a.batch * a.accum_steps == 8192
