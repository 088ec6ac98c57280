"""LARS / LAMB on the flat store, CPU tier: the optimizers against a textbook fp64 per-parameter implementation, the
skipped step, the learning-rate schedule, the two data-parallel strategies on gloo, and the trainer end to end."""
import json
import math
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from k8s_amd.fakeapi.server import free_port
from k8s_amd.ops.optim import FusedLAMB, FusedLARS
from k8s_amd.parallel.flat import ALIGN, ParamStore, init_const, init_normal
from k8s_amd.trainer.schedule import lr_at

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from layerwise_textbook import Textbook  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


SHAPES = [(64, 33), (129,), (7, 5, 3), (256,), (16, 16), (1000,), (40,), (300,), (50,)]
# an all-zero slot that decays; a zero-gradient slot that decays and one that does not. By the definitions r = 1 for
# the first (||p|| = 0) and the last (no decay) under both optimizers and for the second under LARS (||g|| = 0). Under
# LAMB the second has u = wd p, so ||u|| > 0 and r = ||p|| / ||u|| = 1 / wd: finite, and checked against the textbook.
ZERO_PARAM, ZERO_GRAD, ZERO_GRAD_NODECAY = 6, 7, 8


def _store(world=1, seed=5):
    store = ParamStore()
    params = []
    for i, s in enumerate(SHAPES):
        decay = (i % 2 == 0 or i == ZERO_GRAD) and i != ZERO_GRAD_NODECAY
        init = init_const(0.0) if i == ZERO_PARAM else init_normal(0.5)
        params.append(store.new("p%d" % i, s, init, decay=decay, lowp=(i % 3 != 2)))
    store.finalize("cpu", pad_to=world * ALIGN, seed=seed)
    return store, params


def _grads(rank, step, scale=1.0):
    g = torch.Generator().manual_seed(1000 * step + 17 * rank + 3)
    gs = [torch.randn(s, generator=g) * (1.0 + rank) * scale for s in SHAPES]
    gs[ZERO_GRAD].zero_()
    gs[ZERO_GRAD_NODECAY].zero_()
    return gs


def _make(kind, store, clip):
    if kind == "lars":
        return FusedLARS(store, lr=0.05, momentum=0.9, weight_decay=1e-3, trust_coef=0.02, max_grad_norm=clip)
    return FusedLAMB(store, lr=0.01, weight_decay=0.01, max_grad_norm=clip)


def _textbook(kind, store, params, clip):
    if kind == "lars":
        return Textbook("lars", [p.master for p in params], [p.decay for p in params], 0.05, 1e-3, clip, eta=0.02)
    return Textbook("lamb", [p.master for p in params], [p.decay for p in params], 0.01, 0.01, clip)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_matches_textbook_fp64(kind):
    store, params = _store()
    opt = _make(kind, store, clip=5.0)  # the gradient norm is ~40: the clip is active
    book = _textbook(kind, store, params, 5.0)
    half0 = store.half.clone()
    for step in range(3):
        gs = _grads(0, step)
        store.begin_step()
        for p, g in zip(params, gs):
            store.deposit(p, g)
        lr = None if step == 0 else 0.03 / (step + 1)
        opt.step(grad_scale=0.5, lr=lr)
        book.step(gs, grad_scale=0.5, lr=lr)
        ratio = opt.last_trust_ratio
        assert ratio.shape == (len(params),) and bool(torch.isfinite(ratio).all())
        torch.testing.assert_close(ratio.double(), torch.tensor(book.ratio, dtype=torch.float64), rtol=1e-5, atol=0)
        assert float(ratio[ZERO_GRAD_NODECAY]) == 1.0
        if step == 0:  # (its first update moves the all-zero slot off zero)
            assert float(ratio[ZERO_PARAM]) == 1.0
        if kind == "lars":
            assert float(ratio[ZERO_GRAD]) == 1.0
        else:
            assert float(ratio[ZERO_GRAD]) == pytest.approx(1.0 / 0.01, rel=1e-5)
        for i, p in enumerate(params):
            if not p.decay:
                assert float(ratio[i]) == 1.0
    assert bool(torch.isfinite(store.master).all())
    for i, p in enumerate(params):
        torch.testing.assert_close(p.master.double(), book.p[i].reshape(p.shape), rtol=1e-5, atol=1e-6)
        if p.lowp:
            assert torch.equal(p.half, p.master.to(torch.bfloat16))
        else:  # the working copy of an fp32-read slot is not the optimizer's to write
            sl = slice(p.offset, p.offset + p.numel)
            assert torch.equal(store.half[sl], half0[sl])
    assert opt.step_count == 3
    keys = {"momentum_buffer", "step"} if kind == "lars" else {"exp_avg", "exp_avg_sq", "step"}
    assert set(opt.state_dict()) == keys


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_all_zero_gradient_gives_ratio_one_and_no_nan(kind):
    """Every gradient zero, no clipping: the norms in both denominators vanish. LARS leaves every weight where it
    is decayed to (r = 1); nothing is NaN under either optimizer."""
    store, params = _store()
    opt = _make(kind, store, clip=None)
    before = store.master.clone()
    for p in params:
        store.deposit(p, torch.zeros(p.shape))
    opt.step()
    r = opt.last_trust_ratio
    assert bool(torch.isfinite(store.master).all()) and bool(torch.isfinite(r).all())
    assert float(r[ZERO_PARAM]) == 1.0
    if kind == "lars":
        assert bool((r == 1.0).all())
        for p in params:
            sl = slice(p.offset, p.offset + p.numel)
            want = before[sl] * (1 - 0.05 * 1e-3) if p.decay else before[sl]
            torch.testing.assert_close(store.master[sl], want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_nonfinite_gradient_skips_the_step(kind):
    store, params = _store()
    opt = _make(kind, store, clip=5.0)
    for step in range(2):
        for p, g in zip(params, _grads(0, step)):
            store.deposit(p, g)
        opt.step()
    before = [store.master.clone(), store.half.clone(), opt.last_trust_ratio.clone()] + \
        [t.clone() for t in opt.state_tensors()]
    gs = _grads(0, 2)
    gs[3][5] = float("inf")
    for p, g in zip(params, gs):
        store.deposit(p, g)
    opt.step()
    after = [store.master, store.half, opt.last_trust_ratio] + opt.state_tensors()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------- learning-rate schedule
def test_lr_at_defaults_are_the_warmup_expression():
    for lr in (0.1, 1e-4, 3.2):
        for warmup in (0, 1, 5, 7, 100):
            for step in range(0, 130):
                want = lr * min(1.0, (step + 1) / warmup) if warmup else lr
                assert lr_at(step, lr, warmup) == want
                assert lr_at(step, lr, warmup, 130) == want
                assert lr_at(step, lr, warmup, 130, "constant", 0.0, 2.0) == want


@pytest.mark.parametrize("schedule", ["poly", "cosine"])
def test_lr_at_decay_end_points_and_monotonicity(schedule):
    lr, end, warmup, steps = 0.8, 0.01, 5, 40
    vals = [lr_at(s, lr, warmup, steps, schedule, end, 2.0) for s in range(steps)]
    for s in range(warmup):  # the warmup is the linear one, whatever follows
        assert vals[s] == lr * min(1.0, (s + 1) / warmup)
    assert vals[warmup - 1] == lr
    assert vals[-1] == pytest.approx(end, abs=1e-12)
    assert all(a < b for a, b in zip(vals[:warmup - 1], vals[1:warmup]))
    assert all(a > b for a, b in zip(vals[warmup - 1:-1], vals[warmup:]))
    assert all(end - 1e-12 <= v <= lr for v in vals)
    assert lr_at(steps + 10, lr, warmup, steps, schedule, end) == pytest.approx(end, abs=1e-12)  # past the end
    mid = warmup + (steps - warmup) // 2 - 1  # t = 17 / 35
    t = (mid + 1 - warmup) / (steps - warmup)
    f = (1 - t) ** 2 if schedule == "poly" else 0.5 * (1 + math.cos(math.pi * t))
    assert vals[mid] == pytest.approx(end + (lr - end) * f, rel=1e-12)
    assert lr_at(3, lr, 0, 8, "poly", 0.0, 1.0) == pytest.approx(lr * 0.5)  # no warmup, linear decay
    with pytest.raises(ValueError):
        lr_at(0, lr, 0, 8, "step")


# --------------------------------------------------------------------------- two ranks on gloo
def _worker(rank, world, port, strategy, kind, steps, out_dir):
    from k8s_amd.parallel.ddp import GradReducer
    from k8s_amd.parallel.ps import ShardedParameterService

    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    store, params = _store(world)
    opt = _make(kind, store, clip=10.0)
    if strategy == "ps":
        svc = ShardedParameterService(store, opt, bucket_mb=0.002)  # several buckets: slots are cut between ranks
        begin, finish = svc.begin_step, (lambda: svc.step())
    else:
        red = GradReducer(store, bucket_mb=0.002)
        begin = red.begin_step

        def finish():
            red.finish()
            opt.step(grad_scale=red.grad_scale)
        svc = None
    for step in range(steps):
        begin()
        for p, g in reversed(list(zip(params, _grads(rank, step)))):  # backward order
            store.deposit(p, g)
        finish()
    if svc is not None:
        svc.sync_master()
    full = svc.gather_state() if svc is not None else None
    if rank == 0:
        sd = opt.state_dict(full)
        torch.save({"master": store.master.clone(), "ratio": opt.last_trust_ratio.clone(),
                    **{k: v.clone() for k, v in sd.items() if torch.is_tensor(v)},
                    "state_numel": opt.state_numel(), "total": store.total},
                   os.path.join(out_dir, "%s_%s.pt" % (strategy, kind)))
    dist.barrier()
    dist.destroy_process_group()


def _run(world, strategy, kind, steps=4):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(world, free_port(), strategy, kind, steps, d), nprocs=world)
        return torch.load(os.path.join(d, "%s_%s.pt" % (strategy, kind)), weights_only=True)


def _reference(world, kind, steps):
    """Single-process ground truth: the fp32 sum of every rank's gradient, one optimizer over everything."""
    store, params = _store(world)
    opt = _make(kind, store, clip=10.0)
    for step in range(steps):
        store.begin_step()
        per = [_grads(r, step) for r in range(world)]
        for i, p in enumerate(params):
            store.deposit(p, sum(per[r][i] for r in range(world)))
        opt.step(grad_scale=1.0 / world)
    return store.master.clone(), opt.last_trust_ratio.clone()


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_allreduce_and_sharded_ps_agree(kind):
    world = 2
    a = _run(world, "allreduce", kind)
    b = _run(world, "ps", kind)
    keys = ["master", "ratio"] + (["momentum_buffer"] if kind == "lars" else ["exp_avg", "exp_avg_sq"])
    for k in keys:  # not bit-for-bit: a slot cut between the ranks adds its sums in another order
        torch.testing.assert_close(a[k], b[k], rtol=1e-5, atol=1e-6, msg=k)
    master, ratio = _reference(world, kind, 4)
    for got in (a, b):
        torch.testing.assert_close(got["master"], master, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(got["ratio"], ratio, rtol=1e-5, atol=1e-6)
    n_state = 1 if kind == "lars" else 2
    assert a["state_numel"] == n_state * a["total"]
    assert b["state_numel"] == n_state * b["total"] // world


# --------------------------------------------------------------------------- trainer end to end
def _events(logdir):
    with open(os.path.join(logdir, "metrics.jsonl")) as f:
        return [json.loads(line) for line in f if line.strip()]


@pytest.mark.parametrize("model,opt", [("resnet_tiny", "lars"), ("bert_tiny", "lamb")])
def test_trainer_poly_schedule_checkpoint_resume(model, opt):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("TF_CONFIG", "RANK", "WORLD_SIZE"):
        env.pop(k, None)
    with tempfile.TemporaryDirectory() as d:
        logdir, ckpt = os.path.join(d, "log"), os.path.join(d, "ckpt")
        base = [sys.executable, "-m", "k8s_amd.trainer", "--model", model, "--optimizer", opt, "--device", "cpu",
                "--batch", "2", "--lr-schedule", "poly", "--lr-end", "1e-5", "--warmup-steps", "2",
                "--log-every", "1", "--logdir", logdir, "--ckpt-dir", ckpt, "--max-grad-norm", "1.0"]
        r = subprocess.run(base + ["--steps", "4"], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        first = _events(logdir)
        r = subprocess.run(base + ["--steps", "7"], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        ev = _events(logdir)[len(first):]
    start = [e for e in first if e.get("event") == "start"][0]
    assert start["optimizer"] == opt and start["lr_schedule"] == "poly"
    restored = [e for e in ev if e.get("event") == "restored"]
    assert restored and restored[0]["step"] == 3
    steps = [e for e in ev if e.get("event") == "step"]
    assert [e["step"] for e in steps] == [5, 6]  # (step 4 is the resumed run's step0 event)
    lrs = [e["lr"] for e in steps]
    assert lrs[0] > lrs[1] == pytest.approx(1e-5)
    done = [e for e in first if e.get("event") == "step"]
    assert done and all(a["lr"] > b["lr"] for a, b in zip(done[1:], done[2:]))  # falling after the warmup
    for e in steps + done:
        assert e["trust_ratio_min"] <= e["trust_ratio_mean"] <= e["trust_ratio_max"]
        assert e["trust_ratio_min"] > 0 and math.isfinite(e["trust_ratio_max"])
        assert math.isfinite(e["loss"])
