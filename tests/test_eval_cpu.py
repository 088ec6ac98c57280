"""Evaluation on CPU: the ``xent_eval`` oracle, ``ResNet.forward_infer`` against the eval-mode forward, and the
trainer's ``--eval-*`` flags (events, TensorBoard scalars, checkpoint round trip, two gloo ranks, error exits)."""
import glob
import json
import os
import subprocess
import sys

import torch

from k8s_amd.fakeapi.server import free_port
from k8s_amd.models.resnet import resnet_tiny
from k8s_amd.ops import conv as kconv
from k8s_amd.ops import nn as K
from k8s_amd.ops import reference as ref
from k8s_amd.parallel.flat import ParamStore
from k8s_amd.utils.tfevents import read_events

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ ops
def test_xent_eval_oracle_against_brute_force():
    torch.manual_seed(0)
    R, V = 12, 37
    logits = (torch.randn(R, V) * 2).bfloat16().float()  # coarse values: natural ties too
    labels = torch.randint(0, V, (R,))
    labels[3] = -100
    labels[5] = 20
    logits[5, [2, 19, 20, 30]] = logits[5].max() + 1  # the label tied with three columns, on both sides of it
    labels[6] = 0
    logits[6, :] = 1.0  # everything tied: the lowest index wins
    loss, rank = K.xent_eval(logits, labels)
    assert loss.dtype == torch.float32 and rank.dtype == torch.int32
    for r in range(R):
        y = int(labels[r])
        if y == -100:
            assert int(rank[r]) == V and float(loss[r]) == 0.0
            continue
        want = sum(1 for j in range(V) if logits[r, j] > logits[r, y] or (logits[r, j] == logits[r, y] and j < y))
        assert int(rank[r]) == want, (r, int(rank[r]), want)
        lse = torch.logsumexp(logits[r].double(), 0)
        assert abs(float(loss[r]) - float(lse - logits[r, y].double())) < 1e-5
    assert int(rank[5]) == 2 and int(rank[6]) == 0
    # padded vocabulary: only the first `valid` columns count
    padded = torch.cat([logits, torch.full((R, 3), 99.0)], 1)
    loss2, rank2 = K.xent_eval(padded, labels, valid=V)
    assert torch.equal(rank2, rank) and torch.equal(loss2, loss)


def test_conv_infer_composite_matches_oracle():
    """The composite a GPU shape outside the kernel's contract takes (here on CPU tensors) against the oracle."""
    torch.manual_seed(1)
    x, w = torch.randn(2, 6, 5, 3), torch.randn(5, 3, 3, 3) * 0.2
    scale, shift, res = torch.rand(5) + 0.5, torch.randn(5), torch.randn(2, 3, 3, 5)
    n0 = dict(kconv.STATS)
    for r in (None, res):
        for relu in (False, True):
            y = kconv.conv_infer(x, w, 2, 1, scale, shift, r, relu)
            torch.testing.assert_close(y, ref.conv_bn_act_infer(x, w, scale, shift, 2, 1, r, relu), rtol=1e-5,
                                       atol=1e-5)
    assert kconv.STATS == n0  # CPU products are the oracle path: not counted


def _tiny():
    store = ParamStore()
    model = resnet_tiny(store).finalize("cpu")
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for bn in model.batch_norms():
            c = bn.running_mean.numel()
            bn.gamma.master.copy_(torch.rand(c, generator=g) * 0.5 + 0.75)
            bn.beta.master.copy_(torch.randn(c, generator=g) * 0.1)
            bn.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
            bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    store.refresh_lowp()
    return model, store


def test_forward_infer_matches_eval_forward():
    model, store = _tiny()
    x = model.prepare_input(torch.randn(4, 32, 32, 3, generator=torch.Generator().manual_seed(1)))
    before = (store.master.clone(), store.grad.clone(), [b.clone() for b in model.buffers()])
    fused = model.forward_infer(x)
    flat, views = model.fold_bn()
    assert flat.dtype == torch.float32 and flat.numel() == 2 * sum(b.running_mean.numel() for b in model.batch_norms())
    assert views[0][0].data_ptr() == flat.data_ptr()  # views, not copies
    assert torch.equal(model.forward_infer(x, flat.clone()), fused)
    assert not fused.requires_grad and model.training
    assert torch.equal(before[0], store.master) and torch.equal(before[1], store.grad)
    assert all(torch.equal(a, b) for a, b in zip(before[2], model.buffers()))
    model.eval()
    with torch.no_grad():
        plain = model(x)
    torch.testing.assert_close(fused, plain, rtol=1e-5, atol=1e-5)
    # and the fp32 twin's eval mode is the same function
    from k8s_amd.models import resnet_ref

    params = {p.name: p.master.detach().clone() for p in store.params}
    with torch.no_grad():
        twin = resnet_ref.forward(model, params, x.permute(0, 3, 1, 2), training=False)
    torch.testing.assert_close(plain, twin, rtol=1e-4, atol=1e-4)


def test_workload_eval_batches_are_repeatable():
    from k8s_amd.models.registry import build

    w = build("resnet_tiny", "cpu", 4, fixed_batch=False)
    a0, a1 = w.eval_batch(0), w.eval_batch(1)
    w.batch(0)  # the training stream does not move the held-out one
    b0 = w.eval_batch(0)
    assert torch.equal(a0[0], b0[0]) and torch.equal(a0[1], b0[1]) and not torch.equal(a0[0], a1[0])
    assert w.eval_batch(0, 6)[0].shape[0] == 6
    out = w.evaluate(a0)
    assert set(out) == {"loss_sum", "count", "top1", "top5"} and int(out["count"]) == 4
    assert 0 <= int(out["top1"]) <= int(out["top5"]) <= 4
    for name in ("bert_tiny", "llama_tiny"):
        w = build(name, "cpu", 2)
        out = w.evaluate(w.eval_batch(0))
        assert set(out) == {"loss_sum", "count"} and int(out["count"]) > 0 and float(out["loss_sum"]) > 0


# ------------------------------------------------------------------------------------------------ trainer
def _env(tf_config=None):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    env["OMP_NUM_THREADS"] = "2"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG", "K8S_AMD_GRAPH"):
        env.pop(k, None)
    if tf_config is not None:
        env["TF_CONFIG"] = json.dumps(tf_config)
    return env


def _trainer(args, tf_config=None):
    return subprocess.Popen([sys.executable, "-m", "k8s_amd.trainer", "--device", "cpu", "--model", "resnet_tiny",
                             "--batch", "8"] + args, env=_env(tf_config), stdout=subprocess.PIPE,
                            stderr=subprocess.STDOUT, text=True)


def _run(args, tf_config=None, code=0):
    p = _trainer(args, tf_config)
    out, _ = p.communicate(timeout=240)
    assert p.returncode == code, out
    return out


def _evals(out):
    recs = []
    for line in out.splitlines():
        if line.startswith("{"):
            try:
                rec = json.loads(line)
            except ValueError:
                continue
            if rec.get("event") == "eval":
                recs.append(rec)
    return recs


def _result(rec):
    return {k: rec[k] for k in ("step", "loss", "top1", "top5", "examples")}


def test_training_batch_eval_run(tmp_path):
    lg = str(tmp_path / "log")
    ev = _evals(_run(["--steps", "40", "--eval-every", "10", "--eval-data", "train", "--logdir", lg]))
    assert [e["step"] for e in ev] == [9, 19, 29, 39]
    assert ev[-1]["top1"] == 1.0 and ev[-1]["loss"] < ev[0]["loss"]
    assert all(e["examples"] == 8 and e["images_per_sec"] > 0 for e in ev)
    scalars = {}
    for f in glob.glob(os.path.join(lg, "events.out.tfevents.*")):
        for e in read_events(f):
            for k, v in e["scalars"].items():
                scalars.setdefault(k, []).append((e["step"], v))
    assert [s for s, _ in scalars["eval/loss"]] == [9, 19, 29, 39]
    assert scalars["eval/top1"][-1] == (39, 1.0) and "eval/top5" in scalars
    with open(os.path.join(lg, "metrics.jsonl")) as f:
        logged = [json.loads(line) for line in f]
    assert [_result(e) for e in logged if e["event"] == "eval"] == [_result(e) for e in ev]


def test_heldout_eval_survives_checkpoint(tmp_path):
    ck = str(tmp_path / "ckpt")
    common = ["--eval-data", "heldout", "--eval-batches", "2", "--eval-batch", "4", "--ckpt-dir", ck]
    ev = _evals(_run(["--steps", "6", "--eval-every", "3"] + common))
    assert [e["step"] for e in ev] == [2, 5] and ev[-1]["examples"] == 8
    files = sorted(os.listdir(ck))
    first = _evals(_run(["--eval-only"] + common))
    second = _evals(_run(["--eval-only"] + common))
    assert len(first) == 1 and len(second) == 1
    assert _result(first[0]) == _result(ev[-1])
    assert _result(second[0]) == _result(first[0])
    assert sorted(os.listdir(ck)) == files  # --eval-only writes no checkpoint


def test_two_gloo_ranks_eval(tmp_path):
    pm, pw = free_port(), free_port()
    while pw == pm:
        pw = free_port()
    cluster = {"master": ["127.0.0.1:%d" % pm], "worker": ["127.0.0.1:%d" % pw]}
    lg = str(tmp_path / "log")
    args = ["--steps", "4", "--eval-every", "2", "--eval-batches", "3", "--eval-batch", "4", "--logdir", lg]
    procs = [_trainer(args, {"cluster": cluster, "task": {"type": t, "index": 0}, "environment": "cloud"})
             for t in ("master", "worker")]
    outs = []
    for p in procs:
        out, _ = p.communicate(timeout=300)
        outs.append(out)
        assert p.returncode == 0, out
    ev = _evals(outs[0])
    assert [e["step"] for e in ev] == [1, 3]  # one event per evaluation, from the chief
    assert all(e["examples"] == 2 * 3 * 4 for e in ev)
    assert not _evals(outs[1])
    with open(os.path.join(lg, "metrics.jsonl")) as f:
        assert sum(1 for line in f if json.loads(line)["event"] == "eval") == 2


def test_eval_configuration_errors_are_permanent(tmp_path):
    out = _run(["--steps", "10", "--eval-every", "5", "--graph"], code=1)
    assert "--graph" in out
    empty = tmp_path / "empty"
    empty.mkdir()
    out = _run(["--eval-only", "--ckpt-dir", str(empty)], code=1)
    assert "--eval-only" in out
