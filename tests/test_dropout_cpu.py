"""Dropout on the counter generator (csrc/kernels/rng.h, ops/reference.py): known answers, mask statistics, the
CPU autograd paths of nn.dropout / nn.layer_norm(dropout=) / attention(dropout=), bert_tiny and the trainer flag."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from k8s_amd.ops import nn as K
from k8s_amd.ops import reference as ref
from k8s_amd.ops.attention import attention, attention_reference
from k8s_amd.parallel.flat import ParamStore, init_const

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234ABCD5678


# --------------------------------------------------------------------------------------------- 1. known answers
def test_philox_known_answers():
    """The three Random123 Philox4x32-10 known-answer vectors (kat_vectors: zeros, all ones, the pi digits)."""
    def run(ctr, key):
        t = [torch.tensor([v], dtype=torch.int64) for v in ctr + key]
        return [int(v) for v in ref.philox4x32(tuple(t[:4]), tuple(t[4:]))]

    assert run([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert run([f, f, f, f], [f, f]) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert run([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_rowkey_and_keep_known_answers():
    rows = torch.tensor([0, 1, 2, 2 ** 32 + 5], dtype=torch.int64)
    rk = ref.dropout_rowkey((SEED, 3), 7, rows)
    assert [int(v) for v in rk] == [0x0582B5E2, 0xDC5B8661, 0x79E04C65, 0x620183D4]

    def bits(m):
        return ["".join("1" if v else "0" for v in r) for r in m.tolist()]

    assert bits(ref.dropout_keep((SEED, 3), 7, 2, 8, 0.5)) == ["11101000", "00001110"]
    assert bits(ref.dropout_keep((SEED, 3), 7, 4, 16, 0.1)) == ["1111110011111111", "1110111111111111",
                                                                "1101111111110100", "1111111111111111"]
    # the same through a DropoutState and its tensor, with explicit row / column index tensors
    st = K.DropoutState(SEED)
    st.set_step(3)
    assert st.seed == SEED and st.step == 3
    a = ref.dropout_keep(st, 7, torch.arange(4), torch.arange(16), 0.1)
    assert torch.equal(a, ref.dropout_keep((SEED, 3), 7, 4, 16, 0.1))
    assert torch.equal(a, ref.dropout_keep(st.tensor, 7, 4, 16, 0.1))
    # row 2^32 + 5 is not row 5: the high word reaches the counter
    hi = ref.dropout_keep((SEED, 3), 7, torch.tensor([5, 2 ** 32 + 5]), 64, 0.5)
    assert not torch.equal(hi[0], hi[1])


def test_drop_params():
    assert ref.drop_params(0.0) == (0, 1.0)
    assert ref.drop_params(0.5) == (2 ** 31, 2.0)
    thr, scale = ref.drop_params(0.1)
    assert thr == math.floor(0.1 * 2 ** 32 + 0.5)
    assert scale == torch.tensor(1.0 / (1.0 - thr / 2 ** 32), dtype=torch.float32).item()
    assert ref.drop_params(1.0 - 2 ** -40)[0] == 2 ** 32 - 1
    with pytest.raises(ValueError):
        ref.drop_params(1.0)


# --------------------------------------------------------------------------------------------- 2. statistics
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_statistics(p):
    R, C = 512, 768
    thr, _ = ref.drop_params(p)
    q = 1.0 - thr / 2 ** 32
    sd = math.sqrt(q * (1 - q))
    masks = {}
    for step in range(3):
        for site in range(3):
            masks[(step, site)] = ref.dropout_keep((SEED, step), site, R, C, p).double()
    for key, m in masks.items():
        n = R * C
        z = (m.mean().item() - q) / (sd / math.sqrt(n))
        assert abs(z) <= 4.5, ("keep fraction", key, z)
        d = m - q
        for name, prod in (("rows", d[:, :-1] * d[:, 1:]), ("cols", d[:-1, :] * d[1:, :])):
            corr = prod.mean().item() / (sd * sd)
            assert abs(corr) * math.sqrt(prod.numel()) <= 4.5, ("lag-1 correlation along " + name, key, corr)
        zr = (m.mean(1) - q) / (sd / math.sqrt(C))
        zc = (m.mean(0) - q) / (sd / math.sqrt(R))
        assert zr.abs().max().item() <= 5.5, ("per-row keep fraction", key, zr.abs().max().item())
        assert zc.abs().max().item() <= 5.5, ("per-column keep fraction", key, zc.abs().max().item())
    agree = q * q + (1 - q) * (1 - q)
    keys = sorted(masks)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            f = (masks[a] == masks[b]).double().mean().item()
            z = (f - agree) / math.sqrt(agree * (1 - agree) / (R * C))
            assert abs(z) <= 4.5, ("agreement", a, b, z)


# --------------------------------------------------------------------------------------------- 3. autograd (CPU fp32)
def _ln_params(D, seed):
    store = ParamStore()
    pg = store.new("g", (D,), init_const(1), decay=False, lowp=False)
    pb = store.new("b", (D,), init_const(0), decay=False, lowp=False)
    store.finalize("cpu", seed=seed)
    g = torch.Generator().manual_seed(seed)
    pg.master.copy_(torch.rand(D, generator=g) + 0.5)
    pb.master.copy_(torch.randn(D, generator=g) * 0.1)
    return store, pg, pb


def test_layer_norm_dropout_autograd():
    R, D, p, site = 9, 40, 0.3, 5
    st = K.DropoutState(11)
    st.set_step(4)
    store, pg, pb = _ln_params(D, 1)
    gen = torch.Generator().manual_seed(2)
    x0, r0, dy, dxs = (torch.randn(R, D, generator=gen) for _ in range(4))
    x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
    store.begin_step()
    y, xsum = K.layer_norm(x, pg, pb, 1e-5, residual=r, dropout=(p, st, site))
    torch.autograd.backward([y, xsum], [dy, dxs])
    store.zero_unwritten()
    # the written-out composition with the same mask
    keep = ref.dropout_keep(st, site, R, D, p)
    _, scale = ref.drop_params(p)
    xr, rr = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
    gr, br = (t.master.detach().clone().reshape(D).requires_grad_(True) for t in (pg, pb))
    xs = torch.where(keep, xr * scale, torch.zeros(())) + rr
    yr = torch.nn.functional.layer_norm(xs, (D,), gr, br, 1e-5)
    torch.autograd.backward([yr, xs], [dy, dxs])
    for a, b in ((y, yr), (xsum, xs), (x.grad, xr.grad), (r.grad, rr.grad), (pg.grad.reshape(D), gr.grad),
                 (pb.grad.reshape(D), br.grad)):
        assert (a.detach() - b.detach()).abs().max().item() <= 1e-5
    assert (x.grad[~keep] == 0).all() and not torch.equal(x.grad, r.grad)
    # p = 0: the call without the argument
    y0, s0 = K.layer_norm(x0, pg, pb, 1e-5, residual=r0, dropout=(0.0, st, site))
    y1, s1 = K.layer_norm(x0, pg, pb, 1e-5, residual=r0)
    assert torch.equal(y0, y1) and torch.equal(s0, s1)
    with pytest.raises(ValueError):
        K.layer_norm(x0, pg, pb, 1e-5, dropout=(p, st, site))


def test_dropout_autograd():
    R, D, p, site = 7, 24, 0.5, 2
    st = K.DropoutState(5)
    gen = torch.Generator().manual_seed(3)
    x0, dy = torch.randn(R, D, generator=gen), torch.randn(R, D, generator=gen)
    x = x0.clone().requires_grad_(True)
    y = K.dropout(x, p, st, site)
    y.backward(dy)
    keep = ref.dropout_keep(st, site, R, D, p)
    xr = x0.clone().requires_grad_(True)
    yr = torch.where(keep, xr * 2.0, torch.zeros(()))
    yr.backward(dy)
    assert (y.detach() - yr.detach()).abs().max().item() <= 1e-5
    assert (x.grad - xr.grad).abs().max().item() <= 1e-5
    assert 0 < keep.sum().item() < keep.numel()
    assert K.dropout(x0, 0.0, st, site) is x0
    # a [B, S, D] view uses rows B * S
    y3 = K.dropout(x0.reshape(1, R, D), p, st, site)
    assert torch.equal(y3.reshape(R, D), y.detach())


@pytest.mark.parametrize("causal,lens", [(False, None), (True, [13, 6])])
def test_attention_dropout_autograd(causal, lens):
    B, S, H, D, p, site = 2, 13, 3, 16, 0.25, 4
    st = K.DropoutState(21)
    st.set_step(2)
    gen = torch.Generator().manual_seed(4)
    q0, k0, v0, do = (torch.randn(B, S, H, D, generator=gen) for _ in range(4))
    kv = torch.tensor(lens) if lens else None
    q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
    o = attention(q, k, v, causal=causal, kv_lens=kv, dropout=(p, st, site))
    o.backward(do)
    keep = ref.attention_keep(st, site, B, H, S, S, p)
    assert torch.equal(keep.reshape(B * H * S, S), ref.dropout_keep(st, site, B * H * S, S, p))
    _, scale = ref.drop_params(p)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
    s = torch.einsum("bqhd,bkhd->bhqk", qr, kr) / math.sqrt(D)
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    if lens:
        s = s.masked_fill((torch.arange(S)[None, :] >= kv[:, None])[:, None, None, :], float("-inf"))
    pr = torch.where(keep, torch.softmax(s, -1) * scale, torch.zeros(()))
    orf = torch.einsum("bhqk,bkhd->bqhd", pr, vr)
    orf.backward(do)
    for a, b in ((o, orf), (q.grad, qr.grad), (k.grad, kr.grad), (v.grad, vr.grad)):
        assert (a.detach() - b.detach()).abs().max().item() <= 1e-5
    assert torch.equal(attention(q0, k0, v0, causal=causal, kv_lens=kv, dropout=(0.0, st, site)),
                       attention(q0, k0, v0, causal=causal, kv_lens=kv))
    assert torch.equal(attention_reference(q0, k0, v0, causal, kv, None, keep, scale), o.detach())


# --------------------------------------------------------------------------------------------- 4. bert_tiny
def _bert(dropout, seed=3, dropout_seed=None):
    from k8s_amd.models.registry import build
    from k8s_amd.ops.optim import FusedAdam

    torch.manual_seed(0)
    w = build("bert_tiny", "cpu", 4, seed=seed, dropout=dropout, dropout_seed=dropout_seed)
    return w, FusedAdam(w.store, lr=1e-3, weight_decay=0.01)


def _train(w, opt, steps):
    out = []
    for i in range(steps):
        w.store.begin_step()
        loss = w.loss(w.batch(i))
        loss.backward()
        w.store.zero_unwritten()
        opt.step()
        out.append(loss.item())
    return out


def test_bert_tiny_dropout():
    w0, _ = _bert(None)
    w1, o1 = _bert(0.1)
    assert w1.model.c.hidden_dropout == 0.1 and w1.model.c.attention_dropout == 0.1
    assert torch.equal(w0.store.master, w1.store.master)
    b = w0.batch(0)
    with torch.no_grad():
        plain = w0.loss(b).item()
        dropped = w1.loss(b).item()  # training mode: this forward counts as step 1
    assert dropped != plain and abs(dropped - plain) < 0.5
    # evaluation: eval mode, no dropout, the training flag restored, the step untouched
    e0, e1 = w0.evaluate(b), w1.evaluate(b)
    assert e0["loss_sum"].item() == e1["loss_sum"].item() and e0["count"].item() == e1["count"].item()
    assert w1.model.training and w1.model.drop_state.step == 1
    w1.model.eval()
    with torch.no_grad():
        assert w1.loss(b).item() == plain
    w1.model.train()
    assert w1.model.drop_state.step == 1
    # same seed: identical loss sequences; another seed: not; the step counts the training forwards
    wa, oa = _bert(0.1)
    wb, ob = _bert(0.1)
    wc, oc = _bert(0.1, dropout_seed=99)
    la, lb, lc = _train(wa, oa, 3), _train(wb, ob, 3), _train(wc, oc, 3)
    assert la == lb and la != lc
    assert wa.model.drop_state.step == 3 and w0.model.drop_state.step == 0
    with pytest.raises(ValueError):
        from k8s_amd.models.registry import build

        build("llama_tiny", "cpu", 2, dropout=0.1)


# --------------------------------------------------------------------------------------------- 5. trainer
def _trainer(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""
    env["OMP_NUM_THREADS"] = "2"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "k8s_amd.trainer", "--device", "cpu"] + args, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    ev = []
    for line in p.stdout.splitlines():
        if line.startswith("{"):
            try:
                ev.append(json.loads(line))
            except ValueError:
                pass
    return p, ev


def _losses(ev):
    return {e["step"]: e["loss"] for e in ev if e.get("event") in ("step0", "step")}


def test_trainer_dropout_resume(tmp_path):
    base = ["--model", "bert_tiny", "--batch", "4", "--dropout", "0.1", "--log-every", "1", "--seed", "5"]
    p, ev = _trainer(base + ["--steps", "4"])
    assert p.returncode == 0, p.stdout
    assert [e for e in ev if e["event"] == "start"][0]["dropout"] == 0.1
    full = _losses(ev)
    p0, ev0 = _trainer(["--model", "bert_tiny", "--batch", "4", "--log-every", "1", "--seed", "5", "--steps", "1"])
    assert p0.returncode == 0 and [e for e in ev0 if e["event"] == "start"][0]["dropout"] == 0.0
    assert _losses(ev0)[0] != full[0]
    ck = str(tmp_path / "ckpt")
    p1, _ = _trainer(base + ["--steps", "2", "--ckpt-dir", ck])
    assert p1.returncode == 0, p1.stdout
    p2, ev2 = _trainer(base + ["--steps", "4", "--ckpt-dir", ck])
    assert p2.returncode == 0, p2.stdout
    assert [e for e in ev2 if e["event"] == "restored"][0]["step"] == 1
    resumed = _losses(ev2)
    assert sorted(resumed) == [2, 3]
    # the same fp32 arithmetic on the same weights, batch and masks; 1e-5 leaves room for the checkpoint round trip
    # only (a wrong mask step moves the loss by ~1e-2)
    for s in (2, 3):
        assert abs(resumed[s] - full[s]) <= 1e-5 * max(1.0, abs(full[s])), (s, resumed, full)


def test_trainer_dropout_needs_bert():
    p, _ = _trainer(["--model", "resnet_tiny", "--dropout", "0.1", "--steps", "1"])
    assert p.returncode == 1 and "--dropout" in p.stdout
