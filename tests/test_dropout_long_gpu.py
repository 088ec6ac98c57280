"""Attention dropout fused into the long-sequence kernels (attention.hip: the DROP forms of the multi-tile forward,
flash_delta_kernel's row-key table, flash_bwd_dkv_kernel, flash_bwd_dq_kernel and flash_dkv_reduce_kernel): the shape
contract, exact mask recovery per kernel, numerics against the fp32 reference with the same mask, the packed path,
step-to-step and captured masks, and a two-layer BERT at seq 256 against its CPU twin."""
import dataclasses
import glob
import math
import os

import pytest
import torch

from k8s_amd.ops import nn as K
from k8s_amd.ops import reference as ref
from k8s_amd.ops.attention import attention, attention_qkv, attention_reference

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234ABCD5678
PS = [0.1, 0.5]


def _C():
    from k8s_amd.ops._ext import load

    return load()


# --------------------------------------------------------------------------------------------- shape contract (CPU)
def test_flash_dropout_fused_contract():
    if not glob.glob(os.path.join(ROOT, "k8s_amd", "_C*.so")):
        pytest.skip("extension not built here (python -m k8s_amd._build)")
    import k8s_amd._C as C

    def fused(D, Sq, Sk, Hq, Hkv, causal=False, B=2):
        return C.flash_dropout_fused(D, Sq, Sk, Hq, Hkv, causal, B)

    assert fused(64, 256, 256, 12, 12)
    assert fused(64, 128, 128, 4, 2)
    assert fused(64, 512, 512, 2, 2, True, 1)  # the split dK/dV form
    for S in (128, 100, 16):  # the one-block shapes
        assert C.flash_bwd_one_block(64, S, S, 2, 2, False, 2) and fused(64, S, S, 2, 2)
    assert not fused(64, 200, 200, 2, 2)
    assert not fused(128, 256, 256, 8, 8)
    assert not fused(64, 256, 200, 2, 2)


# --------------------------------------------------------------------------------------------- helpers
def _close(a, b, tol, what=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    print("%s: max err %g (scale %g, tol %g)" % (what, err, scale, tol))
    assert err <= tol * max(1.0, scale), "%s: max err %g (scale %g)" % (what, err, scale)


def _misses(a, b, tol):
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).abs().max().item() > tol * max(1.0, b.abs().max().item() + 1e-6)


def _state(cuda, step=3, seed=SEED):
    st = K.DropoutState(seed, cuda)
    st.set_step(step)
    return st


def _qkv(cuda, B, S, H, D=64, seed=0):
    torch.manual_seed(seed)
    x = torch.randn(B * S, 3 * H * D, device=cuda).bfloat16()
    g = x.view(B, S, 3 * H, D)
    return x, g.narrow(2, 0, H), g.narrow(2, H, H), g.narrow(2, 2 * H, H)


def _valid(cuda, B, lens):
    valid = torch.ones(B, 1, 1, 1, device=cuda)
    for bi, n in enumerate(lens or []):
        if n == 0:  # every key masked: the reference gives NaN, the kernel 0
            valid[bi] = 0
    return valid


def _keep_checked(st, site, B, H, S, p):
    """The reference mask, every query row of which keeps at least one key and drops at least one (the precondition of
    the sign arguments; its failure probability is below 1e-10 at these sizes -- change the seed, not the test)."""
    keep = ref.attention_keep(st, site, B, H, S, S, p)
    kept = keep.sum(-1)
    assert (kept >= 1).all() and (kept <= S - 1).all()
    return keep


def _fwd(q, k, v, st, p, site, causal=False, lens=None):
    thr, scale = ref.drop_params(p)
    return _C().flash_fwd(q, k, v, causal, lens, 0.125, st.tensor, thr, scale, site)


def _bwd(do, q, k, v, o, lse, st, p, site):
    thr, scale = ref.drop_params(p)
    return _C().flash_bwd(do, q, k, v, o, lse, False, None, 0.125, None, None, st.tensor, thr, scale, site)


def _eye_rows(cuda):
    return torch.eye(64, device=cuda, dtype=torch.bfloat16).view(1, 64, 1, 64)


RECOVERY = [(2, 2, 256), (1, 1, 1024)]  # 64-wide tiles; the 128-wide tiles


# --------------------------------------------------------------------------------------------- mask recovery, exact
@gpu
@pytest.mark.parametrize("B,H,S", RECOVERY)
@pytest.mark.parametrize("p", PS)
def test_long_forward_mask_recovery(cuda, B, H, S, p):
    """q = k = 0 makes every probability 1 / S; V[key0 + j] = e_j shows keep(query, key0 + j) as O[query, j] > 0."""
    st, site = _state(cuda, step=5), 7
    keep = _keep_checked(st, site, B, H, S, p)
    z = torch.zeros(B, S, H, 64, device=cuda, dtype=torch.bfloat16)
    for key0 in range(0, S, 64):
        v = torch.zeros_like(z)
        v[:, key0:key0 + 64] = _eye_rows(cuda)
        o, _ = _fwd(z, z, v, st, p, site)
        got = (o > 0).permute(0, 2, 1, 3)  # [B, H, query, j]
        want = keep[..., key0:key0 + 64]
        assert torch.equal(got, want), (key0, (got != want).sum().item())


@gpu
@pytest.mark.parametrize("B,H,S", RECOVERY)
@pytest.mark.parametrize("p", PS)
def test_long_forward_lse_is_undropped(cuda, B, H, S, p):
    """l keeps the undropped row sum: lse with dropout is the plain forward's lse, bit for bit."""
    st = _state(cuda, step=5)
    _, q, k, v = _qkv(cuda, B, S, H, seed=2)
    _, lse = _fwd(q, k, v, st, p, 7)
    _, lse0 = _C().flash_fwd(q, k, v, False, None, 0.125)
    assert torch.equal(lse[..., :S], lse0[..., :S])


@gpu
@pytest.mark.parametrize("B,H,S", RECOVERY)
@pytest.mark.parametrize("p", PS)
def test_long_backward_dv_mask_recovery(cuda, B, H, S, p):
    """dO[q0 + j] = e_j for one 64-query block makes dV[key, j] = scale * keep(q0 + j, key) / S (the dK/dV kernel)."""
    st, site = _state(cuda, step=5), 10
    keep = _keep_checked(st, site, B, H, S, p)
    z = torch.zeros(B, S, H, 64, device=cuda, dtype=torch.bfloat16)
    torch.manual_seed(1)
    v = torch.randn(B, S, H, 64, device=cuda).bfloat16()
    o, lse = _fwd(z, z, v, st, p, site)
    for q0 in range(0, S, 64):
        do = torch.zeros_like(o)
        do[:, q0:q0 + 64] = _eye_rows(cuda)
        _, _, dv = _bwd(do, z, z, v, o, lse, st, p, site)
        got = (dv > 0).permute(0, 2, 3, 1)  # [B, H, j, key]
        want = keep[:, :, q0:q0 + 64, :]
        assert torch.equal(got, want), (q0, (got != want).sum().item())
        assert (dv[(dv > 0).logical_not()] == 0).all()


def _ones_column(cuda, B, S, H):
    x = torch.zeros(B, S, H, 64, device=cuda, dtype=torch.bfloat16)
    x[..., 0] = 1
    return x


def _ds_margin(keep, S, p):
    """dS[q, k] = (scale * keep - delta[q]) / S with delta[q] = bf16(O[q, 0]) = scale * kept / S up to 2^-8 relative:
    its sign is keep's when scale * (1 - kept / S) is above the rounding of O."""
    _, scale = ref.drop_params(p)
    kept = keep.sum(-1).double()
    assert (scale * (1 - kept / S) > 2.0 ** -7 * scale).all()


@gpu
@pytest.mark.parametrize("B,H,S", RECOVERY)
@pytest.mark.parametrize("p", PS)
def test_long_backward_dk_mask_recovery(cuda, B, H, S, p):
    """k = 0 and Q[q0 + j] = e_j: scores stay 0, and with V[:, 0] = dO[:, 0] = 1 the sign of dK[key, j] is
    keep(q0 + j, key) -- the dS path of the dK/dV kernel."""
    st, site = _state(cuda, step=5), 11
    keep = _keep_checked(st, site, B, H, S, p)
    _ds_margin(keep, S, p)
    z = torch.zeros(B, S, H, 64, device=cuda, dtype=torch.bfloat16)
    v = _ones_column(cuda, B, S, H)
    do = _ones_column(cuda, B, S, H)
    for q0 in range(0, S, 64):
        q = torch.zeros_like(z)
        q[:, q0:q0 + 64] = _eye_rows(cuda)
        o, lse = _fwd(q, z, v, st, p, site)
        _, dk, _ = _bwd(do, q, z, v, o, lse, st, p, site)
        dk = dk.permute(0, 2, 3, 1)  # [B, H, j, key]
        want = keep[:, :, q0:q0 + 64, :]
        assert torch.equal(dk > 0, want), (q0, ((dk > 0) != want).sum().item())
        assert torch.equal(dk < 0, ~want), (q0, ((dk < 0) == want).sum().item())


@gpu
@pytest.mark.parametrize("B,H,S", RECOVERY)
@pytest.mark.parametrize("p", PS)
def test_long_backward_dq_mask_recovery(cuda, B, H, S, p):
    """q = 0 and K[key0 + j] = e_j: the sign of dQ[q, j] is keep(q, key0 + j) -- the dQ kernel."""
    st, site = _state(cuda, step=5), 12
    keep = _keep_checked(st, site, B, H, S, p)
    _ds_margin(keep, S, p)
    z = torch.zeros(B, S, H, 64, device=cuda, dtype=torch.bfloat16)
    v = _ones_column(cuda, B, S, H)
    do = _ones_column(cuda, B, S, H)
    o, lse = _fwd(z, z, v, st, p, site)  # (q = 0: the forward does not depend on k)
    for key0 in range(0, S, 64):
        k = torch.zeros_like(z)
        k[:, key0:key0 + 64] = _eye_rows(cuda)
        dq, _, _ = _bwd(do, z, k, v, o, lse, st, p, site)
        dq = dq.permute(0, 2, 1, 3)  # [B, H, query, j]
        want = keep[..., key0:key0 + 64]
        assert torch.equal(dq > 0, want), (key0, ((dq > 0) != want).sum().item())
        assert torch.equal(dq < 0, ~want), (key0, ((dq < 0) == want).sum().item())


# --------------------------------------------------------------------------------------------- numerics
LONG_CASES = [
    # B, Sq, Sk, Hq, Hkv, causal, lens, full (False: O and dQ only)
    (1, 192, 192, 2, 2, False, None, True),
    (3, 256, 256, 2, 2, False, [256, 130, 0], True),
    (1, 512, 512, 2, 2, True, None, True),
    (2, 256, 256, 2, 2, True, [256, 100], True),
    (2, 64, 256, 2, 2, True, None, True),
    (2, 128, 128, 4, 2, False, None, True),
    (1, 1024, 1024, 1, 1, False, [900], True),
    (32, 256, 256, 8, 8, False, None, False),
]


def _operands(cuda, B, Sq, Sk, Hq, Hkv, seed=0):
    torch.manual_seed(seed)
    q = torch.randn(B, Sq, Hq, 64, device=cuda).bfloat16()
    k = torch.randn(B, Sk, Hkv, 64, device=cuda).bfloat16()
    v = torch.randn(B, Sk, Hkv, 64, device=cuda).bfloat16()
    return q, k, v


@gpu
@pytest.mark.parametrize("B,Sq,Sk,Hq,Hkv,causal,lens,full", LONG_CASES)
@pytest.mark.parametrize("p", PS)
def test_long_attention_dropout_fwd_bwd(cuda, B, Sq, Sk, Hq, Hkv, causal, lens, full, p):
    import k8s_amd.ops.attention as A

    C = _C()
    D, site = 64, 13
    st = _state(cuda, step=4)
    assert not C.flash_bwd_one_block(D, Sq, Sk, Hq, Hkv, causal, B)
    assert C.flash_dropout_fused(D, Sq, Sk, Hq, Hkv, causal, B)
    if (Sq, causal) == (512, True):
        assert C.flash_dkv_splits(B, Sq, Sk, Hkv, causal) == 4  # the fp32 partials and the reduce kernel's dV scale
    q, k, v = _operands(cuda, B, Sq, Sk, Hq, Hkv)
    kv_lens = torch.tensor(lens, device=cuda, dtype=torch.int32) if lens else None
    scale = 1.0 / math.sqrt(D)
    keep = ref.attention_keep(st, site, B, Hq, Sq, Sk, p)
    _, ks = ref.drop_params(p)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    want = attention_reference(qr, kr, vr, causal, kv_lens, scale, keep, ks)
    qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    before = A.DROPOUT_FALLBACKS
    out = attention(qq, kk, vv, causal=causal, kv_lens=kv_lens, dropout=(p, st, site))
    valid = _valid(cuda, B, lens)
    _close(out * valid, torch.nan_to_num(want) * valid, 2e-2, "O")
    do = torch.randn_like(out)
    want.backward(do.float())
    out.backward(do)
    assert A.DROPOUT_FALLBACKS == before  # the fused kernels ran, forward and backward
    _close(qq.grad, torch.nan_to_num(qr.grad), 3e-2, "dQ")
    if full:
        _close(kk.grad, torch.nan_to_num(kr.grad), 3e-2, "dK")
        _close(vv.grad, torch.nan_to_num(vr.grad), 3e-2, "dV")
    if Sq == 192:  # the bound does not hide a wrong mask: another site's mask misses it
        other = ref.attention_keep(st, site + 1, B, Hq, Sq, Sk, p)
        q2, k2, v2 = (t.detach().float().requires_grad_(True) for t in (q, k, v))
        wrong = attention_reference(q2, k2, v2, causal, kv_lens, scale, other, ks)
        wrong.backward(do.float())
        assert _misses(out, wrong, 2e-2)
        assert _misses(vv.grad, v2.grad, 3e-2)


# --------------------------------------------------------------------------------------------- packed path
@gpu
@pytest.mark.parametrize("p", PS)
def test_long_attention_qkv_packed(cuda, p):
    """attention_qkv at S = 256: the packed gradient written in place by the long kernels; the bias gradient stays a
    one-block feature (link.done false: the projection runs its own column sums)."""
    import k8s_amd.ops.attention as A
    from k8s_amd.parallel.flat import ParamStore, init_const

    B, S, H, D, site = 2, 256, 2, 64, 16
    st = _state(cuda, step=6)
    x, q, k, v = _qkv(cuda, B, S, H, seed=3)
    store = ParamStore()
    pb = store.new("qkv.bias", (3 * H * D,), init_const(0), decay=False, lowp=False)
    store.finalize(cuda, seed=1)
    link = K.BiasLink()
    link.pb = pb
    leaf = x.clone().requires_grad_(True)
    store.begin_step()
    before = A.DROPOUT_FALLBACKS
    o = attention_qkv(leaf * 1, B, S, H, H, D, bias_link=link, dropout=(p, st, site))
    do = torch.randn_like(o)
    o.backward(do)
    store.zero_unwritten()
    assert A.DROPOUT_FALLBACKS == before
    assert not link.done
    keep = ref.attention_keep(st, site, B, H, S, S, p)
    _, ks = ref.drop_params(p)
    xr = x.float().requires_grad_(True)
    g = xr.view(B, S, 3 * H, D)
    want = attention_reference(g.narrow(2, 0, H), g.narrow(2, H, H), g.narrow(2, 2 * H, H), False, None,
                               1.0 / math.sqrt(D), keep, ks)
    _close(o, want, 2e-2, "O")
    want.backward(do.float())
    _close(leaf.grad, xr.grad, 3e-2, "dqkv")


# --------------------------------------------------------------------------------------------- dropout 0 is plain
@gpu
def test_long_attention_dropout_zero_is_plain(cuda):
    st = _state(cuda)
    _, q, k, v = _qkv(cuda, 2, 256, 2)
    outs = []
    for kw in ({}, {"dropout": (0.0, st, 1)}):
        qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        o = attention(qq, kk, vv, **kw)
        o.backward(torch.ones_like(o))
        outs.append((o.detach(), qq.grad, kk.grad, vv.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------- steps and capture
def _step_fn(cuda, p, st, site, B=2, S=256, H=2):
    _, q, k, v = _qkv(cuda, B, S, H, seed=5)
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    torch.manual_seed(6)
    do = torch.randn(B, S, H, 64, device=cuda).bfloat16()

    def body(inputs=None, lr=None):
        st.advance()
        o = attention(q, k, v, dropout=(p, st, site))
        return (o.detach(),) + torch.autograd.grad(o, (q, k, v), do)

    return (q, k, v, do), body


@gpu
@pytest.mark.parametrize("p", PS)
def test_long_attention_masks_change_with_the_step(cuda, p):
    import k8s_amd.ops.attention as A

    B, S, H, site = 2, 256, 2, 4
    st = _state(cuda, step=20)
    (q, k, v, do), body = _step_fn(cuda, p, st, site)
    _, ks = ref.drop_params(p)
    before = A.DROPOUT_FALLBACKS
    masks = []
    for step in (21, 22):
        got = body()
        assert st.step == step
        keep = ref.attention_keep(st, site, B, H, S, S, p)
        masks.append(keep)
        qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
        want = attention_reference(qr, kr, vr, False, None, 0.125, keep, ks)
        want.backward(do.float())
        _close(got[0], want, 2e-2, "O step %d" % step)
        for name, a, b in zip(("dQ", "dK", "dV"), got[1:], (qr.grad, kr.grad, vr.grad)):
            _close(a, b, 3e-2, "%s step %d" % (name, step))
    assert A.DROPOUT_FALLBACKS == before
    assert not torch.equal(masks[0], masks[1])


class _NoOptimizer:
    """What StepGraph asks of an optimizer, for a body that has none."""
    step_count = 0

    def use_device_hyper(self):
        pass

    def prepare_replay(self, lr):
        pass


@gpu
@pytest.mark.parametrize("p", PS)
def test_long_attention_graph_replay_matches_eager(cuda, p):
    """Four steps eager against two eager steps, one capture and two replays of the same body: the kernels read the
    device [seed, step] pair (the row-key table is rebuilt on every replay), so every step is bitwise equal."""
    from k8s_amd.utils.graph import StepGraph

    site = 4
    st1 = _state(cuda, step=30)
    _, body1 = _step_fn(cuda, p, st1, site)
    eager = [tuple(t.clone() for t in body1()) for _ in range(4)]
    st2 = _state(cuda, step=30)
    _, body2 = _step_fn(cuda, p, st2, site)
    g = StepGraph(body2, _NoOptimizer(), warmup=1)
    graphed = [tuple(t.clone() for t in g((), 0.0)) for _ in range(4)]
    torch.cuda.synchronize()
    assert g.replays == 2 and st1.step == st2.step == 34
    for a, b in zip(eager, graphed):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert not torch.equal(eager[2][0], eager[3][0])


# --------------------------------------------------------------------------------------------- model level
def _bert256_pair(cuda, dropout):
    """A two-layer BERT at batch 2 x seq 256 on the GPU kernels and on the CPU fp32 references: same weights, batch,
    dropout seed and step."""
    from k8s_amd.models import bert as M
    from k8s_amd.parallel.flat import ParamStore

    cfg = dataclasses.replace(M.BERT_TINY, max_position=256)
    if dropout:
        cfg = dataclasses.replace(cfg, hidden_dropout=dropout, attention_dropout=dropout)

    def make(device):
        model = M.BertForPreTraining(ParamStore(), cfg).finalize(device, grad_dtype=torch.float32, seed=3, pad_to=64)
        model.drop_state = K.DropoutState(77, device)
        return model

    mg, mc = make(cuda), make("cpu")
    mc.store.master.copy_(mg.store.master.cpu())
    mc.store.refresh_lowp()
    gen = torch.Generator(device=cuda)
    gen.manual_seed(1003)
    batch = M.synthetic_batch(cfg, 2, 256, cuda, generator=gen)
    res = []
    for m, b, dt in ((mg, batch, torch.bfloat16), (mc, tuple(t.cpu() for t in batch), torch.float32)):
        m.store.begin_step()
        loss = m(*b, dtype=dt)[0]
        loss.backward()
        m.store.zero_unwritten()
        res.append((loss.float().item(), {p.name: p.grad.float().cpu().clone() for p in m.store.params}))
    assert mg.drop_state.step == mc.drop_state.step == (1 if dropout else 0)
    return res


@gpu
def test_bert_seq256_dropout_matches_cpu(cuda):
    import k8s_amd.ops.attention as A

    before = A.DROPOUT_FALLBACKS
    (l0, g0), (r0, h0) = _bert256_pair(cuda, None)
    (l1, g1), (r1, h1) = _bert256_pair(cuda, 0.1)
    assert A.DROPOUT_FALLBACKS == before
    assert r1 != r0  # dropout changed the reference loss
    assert abs(l1 - r1) < 3e-2 * max(1.0, abs(r1)), (l1, r1)
    bad = []
    for name, r in h1.items():
        if r.norm().item() == 0 or h0[name].norm().item() == 0:
            continue
        err = (g1[name] - r).norm().item() / r.norm().item()
        floor = (g0[name] - h0[name]).norm().item() / h0[name].norm().item()
        print("%s: err %.4f floor %.4f" % (name, err, floor))
        if err > 2.0 * floor + 0.03:
            bad.append((name, round(err, 4), round(floor, 4)))
    assert not bad, bad
