"""Dropout kernels on the GPU (dropout.hip, the DROP forms in norm.hip and attention.hip) against the torch
definition of the counter generator (ops/reference.py): exact masks, fused add & LayerNorm, attention probabilities,
bert_tiny end to end and under whole-step graph capture."""
import math

import pytest
import torch

from k8s_amd.ops import nn as K
from k8s_amd.ops import reference as ref
from k8s_amd.ops.attention import attention, attention_qkv, attention_reference

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD5678


def _C():
    from k8s_amd.ops._ext import load

    return load()


def _close(a, b, tol, what=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    print("%s: max err %g (scale %g, tol %g)" % (what, err, scale, tol))
    assert err <= tol * max(1.0, scale), "%s: max err %g (scale %g)" % (what, err, scale)


def _state(cuda, step=3, seed=SEED):
    st = K.DropoutState(seed, cuda)
    st.set_step(step)
    return st


# --------------------------------------------------------------------------------------------- 6. mask kernel
@pytest.mark.parametrize("row0,R,C,site", [(0, 70, 200, 7), (2 ** 32 - 3, 8, 40, 7), (12345, 1, 8, 7),
                                           (12345, 1, 8, 40)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_matches_reference(cuda, row0, R, C, site, p):
    st = _state(cuda)
    thr, _ = ref.drop_params(p)
    got = _C().dropout_mask(st.tensor, thr, site, row0, R, C)
    want = ref.dropout_keep((SEED, 3), site, row0 + torch.arange(R, dtype=torch.int64), C, p)  # CPU, from the ints
    assert got.dtype == torch.uint8 and tuple(got.shape) == (R, C)
    assert torch.equal(got.cpu().bool(), want)
    # and the reference run on the device from the device state
    assert torch.equal(ref.dropout_keep(st, site, row0 + torch.arange(R, device=cuda), C, p).cpu(), want)


# --------------------------------------------------------------------------------------------- 7. elementwise
@pytest.mark.parametrize("R,D", [(70, 768), (3, 8)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_fwd_bwd_matches_reference(cuda, R, D, p):
    st = _state(cuda, step=9)
    torch.manual_seed(0)
    x = torch.randn(R, D, device=cuda).bfloat16().requires_grad_(True)
    dy = torch.randn(R, D, device=cuda).bfloat16()
    y = K.dropout(x, p, st, 5)
    y.backward(dy)
    keep = ref.dropout_keep((SEED, 9), 5, R, D, p).to(cuda)
    _, scale = ref.drop_params(p)
    assert torch.equal(y.detach(), ref.dropout(x.detach(), keep, scale))
    assert torch.equal(x.grad, ref.dropout(dy, keep, scale))
    assert 0 < keep.sum().item() < R * D or R * D < 64


# --------------------------------------------------------------------------------------------- 8. add & LayerNorm
# (5, 64) smallest; (70, 768) two-launch path, half-idle second chunk, ragged last block; (300, 1024) two-launch path;
# (33, 2048) CPL 4; (16384 + 70, 64) the one-pass fused kernel: NS = 3 without an incoming xsum gradient, NS = 2 with
NORM_CASES = [(5, 64, False), (70, 768, False), (300, 1024, False), (33, 2048, False), (16384 + 70, 64, False),
              (16384 + 70, 64, True)]


@pytest.mark.parametrize("R,D,with_dres", NORM_CASES)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_add_layer_norm(cuda, R, D, with_dres, p):
    C = _C()
    st = _state(cuda, step=2)
    site = 4
    thr, scale = ref.drop_params(p)
    torch.manual_seed(1)
    x = torch.randn(R, D, device=cuda).bfloat16()
    r = torch.randn(R, D, device=cuda).bfloat16()
    g = torch.rand(D, device=cuda) + 0.5
    b = torch.randn(D, device=cuda)
    keep = ref.dropout_keep(st, site, R, D, p)
    y, mean, rstd, xs = C.norm_fwd(x, r, g, b, 1e-5, False, st.tensor, thr, scale, site)
    yr, meanr, rstdr, xsr = ref.dropout_add_norm_fwd(x, r, g, b, 1e-5, keep, scale)
    _close(y, yr, 2e-2, "y")
    _close(rstd, rstdr, 1e-3, "rstd")
    _close(xs, xsr, 2e-2, "xsum")
    assert torch.equal(xs[~keep], r[~keep])  # a dropped element contributes exactly nothing
    dy = torch.randn(R, D, device=cuda).bfloat16()
    dres = torch.randn(R, D, device=cuda).bfloat16() if with_dres else None
    dg, db = torch.empty(D, device=cuda), torch.empty(D, device=cuda)
    dsum = None if with_dres else torch.full((D,), float("nan"), device=cuda)
    dx, da = C.norm_bwd_dropout(dy, xs, g, mean, rstd, dres, dg, db, dsum, st.tensor, thr, scale, site)
    dxr, dar, dgr, dbr, dsumr = ref.dropout_add_norm_bwd(dy, xs, g, meanr, rstdr, dres, keep, scale)
    _close(dx, dxr, 3e-2, "dres_out")
    _close(da, dar, 3e-2, "da")
    _close(dg, dgr, 2e-2, "dgamma")
    _close(db, dbr, 2e-2, "dbeta")
    # the mask itself, exactly: da is zero where dropped and the scaled dx (to bf16 rounding) where kept
    assert (da[~keep] == 0).all()
    kept = da.float()[keep] - dx.float()[keep] * scale
    assert (kept.abs() <= 2.0 ** -6 * (dx.float()[keep].abs() * scale) + 1e-30).all()
    if dsum is not None:
        _close(dsum, dsumr, 2e-2, "dsum")
    # the residual's gradient is what the kernel without dropout returns for the same saved tensors: the same fp32
    # expressions in another instantiation, where only the compiler's multiply-add contraction may differ -- one fp32
    # ulp before rounding, so at most one bf16 ulp (2^-7 relative) per element, 1e-5 on the fp32 column sums
    dg0, db0 = torch.empty(D, device=cuda), torch.empty(D, device=cuda)
    dx0 = C.norm_bwd(dy, xs, g, mean, rstd, dres, dg0, db0, False)
    assert ((dx.float() - dx0.float()).abs() <= 2.0 ** -7 * dx0.float().abs() + 1e-30).all()
    _close(dg, dg0, 1e-5, "dgamma vs plain")
    _close(db, db0, 1e-5, "dbeta vs plain")


def test_layer_norm_dropout_zero_is_plain(cuda):
    from k8s_amd.parallel.flat import ParamStore, init_const

    R, D = 70, 768
    store = ParamStore()
    pg = store.new("g", (D,), init_const(1), decay=False, lowp=False)
    pb = store.new("b", (D,), init_const(0), decay=False, lowp=False)
    store.finalize(cuda, seed=1)
    st = _state(cuda)
    torch.manual_seed(2)
    x0, r0, dy = (torch.randn(R, D, device=cuda).bfloat16() for _ in range(3))
    out = []
    for kw in ({}, {"dropout": (0.0, st, 3)}):
        x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
        store.begin_step()
        y, xs = K.layer_norm(x, pg, pb, 1e-5, residual=r, **kw)
        y.backward(dy)
        store.zero_unwritten()
        out.append((y.detach(), xs.detach(), x.grad, r.grad, store.grad.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------- 9. mask recovery
def _flash(q, k, v, st, p, site, causal=False, lens=None):
    thr, scale = ref.drop_params(p)
    return _C().flash_fwd(q, k, v, causal, lens, 0.125, st.tensor, thr, scale, site)


@pytest.mark.parametrize("B,H,S", [(2, 2, 128), (1, 3, 100), (1, 2, 16)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_forward_mask_recovery(cuda, B, H, S, p):
    """q = k = 0 makes every probability 1 / S; V[key] = e_(key - key0) then shows keep(query, key) as O[query, d] > 0,
    bit for bit, for the keys key0 .. key0 + 63."""
    st, site = _state(cuda, step=5), 7
    keep = ref.attention_keep(st, site, B, H, S, S, p)  # [B, H, S, S]
    z = torch.zeros(B, S, H, 64, device=cuda, dtype=torch.bfloat16)
    for key0 in range(0, S, 64):
        n = min(64, S - key0)
        v = torch.zeros(B, S, H, 64, device=cuda, dtype=torch.bfloat16)
        v[:, key0:key0 + n] = torch.eye(64, device=cuda, dtype=torch.bfloat16)[:n].view(1, n, 1, 64)
        o, _ = _flash(z, z, v, st, p, site)
        got = (o > 0).permute(0, 2, 1, 3)[..., :n]  # [B, H, S, key]
        assert torch.equal(got, keep[..., key0:key0 + n]), (key0, (got != keep[..., key0:key0 + n]).sum().item())
        assert (o.permute(0, 2, 1, 3)[..., n:] == 0).all()


@pytest.mark.parametrize("B,H", [(2, 2), (1, 3), (1, 2)])
@pytest.mark.parametrize("S", [64, 37])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_backward_mask_recovery(cuda, B, H, S, p):
    """dO[query] = e_query (S <= 64) makes dV[key, query] = scale * keep(query, key) / S."""
    C = _C()
    st, site = _state(cuda, step=5), 10
    thr, scale = ref.drop_params(p)
    keep = ref.attention_keep(st, site, B, H, S, S, p)
    z = torch.zeros(B, S, H, 64, device=cuda, dtype=torch.bfloat16)
    v = torch.randn(B, S, H, 64, device=cuda).bfloat16()
    o, lse = C.flash_fwd(z, z, v, False, None, 0.125, st.tensor, thr, scale, site)
    do = torch.zeros_like(o)
    do[:] = torch.eye(64, device=cuda, dtype=torch.bfloat16)[:S].view(1, S, 1, 64)
    _, _, dv = C.flash_bwd(do, z, z, v, o, lse, False, None, 0.125, None, None, st.tensor, thr, scale, site)
    got = (dv > 0).permute(0, 2, 3, 1)[:, :, :S]  # [B, H, query, key]
    assert torch.equal(got, keep), (got != keep).sum().item()
    assert (dv[..., S:] == 0).all()


# --------------------------------------------------------------------------------------------- 10. numerics
ATTN_CASES = [
    # B, S, H, causal, lens
    (2, 128, 2, False, None),
    (3, 77, 4, False, [77, 30, 0]),
    (2, 72, 2, False, [72, 37]),
    (2, 128, 3, True, [128, 65]),
    (2, 100, 4, True, None),
    (1, 16, 2, False, None),
]


def _qkv(cuda, B, S, H, D=64, seed=0):
    torch.manual_seed(seed)
    x = torch.randn(B * S, 3 * H * D, device=cuda).bfloat16()
    g = x.view(B, S, 3 * H, D)
    return x, g.narrow(2, 0, H), g.narrow(2, H, H), g.narrow(2, 2 * H, H)


def _valid(cuda, B, S, lens):
    valid = torch.ones(B, S, 1, 1, device=cuda)
    for bi, n in enumerate(lens or []):
        if n == 0:  # every key masked: the reference gives NaN, the kernel 0
            valid[bi] = 0
    return valid


@pytest.mark.parametrize("B,S,H,causal,lens", ATTN_CASES)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_dropout_fwd_bwd(cuda, B, S, H, causal, lens, p):
    import k8s_amd.ops.attention as A

    D, site = 64, 13
    st = _state(cuda, step=4)
    _, q, k, v = _qkv(cuda, B, S, H)
    kv_lens = torch.tensor(lens, device=cuda, dtype=torch.int32) if lens else None
    scale = 1.0 / math.sqrt(D)
    keep = ref.attention_keep(st, site, B, H, S, S, p)
    _, ks = ref.drop_params(p)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    want = attention_reference(qr, kr, vr, causal, kv_lens, scale, keep, ks)
    qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    before = A.DROPOUT_FALLBACKS
    out = attention(qq, kk, vv, causal=causal, kv_lens=kv_lens, dropout=(p, st, site))
    assert A.DROPOUT_FALLBACKS == before  # the fused kernels ran
    valid = _valid(cuda, B, S, lens)
    _close(out * valid, torch.nan_to_num(want) * valid, 2e-2, "O")
    do = torch.randn_like(out)
    want.backward(do.float())
    out.backward(do)
    _close(qq.grad, torch.nan_to_num(qr.grad), 3e-2, "dQ")
    _close(kk.grad, torch.nan_to_num(kr.grad), 3e-2, "dK")
    _close(vv.grad, torch.nan_to_num(vr.grad), 3e-2, "dV")


@pytest.mark.parametrize("B,S,H,causal,lens", [(3, 128, 4, False, [128, 60, 0]), (2, 77, 3, True, None)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_qkv_dropout_packed_and_bias_grad(cuda, B, S, H, causal, lens, p):
    """attention_qkv with dropout: the packed gradient written in place against the reference, and the BiasLink bias
    gradient (the one-block kernel's column partials) against the column sums of that packed gradient."""
    from k8s_amd.parallel.flat import ParamStore, init_const

    D, site = 64, 16
    st = _state(cuda, step=6)
    x, q, k, v = _qkv(cuda, B, S, H, seed=3)
    kv_lens = torch.tensor(lens, device=cuda, dtype=torch.int32) if lens else None
    store = ParamStore()
    pb = store.new("qkv.bias", (3 * H * D,), init_const(0), decay=False, lowp=False)
    store.finalize(cuda, seed=1)
    link = K.BiasLink()
    link.pb = pb
    leaf = x.clone().requires_grad_(True)
    store.begin_step()
    o = attention_qkv(leaf * 1, B, S, H, H, D, causal=causal, kv_lens=kv_lens, bias_link=link, dropout=(p, st, site))
    do = torch.randn_like(o)
    o.backward(do)
    store.zero_unwritten()
    assert link.done
    _close(pb.grad.reshape(-1), leaf.grad.float().sum(0), 2e-2, "db")
    keep = ref.attention_keep(st, site, B, H, S, S, p)
    _, ks = ref.drop_params(p)
    xr = x.float().requires_grad_(True)
    g = xr.view(B, S, 3 * H, D)
    want = attention_reference(g.narrow(2, 0, H), g.narrow(2, H, H), g.narrow(2, 2 * H, H), causal, kv_lens,
                               1.0 / math.sqrt(D), keep, ks)
    valid = _valid(cuda, B, S, lens)
    _close(o * valid, torch.nan_to_num(want) * valid, 2e-2, "O")
    want.backward(do.float())
    _close(leaf.grad, torch.nan_to_num(xr.grad), 3e-2, "dqkv")


def test_attention_dropout_zero_is_plain(cuda):
    st = _state(cuda)
    _, q, k, v = _qkv(cuda, 2, 100, 2)
    outs = []
    for kw in ({}, {"dropout": (0.0, st, 1)}):
        qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        o = attention(qq, kk, vv, **kw)
        o.backward(torch.ones_like(o))
        outs.append((o.detach(), qq.grad, kk.grad, vv.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_attention_dropout_fallback_is_counted(cuda):
    """S = 200 is outside the one-block kernels: the reference composition with the same mask, counted."""
    import k8s_amd.ops.attention as A

    B, S, H, D, p, site = 1, 200, 2, 64, 0.1, 19
    st = _state(cuda, step=8)
    _, q, k, v = _qkv(cuda, B, S, H)
    keep = ref.attention_keep(st, site, B, H, S, S, p)
    _, ks = ref.drop_params(p)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    want = attention_reference(qr, kr, vr, False, None, 1.0 / math.sqrt(D), keep, ks)
    qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    before = A.DROPOUT_FALLBACKS
    with pytest.warns(UserWarning) if before == 0 else _nullcontext():
        out = attention(qq, kk, vv, dropout=(p, st, site))
    assert A.DROPOUT_FALLBACKS == before + 1
    _close(out, want, 2e-2, "O")
    do = torch.randn_like(out)
    want.backward(do.float())
    out.backward(do)
    _close(qq.grad, qr.grad, 3e-2, "dQ")
    _close(kk.grad, kr.grad, 3e-2, "dK")
    _close(vv.grad, vr.grad, 3e-2, "dV")


class _nullcontext:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


# --------------------------------------------------------------------------------------------- 11. bert_tiny vs CPU
def _bert_pair(cuda, dropout):
    """bert_tiny on the GPU kernels and on the CPU fp32 references: same weights, batch, dropout seed and step."""
    from k8s_amd.models.registry import build

    torch.manual_seed(0)
    wg = build("bert_tiny", cuda, 4, seed=3, dropout=dropout, dropout_seed=77)
    wc = build("bert_tiny", "cpu", 4, seed=3, dropout=dropout, dropout_seed=77)
    wc.store.master.copy_(wg.store.master.cpu())
    wc.store.refresh_lowp()
    batch = wg.batch(0)
    res = []
    for w, b in ((wg, batch), (wc, tuple(t.cpu() for t in batch))):
        w.store.begin_step()
        loss = w.loss(b)
        loss.backward()
        w.store.zero_unwritten()
        res.append((loss.float().item(), {p.name: p.grad.float().cpu().clone() for p in w.store.params}))
    assert wg.model.drop_state.step == wc.model.drop_state.step == (1 if dropout else 0)
    return res


def test_bert_tiny_dropout_matches_cpu(cuda):
    import k8s_amd.ops.attention as A

    before = A.DROPOUT_FALLBACKS
    (l0, g0), (r0, h0) = _bert_pair(cuda, None)
    (l1, g1), (r1, h1) = _bert_pair(cuda, 0.1)
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


# --------------------------------------------------------------------------------------------- 12. graph capture
def test_step_graph_with_dropout_matches_eager(cuda):
    from k8s_amd.models.registry import build
    from k8s_amd.ops.optim import FusedAdam
    from k8s_amd.parallel.ddp import GradReducer
    from k8s_amd.utils.graph import StepGraph

    def make():
        torch.manual_seed(0)
        w = build("bert_tiny", cuda, 4, seed=3, dropout=0.1)
        o = FusedAdam(w.store, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
        red = GradReducer(w.store)

        def body(inputs, lr):
            red.begin_step()
            loss = w.loss(inputs)
            loss.backward()
            red.finish()
            o.step(grad_scale=red.grad_scale, lr=lr)
            return loss

        return w, o, body

    lrs = [1e-3 * (i + 1) for i in range(6)]
    w1, o1, body1 = make()
    eager = [float(body1(w1.batch(i), lr)) for i, lr in enumerate(lrs)]
    w2, o2, body2 = make()
    g = StepGraph(body2, o2, warmup=2)
    graphed = [float(g(w2.batch(i), lr)) for i, lr in enumerate(lrs)]
    torch.cuda.synchronize()
    assert g.replays == 3 and o1.step_count == o2.step_count
    assert w1.model.drop_state.step == w2.model.drop_state.step == 6
    for a, b in zip(eager, graphed):
        assert abs(a - b) <= 2e-2 * max(1.0, abs(a)), (eager, graphed)
    runs = []
    for _ in range(2):
        w3, o3, body3 = make()
        for i, lr in enumerate(lrs):
            body3(w3.batch(i), lr)
        runs.append(w3)
    torch.cuda.synchronize()

    def rel(x, y):
        return ((x.store.master - y.store.master).norm() / x.store.master.norm()).item()

    floor = max(rel(w1, runs[0]), rel(w1, runs[1]), rel(runs[0], runs[1]))
    assert rel(w1, w2) <= max(5 * floor, 2e-3), (rel(w1, w2), floor)
