"""The relu-kind ApplyLink between an identity block's conv1 and bn1 (offer / fill / covers / take) and
ops.conv._plan_bwd's "conv1_fused" branch with its fallbacks. The planner launches nothing: it is driven with small CPU
tensors, a stub in place of the extension and ``_hip`` answering yes; the CPU model path takes none of it."""
import types

import pytest
import torch

from k8s_amd.ops import conv as kc
from k8s_amd.ops import nn as K

N, H, W, C = 2, 4, 64, 256  # conv1: C -> W channels
SWITCH = "K8S_AMD_CONV1_FUSED"


def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


def _stub(ok=True):
    """The predicates the planners ask; ``ok`` False: an extension without the kernel's shapes."""
    return types.SimpleNamespace(
        conv1_fused_ok=lambda M, w, n: ok and M >= 1 and (w, n) in ((64, 256), (128, 512)),
        bwd1x1_final_ok=lambda M, c, k: False, bwd1x1_fused_ok=lambda M, c, k: False,
        gemm_short_bnstats_ok=lambda M, n, k, dual: True)


def _mask_link(shape=(N, H, H, C), kind="mask"):
    link = K.BnStatLink()
    n = shape[0] * shape[1] * shape[2] * shape[3]
    if kind == "mask":
        link.fill_mask(_t(*shape), _t(n // 8, dtype=torch.uint8), _t(shape[-1], dtype=torch.float32))
    elif kind == "dual":
        link.fill_dual(_t(*shape), _t(n // 8, dtype=torch.uint8), _t(shape[-1], dtype=torch.float32), _t(*shape),
                       _t(shape[-1], dtype=torch.float32))
    return link


def _bn1(gy, w=W, mask=None):
    """bn1's deferred backward as conv1's backward takes it: filled for ``gy``."""
    l = K.ApplyLink()
    if mask is None:
        l.fill_relu(gy, _t(*gy.shape), _t(4 * w, dtype=torch.float32))
    else:
        l.fill_mask(gy, _t(*gy.shape), mask, _t(4 * w, dtype=torch.float32))
    return l.take()


def _plan(monkeypatch, addend="masked", link="mask", bn1="filled", xform=None, stride=1, r=1, w=W, c=C, ok=True,
          dw_ok=True, gy=None):
    monkeypatch.setattr(kc, "_hip", lambda *ts: True)
    gy = _t(N, H // stride, H // stride, w) if gy is None else gy
    x, wt = _t(N, H, H, c), _t(w, r, r, c)
    add = K.MaskedGrad(_t(N, H, H, c), _t(N * H * H * c // 8, dtype=torch.uint8)) if addend == "masked" else addend
    ln = _mask_link((N, H, H, c)) if link == "mask" else link
    b1 = _bn1(gy, w) if bn1 == "filled" else bn1
    return kc._plan_bwd(_stub(ok), gy, x, wt, stride, r // 2, add, xform, ln, dw_ok, b1)


def test_plan_bwd_conv1_family(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    assert _plan(monkeypatch) == "conv1_fused"
    assert _plan(monkeypatch, w=128, c=512) == "conv1_fused"
    # every condition on its own sends it back to the stride-1 planner (whose route is then the parent's)
    assert _plan(monkeypatch, bn1=None) == "stride1"
    assert _plan(monkeypatch, addend=None) == "stride1"
    assert _plan(monkeypatch, addend=_t(N, H, H, C)) == "stride1"  # a materialised residual gradient
    assert _plan(monkeypatch, link=None) == "stride1"
    assert _plan(monkeypatch, link=_mask_link(kind="dual")) == "stride1"  # behind a stage-entry block: not built
    assert _plan(monkeypatch, link=_mask_link((N, H + 1, H + 1, C))) == "stride1"  # filled for another tensor
    assert _plan(monkeypatch, r=3) == "stride1"
    assert _plan(monkeypatch, ok=False) == "stride1"
    assert _plan(monkeypatch, w=256, c=1024) == "stride1"  # stages 3-4
    assert _plan(monkeypatch, dw_ok=False) == "stride1"
    assert _plan(monkeypatch, xform=_t(2 * C, dtype=torch.float32)) == "stride1"
    # a mask-kind link is conv3's: the fused 1x1 family's, never this route's
    gy = _t(N, H, H, W)
    assert _plan(monkeypatch, gy=gy, bn1=_bn1(gy, mask=_t(N * H * H * W // 8, dtype=torch.uint8))) == "stride1"


def test_plan_bwd_conv1_needs_the_untouched_gradient(monkeypatch):
    """The link covers the dz1 bn1 returned: a copy, or an in-place change, is another gradient."""
    monkeypatch.delenv(SWITCH, raising=False)
    gy = _t(N, H, H, W)
    b1 = _bn1(gy)
    assert _plan(monkeypatch, gy=gy, bn1=b1) == "conv1_fused"
    assert _plan(monkeypatch, gy=gy.clone(), bn1=b1) == "stride1"
    gy.add_(1.0)
    assert _plan(monkeypatch, gy=gy, bn1=b1) == "stride1"


def test_switch_read_per_call(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    assert kc.conv1_fused_on() and _plan(monkeypatch) == "conv1_fused"
    monkeypatch.setenv(SWITCH, "0")
    assert not kc.conv1_fused_on() and _plan(monkeypatch) == "stride1"
    monkeypatch.setenv(SWITCH, "1")
    assert kc.conv1_fused_on() and _plan(monkeypatch) == "conv1_fused"


def test_parent_route_and_counters(monkeypatch):
    """What the fallback runs: the data gradient's parent route, under its own name; the route and its counters exist."""
    monkeypatch.setattr(kc, "_hip", lambda *ts: True)
    add = K.MaskedGrad(_t(N, H, H, C), _t(N * H * H * C // 8, dtype=torch.uint8))
    assert kc._plan_dgrad(_stub(), _t(N, H, H, W), _t(W, 1, 1, C), 0, add, _mask_link()) == "short_mask_sums"
    for k in ("conv1_onload", "conv1_apply", "conv1_fused"):
        assert k in kc.STATS
    assert not kc.conv1_fused_shape_ok(types.SimpleNamespace(), 128, 64, 256)  # a stub without the predicate


def test_relu_form_offer_fill_covers_take():
    y1 = torch.zeros(4, 8)
    b1 = K.ApplyLink()
    assert not b1.offered(y1) and b1.take() is None
    b1.offer(y1)
    assert b1.offered(y1) and not b1.offered(y1[:2]) and b1.offered(y1.view_as(y1))
    assert b1.take() is None  # offered, but bn1 has not deferred (the switch off, or bn1 normalised on load)
    dz1, p = torch.ones(4, 8), torch.zeros(32)
    b1.fill_relu(dz1, y1, p)
    t = b1.take()
    assert b1.take() is None  # cleared
    assert t.kind == "relu" and t.mask is None and t.x is y1 and t.params is p
    assert t.covers(dz1) and not t.covers(dz1.clone())
    dz1.add_(1.0)  # an in-place change
    assert not t.covers(dz1)


def test_cpu_identity_block_unchanged():
    """The CPU model path builds the link and offers nothing: an identity block behind a residual BatchNorm runs as
    before."""
    from k8s_amd.models.resnet import BN, Bottleneck
    from k8s_amd.parallel.flat import ParamStore

    torch.manual_seed(0)
    store = ParamStore()
    pre = BN(store, "pre", 64)
    blk = Bottleneck(store, "b", 64, 16, 1, False)
    store.finalize("cpu", seed=3)
    pre.train()
    blk.train()
    before = dict(kc.STATS)
    x = torch.randn(2, 6, 6, 64).requires_grad_(True)
    store.begin_step()
    y = blk(pre(x, residual=torch.randn(2, 6, 6, 64), relu=True))
    y.float().sum().backward()
    assert y.shape == (2, 6, 6, 64) and x.grad is not None and torch.isfinite(x.grad).all()
    assert {k: kc.STATS[k] - before[k] for k in ("conv1_onload", "conv1_apply")} == {"conv1_onload": 0,
                                                                                     "conv1_apply": 0}
