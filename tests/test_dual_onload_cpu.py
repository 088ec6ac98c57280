"""The two ApplyLinks of a stage-1 entry block (offer / fill / covers / take) and ops.conv._plan_bwd's "fused_final"
branch. The planner only reads shapes, so it is driven with meta tensors, a stub in place of the extension and
``_hip`` answering yes; the CPU model path takes none of it."""
import types

import pytest
import torch

from k8s_amd.ops import conv as kc
from k8s_amd.ops import nn as K

N, H, C, KK = 2, 8, 64, 256
BF = dict(device="meta", dtype=torch.bfloat16)


def _t(*shape, **kw):
    return torch.empty(*shape, **{**BF, **kw})


def _stub(final=True):
    return types.SimpleNamespace(bwd1x1_final_ok=lambda M, c, k: final and (c, k) == (64, 256),
                                 bwd1x1_fused_ok=lambda M, c, k: (c, k) in ((64, 256), (128, 512)))


def _pool_link(shape=(N, H, H, C)):
    link = K.BnStatLink()
    link.fill_pool(_t(*shape), _t(N * H * H * shape[-1] // 8, dtype=torch.uint8), _t(shape[-1], dtype=torch.float32))
    return link


def _plan(monkeypatch, addend="tensor", link="pool", xform=None, stride=1, r=1, c=C, k=KK, final=True, dw_ok=True):
    monkeypatch.setattr(kc, "_hip", lambda *ts: True)
    gy, x, w = _t(N, H // stride, H // stride, k), _t(N, H, H, c), _t(k, r, r, c)
    add = _t(N, H, H, c) if addend == "tensor" else addend
    ln = _pool_link((N, H, H, c)) if link == "pool" else link
    return kc._plan_bwd(_stub(final), gy, x, w, stride, r // 2, add, xform, ln, dw_ok)


def test_plan_bwd_final_family(monkeypatch):
    for k in ("K8S_AMD_DUAL_ONLOAD", "K8S_AMD_BN3_ONLOAD", "K8S_AMD_BWD1X1_FUSED"):
        monkeypatch.delenv(k, raising=False)
    assert _plan(monkeypatch) == "fused_final"
    # every condition on its own sends it back to the stride-1 planner
    assert _plan(monkeypatch, addend=None) == "stride1"
    assert _plan(monkeypatch, addend=K.MaskedGrad(_t(N, H, H, C), _t(N * H * H * C // 8, dtype=torch.uint8))) == "stride1"
    assert _plan(monkeypatch, addend=_t(N, H, H, C).transpose(1, 2)) == "stride1"
    assert _plan(monkeypatch, link=None) == "stride1"
    mask_link = K.BnStatLink()
    mask_link.fill_mask(_t(N, H, H, C), _t(N * H * H * C // 8, dtype=torch.uint8), _t(C, dtype=torch.float32))
    assert _plan(monkeypatch, link=mask_link) == "stride1"
    assert _plan(monkeypatch, link=_pool_link((N, H + 1, H + 1, C))) == "stride1"  # filled for another tensor
    assert _plan(monkeypatch, r=3) == "stride1"
    assert _plan(monkeypatch, final=False) == "stride1"
    assert _plan(monkeypatch, c=128, k=512) == "stride1"
    assert _plan(monkeypatch, dw_ok=False) == "stride1"
    assert _plan(monkeypatch, stride=2) != "fused_final"
    assert _plan(monkeypatch, xform=_t(2 * C, dtype=torch.float32)) != "fused_final"


@pytest.mark.parametrize("switch", ["K8S_AMD_DUAL_ONLOAD", "K8S_AMD_BN3_ONLOAD", "K8S_AMD_BWD1X1_FUSED"])
def test_switches_read_per_call(monkeypatch, switch):
    for k in ("K8S_AMD_DUAL_ONLOAD", "K8S_AMD_BN3_ONLOAD", "K8S_AMD_BWD1X1_FUSED"):
        monkeypatch.delenv(k, raising=False)
    assert kc.dual_onload_on() and _plan(monkeypatch) == "fused_final"
    monkeypatch.setenv(switch, "0")
    assert not kc.dual_onload_on() and _plan(monkeypatch) == "stride1"
    monkeypatch.setenv(switch, "1")
    assert kc.dual_onload_on() and _plan(monkeypatch) == "fused_final"


def test_final_data_gradient_keeps_its_route_name(monkeypatch):
    """What conv_bwd counts in ROUTES for a fused_final launch: the name _plan_dgrad gives that data gradient."""
    stub = types.SimpleNamespace(conv3x3_staged_ok=lambda *a: True, gemm_short_bnstats_ok=lambda *a: True,
                                 gemm_dgrad_bnstats_ok=lambda *a: True)
    assert kc._plan_dgrad(stub, _t(N, H, H, KK), _t(KK, 1, 1, C), 0, _t(N, H, H, C), _pool_link()) == "tile_final_sums"
    for k in ("dual_onload", "dual_apply", "fused_final"):
        assert k in kc.STATS


def test_two_links_offer_fill_covers_take():
    y3, yr = torch.zeros(4, 8), torch.zeros(4, 8)
    b3, b3r = K.ApplyLink(), K.ApplyLink()
    assert not b3.offered(y3) and b3.take() is None and b3.kind is None
    b3.offer(y3)
    b3r.offer(yr)
    assert b3.offered(y3) and b3r.offered(yr) and not b3.offered(yr) and not b3r.offered(y3)
    assert not b3.offered(y3[:2]) and b3.offered(y3.view_as(y3))
    assert b3.take() is None  # offered, but the BatchNorm has not deferred
    dy, mask, p, pr = torch.ones(4, 8), torch.zeros(4, dtype=torch.uint8), torch.zeros(32), torch.ones(32)
    b3.fill_dual(dy, y3, mask, p)
    b3r.fill_dual(dy, yr, mask, pr)
    t3, tr = b3.take(), b3r.take()
    assert b3.take() is None and b3r.take() is None  # cleared
    assert t3.kind == tr.kind == "dual" and t3.x is y3 and tr.x is yr and t3.params is p and tr.params is pr
    assert t3.covers(dy) and tr.covers(dy)  # the one dy is both halves' gradient
    assert not t3.covers(dy.clone())
    dy.add_(1.0)  # an in-place change
    assert not t3.covers(dy) and not tr.covers(dy)
    single = K.ApplyLink()
    single.fill_mask(dy, y3, mask, p)
    assert single.take().kind == "mask"


def test_cpu_entry_block_unchanged():
    """The CPU model path builds the links and offers nothing: an entry block's forward and backward run as before."""
    from k8s_amd.models.resnet import Bottleneck
    from k8s_amd.parallel.flat import ParamStore

    torch.manual_seed(0)
    store = ParamStore()
    blk = Bottleneck(store, "b", 64, 16, 1, True)
    store.finalize("cpu", seed=3)
    blk.train()
    before = dict(kc.STATS)
    x = torch.randn(2, 6, 6, 64).requires_grad_(True)
    store.begin_step()
    y = blk(x)
    y.float().sum().backward()
    assert y.shape == (2, 6, 6, 64) and x.grad is not None and torch.isfinite(x.grad).all()
    assert {k: kc.STATS[k] - before[k] for k in ("dual_onload", "dual_apply", "fused_final")} == {
        "dual_onload": 0, "dual_apply": 0, "fused_final": 0}
