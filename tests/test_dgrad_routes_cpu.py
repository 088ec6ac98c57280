"""Which kernel route a convolution's data gradient takes (ops.conv._plan_dgrad / _plan_dgrad_strided), and the
identity check of ops.nn.BnStatLink. The planners only read shapes, so they are driven with meta tensors and a stub in
place of the extension; the expected routes were read off the if-chain the planners replaced."""
import types

import pytest
import torch

from k8s_amd.ops import conv as kc
from k8s_amd.ops import nn as K

N, H, C = 2, 14, 256
BF = dict(device="meta", dtype=torch.bfloat16)


def _t(*shape, **kw):
    return torch.empty(*shape, **{**BF, **kw})


def _stub(staged=True, short=True, short_dual=True, tile_relu=True):
    """The extension's predicates answering what the case says."""
    return types.SimpleNamespace(
        conv3x3_staged_ok=lambda *a: staged,
        gemm_short_bnstats_ok=lambda M, C_, K_, dual: short_dual if dual else short,
        gemm_dgrad_bnstats_ok=lambda *a: tile_relu)


def _link(kind, shape=(N, H, H, C)):
    if kind is None:
        return None
    c = shape[-1]
    x, mask, f = _t(*shape), _t(N * H * H * c // 8, dtype=torch.uint8), lambda: _t(c, dtype=torch.float32)
    link = K.BnStatLink()
    if kind == "relu":
        link.fill_relu(x, f(), f(), f(), f())
    elif kind == "dual":
        link.fill_dual(x, mask, f(), _t(*shape), f())
    else:
        getattr(link, "fill_" + kind)(x, mask, f())
    return link


def _addend(kind, shape=(N, H, H, C)):
    if kind == "masked":
        return K.MaskedGrad(_t(*shape), _t(N * H * H * shape[-1] // 8, dtype=torch.uint8))
    return _t(*shape) if kind == "tensor" else None


# (r, pad, addend, link kind, stub answers, switches turned the other way, expected route)
STRIDE1 = [
    (3, 1, None, "relu", {}, {}, "conv3x3_relu_sums"),
    (3, 1, None, "relu", {}, {"BSTATS_3X3": False}, "implicit_flipped"),
    (3, 1, None, "relu", {"staged": False}, {}, "implicit_flipped"),
    (3, 1, "tensor", "relu", {}, {}, "implicit_flipped"),
    (1, 0, "masked", "mask", {}, {}, "short_mask_sums"),
    (1, 0, "masked", "mask", {}, {"BSTATS_TILE_MASK": False}, "short_mask_sums"),  # no switch of its own
    (1, 0, "masked", "pool", {}, {}, "short_mask_sums"),
    (1, 0, "masked", "mask", {"short": False}, {}, "tile_mask_sums"),
    (1, 0, "masked", "mask", {"short": False}, {"BSTATS_TILE_MASK": False}, "gemm_masked_add"),
    (1, 0, "masked", "dual", {"short_dual": False}, {}, "gemm_masked_add"),
    (1, 0, "masked", "dual", {"short_dual": False}, {"BSTATS_TILE_SHORT": True}, "tile_mask_sums"),
    (1, 0, "masked", "dual", {"short_dual": False, "short": False}, {}, "tile_mask_sums"),
    (1, 0, None, "relu", {}, {}, "tile_relu_sums"),
    (1, 0, None, "relu", {}, {"BSTATS_GEMM": False}, "gemm_plain"),
    (1, 0, None, "relu", {"tile_relu": False}, {}, "gemm_plain"),
    (1, 0, None, "mask", {}, {}, "short_entry_pending"),
    (1, 0, None, "mask", {}, {"BSTATS_ENTRY": False}, "gemm_plain"),
    (1, 0, None, "mask", {"short": False}, {}, "gemm_plain"),
    (1, 0, None, "pool", {}, {}, "gemm_plain"),
    (1, 0, None, "dual", {}, {}, "gemm_plain"),
    (1, 0, "tensor", "pool", {}, {}, "tile_final_sums"),
    (1, 0, "tensor", "mask", {}, {}, "gemm_add"),
    (1, 0, "tensor", None, {}, {}, "gemm_add"),
    (1, 0, "masked", None, {}, {}, "gemm_masked_add"),
    (1, 0, "masked", "relu", {}, {}, "gemm_masked_add"),
    (1, 0, None, None, {}, {}, "gemm_plain"),
]


@pytest.mark.parametrize("r,pad,addend,kind,stub,switches,want", STRIDE1)
def test_stride1_route(monkeypatch, r, pad, addend, kind, stub, switches, want):
    for name, v in switches.items():
        monkeypatch.setattr(kc, name, v)
    got = kc._plan_dgrad(_stub(**stub), _t(N, H, H, 128), _t(128, r, r, C), pad, _addend(addend), _link(kind))
    assert got == want


@pytest.mark.parametrize("r,pad,addend,kind,want", [
    (3, 1, None, "relu", "implicit_flipped"), (1, 0, None, "relu", "gemm_plain"), (1, 0, None, "mask", "gemm_plain"),
    (1, 0, "masked", "mask", "gemm_masked_add"), (1, 0, "masked", "dual", "gemm_masked_add"),
    (1, 0, "tensor", "pool", "gemm_add")])
def test_link_filled_for_another_shape_takes_no_sums(r, pad, addend, kind, want):
    link = _link(kind, (N, H + 2, H + 2, C))  # e.g. tagged on another tensor
    assert kc._plan_dgrad(_stub(), _t(N, H, H, 128), _t(128, r, r, C), pad, _addend(addend), link) == want
    link.take(_t(1))  # the BatchNorm's backward emptied the link: it serves no later data gradient
    assert link.kind is None
    assert kc._plan_dgrad(_stub(), _t(N, H, H, 128), _t(128, r, r, C), pad, _addend(addend), link) == want


def test_tile_mask_route_checks_row_count():
    """M = N * H * W at 2^31: the tile kernel's masked form is not taken (gemm_short's own predicate answers first)."""
    n = 2 ** 31 // (H * H) + 1
    gy, link = _t(n, H, H, 8), K.BnStatLink()
    link.fill_mask(_t(n, H, H, 8), _t(8, dtype=torch.uint8), _t(8, dtype=torch.float32))
    add = K.MaskedGrad(_t(n, H, H, 8), _t(8, dtype=torch.uint8))
    assert kc._plan_dgrad(_stub(short=False), gy, _t(8, 1, 1, 8), 0, add, link) == "gemm_masked_add"
    assert kc._plan_dgrad(_stub(short=True), gy, _t(8, 1, 1, 8), 0, add, link) == "short_mask_sums"


def _pending(link):
    link.deposit_pending(_t(4, 2, link.x.shape[-1], dtype=torch.float32))
    return link


def test_strided_completes_pending_sums():
    link = _pending(_link("mask"))
    gy, w = _t(N, H // 2, H // 2, 512), _t(512, 1, 1, C)
    assert kc._plan_dgrad_strided(gy, w, 2, 0, H, H, _t(N, H, H, C), link) == "parity_complete_sums"
    assert link.pending and link.sums is not None


@pytest.mark.parametrize("case", ["3x3", "no_addend", "addend_strided", "other_shape"])
def test_strided_clears_pending_sums_it_cannot_complete(case):
    link = _pending(_link("mask", (N, H, H, C // 2) if case == "other_shape" else (N, H, H, C)))
    r = 3 if case == "3x3" else 1
    addend = {"no_addend": None, "addend_strided": _t(N, H, H, 2 * C)[..., ::2]}.get(case, _t(N, H, H, C))
    gy, w = _t(N, H // 2, H // 2, 512), _t(512, r, r, C)
    assert kc._plan_dgrad_strided(gy, w, 2, r // 2, H, H, addend, link) == "parity"
    assert not link.pending and link.sums is None


@pytest.mark.parametrize("on,c,k,want", [(True, 128, 128, "parity_relu_sums"), (False, 128, 128, "parity"),
                                         (True, 64, 128, "parity"), (True, 128, 96, "parity")])
def test_strided_relu_route(monkeypatch, on, c, k, want):
    monkeypatch.setattr(kc, "BSTATS_STRIDED", on)
    link = _link("relu", (N, H, H, c))
    gy, w = _t(N, H // 2, H // 2, k), _t(k, 3, 3, c)
    assert kc._plan_dgrad_strided(gy, w, 2, 1, H, H, None, link) == want
    assert kc._plan_dgrad_strided(gy, w, 2, 1, H, H, None, None) == "parity"
    assert kc._plan_dgrad_strided(gy, w, 2, 1, H, H, _t(N, H, H, c), link) == "parity"


def _deposited():
    link, dx, sums = K.BnStatLink(), torch.zeros(2, 3, 3, 8), torch.ones(1, 2, 8)
    link.fill_mask(torch.zeros(2, 3, 3, 8), torch.zeros(18, dtype=torch.uint8), torch.zeros(8))
    link.deposit(sums, None, dx)
    return link, dx, sums


def _cleared(link):
    return all(getattr(link, f) is None for f in ("kind", "x", "mask", "mean", "sums", "sums2", "dy_key"))


def test_link_take_returns_the_sums_for_the_deposited_tensor():
    link, dx, sums = _deposited()
    n0 = kc.STATS["bn_bstats"]
    assert link.covers(dx)
    pre = link.take(dx)
    assert pre is not None and pre[0] is sums and pre[1] is None and _cleared(link)
    assert kc.STATS["bn_bstats"] == n0  # deposits are counted, not takes


def test_link_take_refuses_another_shape():
    link, dx, _ = _deposited()
    other = dx.view(2, 9, 8)  # the same memory and version
    assert not link.covers(other)
    assert link.take(other) is None and _cleared(link)


def test_link_take_refuses_a_tensor_added_to_in_place():
    """A second consumer's gradient added into dx in place keeps its pointer and shape: the sums cover only a part."""
    link, dx, _ = _deposited()
    dx.add_(torch.ones_like(dx))
    assert not link.covers(dx)
    assert link.take(dx) is None and _cleared(link)


def test_link_pending_sums_are_not_taken_until_complete():
    link, dx, sums = _deposited()
    link.deposit_pending(sums)
    assert not link.covers(dx)
    link.complete(dx)
    assert link.covers(dx) and link.take(dx) == (sums, None)
