"""ops.nn.ApplyLink and the planning around it: the link's protocol per kind, the forward-known half of each fused
family's contract (``ops.conv.fused_candidate``, shared by the forward's offer and ``_plan_bwd``), and the whole
decision table of ``conv_bwd`` -- family dispatched, apply pass run first or not, the counter it is counted under --
against the values recorded from the commit before the link kinds were made explicit (tests/golden/apply_link_plan.json).
Nothing launches: small CPU tensors, a stub in place of the extension, ``_hip`` answering yes."""
import hashlib
import itertools
import json
import os
import types

import pytest
import torch

from k8s_amd.ops import conv as kc
from k8s_amd.ops import nn as K

N, H = 2, 4
SWITCHES = ("K8S_AMD_BWD1X1_FUSED", "K8S_AMD_BN3_ONLOAD", "K8S_AMD_DUAL_ONLOAD", "K8S_AMD_CONV1_FUSED")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "apply_link_plan.json")


class _Stop(Exception):
    """The decision is made: the stub's first kernel launch ends the backward."""


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU, so that ``conv_bwd`` takes the extension's side."""
    is_cuda = property(lambda self: True)


def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


class _Ext:
    """The predicates the planners ask, by shape as the extension answers them; ``off`` names one that says no. Any
    other attribute is a kernel: ``bn_bwd_apply`` is noted and returns a new gradient, the rest end the backward."""
    conv_stat_replicas = 1
    conv3x3_w4_use = None

    def __init__(self, off=None):
        self.off, self.applied = off, 0

    def bwd1x1_fused_ok(self, M, c, k):
        return self.off != "bwd1x1_fused_ok" and (c, k) in ((64, 256), (128, 512))

    def bwd1x1_final_ok(self, M, c, k):
        return self.off != "bwd1x1_final_ok" and (c, k) == (64, 256)

    def conv1_fused_ok(self, M, w, n):
        return self.off != "conv1_fused_ok" and (w, n) in ((64, 256), (128, 512))

    def gemm_short_bnstats_ok(self, M, n, k, dual):
        return k <= 128

    def gemm_dgrad_bnstats_ok(self, M, n, k):
        return True

    def conv3x3_staged_ok(self, *a):
        return False

    def bn_bwd_apply(self, gy, x, mask, params):
        self.applied += 1
        return torch.zeros_like(gy)

    def __getattr__(self, name):
        def kernel(*a, **kw):
            raise _Stop(name)
        return kernel


# ------------------------------------------------------------------------------------------- the link's own protocol
def _filled(kind, dy, x, mask, params):
    link = K.ApplyLink()
    link.offer(x)
    if kind == "relu":
        link.fill_relu(dy, x, params)
    else:
        getattr(link, "fill_" + kind)(dy, x, mask, params)
    return link


@pytest.mark.parametrize("kind", ["mask", "dual", "relu"])
def test_link_protocol_per_kind(kind):
    x, other = torch.zeros(4, 8), torch.zeros(4, 8)
    link = K.ApplyLink()
    assert link.kind is None and not link.offered(x) and link.take() is None
    link.offer(x)
    assert link.offered(x) and link.offered(x.view_as(x)) and not link.offered(other) and not link.offered(x[:2])
    assert link.kind is None and link.take() is None  # offered, but the BatchNorm has not deferred
    dy, mask, params = torch.ones(4, 8), torch.zeros(4, dtype=torch.uint8), torch.zeros(32)
    link = _filled(kind, dy, x, mask, params)
    assert link.kind == kind and link.offered(x)
    t = link.take()
    assert link.take() is None and link.kind is None and link.x is None and link.params is None  # cleared
    assert link.offered(x)  # ... but for the offer, which is the forward's
    assert t.kind == kind and t.x is x and t.params is params
    assert t.mask is (None if kind == "relu" else mask)  # the relu kind stores no mask: recomputed from x
    assert t.covers(dy) and not t.covers(dy.clone()) and not t.covers(x)
    dy.add_(1.0)  # an in-place change
    assert not t.covers(dy)


def test_kind_table():
    """Per kind: the families that take the link on load, the counter of an apply pass run after all, the switch."""
    assert set(K.APPLY_KINDS) == {"mask", "dual", "relu"}
    assert {k: (v.families, v.apply_stat) for k, v in K.APPLY_KINDS.items()} == {
        "mask": (("fused_1x1", "fused_final"), "bn3_apply"), "dual": (("fused_1x1", "fused_final"), "dual_apply"),
        "relu": (("conv1_fused",), "conv1_apply")}
    assert K.APPLY_KINDS["mask"].defer_on is kc.bn3_onload_on and K.APPLY_KINDS["dual"].defer_on is kc.dual_onload_on
    assert K.APPLY_KINDS["relu"].defer_on is kc.conv1_fused_on and K.bn3_onload_on is kc.bn3_onload_on
    assert all(v.apply_stat in kc.STATS for v in K.APPLY_KINDS.values())


def test_switch_hierarchy(monkeypatch):
    """BWD1X1_FUSED=0 implies BN3_ONLOAD=0 implies DUAL_ONLOAD=0; CONV1_FUSED is on its own. Read per call."""
    fns = (kc.bwd1x1_fused_on, kc.bn3_onload_on, kc.dual_onload_on, kc.conv1_fused_on)
    expect = {None: (1, 1, 1, 1), SWITCHES[0]: (0, 0, 0, 1), SWITCHES[1]: (1, 0, 0, 1), SWITCHES[2]: (1, 1, 0, 1),
              SWITCHES[3]: (1, 1, 1, 0)}
    for off, want in expect.items():
        for s in SWITCHES:
            monkeypatch.setenv(s, "0" if s == off else "1")
        assert tuple(int(f()) for f in fns) == want, off
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    assert all(f() for f in fns)


# ------------------------------------------------------------------------------- offer and plan cannot disagree
def _x_link(kind, x, other_shape=False):
    """A BnStatLink of ``kind`` on x (``other_shape``: filled for another tensor), or None."""
    if kind is None:
        return None
    xs = _t(N, H + 1, H + 1, x.shape[-1]) if other_shape else x
    bits, mean = _t(xs.numel() // 8, dtype=torch.uint8), _t(xs.shape[-1], dtype=torch.float32)
    link = K.BnStatLink()
    if kind == "relu":
        link.fill_relu(xs, mean, mean, mean, mean)
    elif kind == "dual":
        link.fill_dual(xs, bits, mean, xs, mean)
    else:
        getattr(link, "fill_" + kind)(xs, bits, mean)
    return link


FAMILY_CASES = [("fused_1x1", 64, 256), ("fused_1x1", 128, 512), ("fused_final", 64, 256), ("conv1_fused", 256, 64),
                ("conv1_fused", 512, 128)]  # (family, C, K); conv1_fused's (W, N) = (K, C)
X_KIND = {"fused_1x1": "relu", "fused_final": "pool", "conv1_fused": "mask"}
EXT_OK = {"fused_1x1": "bwd1x1_fused_ok", "fused_final": "bwd1x1_final_ok", "conv1_fused": "conv1_fused_ok"}
# each forward-known condition, flipped alone; the last three bind only the families that read a stored x
FLIPS = ["filter", "stride", "padding", "x_contiguous", "x_kind", "x_kind_shape", "ext_ok", "onload", "hip", "slot",
         "x_sub"]


def _family_inputs(family, C, Kc, flip=None):
    """(the forward-side arguments, the backward's) of a convolution in ``family``'s contract, the backward-only
    facts holding, with one forward-known condition flipped."""
    r = 3 if flip == "filter" else 1
    stride = 2 if flip == "stride" else 1
    pad = 1 if flip in ("filter", "padding") else 0
    x = _t(N, H, H, C)
    if flip == "x_contiguous":
        x = _t(N, H, C, H).transpose(2, 3)
    w = _t(Kc, r, r, C)
    Ho = (H + 2 * pad - r) // stride + 1
    gy = _t(N, Ho, Ho, Kc)
    kind = X_KIND[family]
    if flip == "x_kind":
        kind = {"relu": "mask", "pool": "mask", "mask": "dual"}[kind]
    ln = _x_link(kind, x, other_shape=flip == "x_kind_shape")
    onload = (family == "fused_1x1") != (flip == "onload")
    slot_ok = flip not in ("slot", "x_sub")  # an fp32 slot for dw, no subsampled input: conv_bwd's dw_ok
    addend = {"fused_1x1": None, "fused_final": _t(N, H, H, C),
              "conv1_fused": K.MaskedGrad(_t(N, H, H, C), _t(N * H * H * C // 8, dtype=torch.uint8))}[family]
    apply_link = None
    if family == "conv1_fused":
        apply_link = _filled("relu", gy, _t(*gy.shape), None, _t(4 * Kc, dtype=torch.float32)).take()
    ext = _Ext(off=EXT_OK[family] if flip == "ext_ok" else None)
    fwd = (ext, x, w, stride, pad, kc._link_kind(ln, x.shape), slot_ok, onload)
    bwd = (ext, gy, x, w, stride, pad, addend, _t(2 * C, dtype=torch.float32) if onload else None, ln, slot_ok,
           apply_link)
    return fwd, bwd


@pytest.mark.parametrize("family,C,Kc", FAMILY_CASES)
def test_offer_and_plan_cannot_disagree(monkeypatch, family, C, Kc):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    hip = {"yes": True}
    monkeypatch.setattr(kc, "_hip", lambda *ts: hip["yes"])
    fwd, bwd = _family_inputs(family, C, Kc)
    assert kc.fused_candidate(*fwd) == family and kc._plan_bwd(*bwd) == family
    grad_link = {"fused_1x1": None, "fused_final": K.GradLink(shared=True), "conv1_fused": K.GradLink()}[family]
    fwd[1].requires_grad_(family != "fused_1x1")
    assert kc.offer_family(*fwd, grad_link=grad_link) == family
    for flip in FLIPS:
        binds = family != "fused_1x1" or flip not in ("hip", "slot", "x_sub")  # not in that family's contract
        fwd, bwd = _family_inputs(family, C, Kc, flip)
        hip["yes"] = flip != "hip"
        said, planned = kc.fused_candidate(*fwd), kc._plan_bwd(*bwd)
        hip["yes"] = True
        if binds:
            assert said != family and planned != family, flip
        else:
            assert said == family and planned == family, flip


# ------------------------------------------------------------------------------------------- the decision table
FAMILIES = [None, "fused_1x1", "fused_final", "conv1_fused", "stride1", "strided", "aten"]
APPLY_STATS = [None, "bn3_apply", "dual_apply", "conv1_apply"]
ADDENDS = ["none", "tensor", "noncontig", "masked"]
X_KINDS = ["none", "relu", "mask", "dual", "pool", "other_shape"]
CK = [(64, 256), (128, 512), (256, 64), (512, 128), (256, 1024)]
DEFERRED = [None] + [(k, c) for k in ("mask", "dual", "relu") for c in (True, False)]
ALL_ON = (True, True, True, True)


def grid():
    """Every case, in the fixture's order: the whole product of the structural axes with every switch on; under every
    other switch setting the 1x1 / stride-1 cases (no other can reach a fused family or keep a link) that need dx and
    have their weight gradient to form."""
    for sw in itertools.product((True, False), repeat=4):
        for addend, xk, xform, r, stride, ck, dw_ok, need_dx, deferred in itertools.product(
                ADDENDS, X_KINDS, (False, True), (1, 3), (1, 2), CK, (True, False), (True, False), DEFERRED):
            if sw == ALL_ON or (r == 1 and stride == 1 and dw_ok and need_dx):
                yield sw, addend, xk, xform, r, stride, ck, dw_ok, need_dx, deferred


_CACHE = {}


def _shared(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _make_deferred(kind, dy, x, mask, params):
    """The taken link a convolution's backward hands to ``conv_bwd``."""
    return _filled(kind, dy, x, mask, params).take()


def _conv_bwd(gy, x, w, stride, pad, need_dx, p, addend, xform, ln, deferred):
    return kc.conv_bwd(gy, x, w, stride, pad, need_dx, p, addend=addend, xform=xform, bn_link=ln, apply_link=deferred)


def decide(case, state):
    """(family dispatched, apply passes run first, the counter they were counted under) of one ``conv_bwd``."""
    _, addend, xk, xform, r, stride, (C, Kc), dw_ok, need_dx, deferred = case
    pad = r // 2
    Ho = (H + 2 * pad - r) // stride + 1
    x = _shared(("x", C), lambda: _t(N, H, H, C))
    w = _shared(("w", Kc, r, C), lambda: _t(Kc, r, r, C))
    gy = _shared(("gy", Ho, Kc), lambda: _t(N, Ho, Ho, Kc).as_subclass(_OnGpu))
    bits = _shared(("bits", C), lambda: _t(N * H * H * C // 8, dtype=torch.uint8))
    add = {"none": None, "tensor": _shared(("add", C), lambda: _t(N, H, H, C)),
           "noncontig": _shared(("addT", C), lambda: _t(N, H, C, H).transpose(2, 3)),
           "masked": K.MaskedGrad(_shared(("add", C), lambda: _t(N, H, H, C)), bits)}[addend]
    ln = _x_link(None if xk == "none" else "mask" if xk == "other_shape" else xk, x, other_shape=xk == "other_shape")
    xf = _shared(("xf", C), lambda: _t(2 * C, dtype=torch.float32)) if xform else None
    p = types.SimpleNamespace(grad=_shared(("dw", Kc, r, C), lambda: _t(Kc * r * r * C, dtype=torch.float32)),
                              shape=(Kc, r, r, C), written=False) if dw_ok else None
    link = None
    if deferred is not None:
        kind, covering = deferred
        dy = gy if covering else _shared(("gy2", Ho, Kc), lambda: _t(N, Ho, Ho, Kc).as_subclass(_OnGpu))
        mask = None if kind == "relu" else _shared(("bits3", Ho, Kc),
                                                   lambda: _t(N * Ho * Ho * Kc // 8, dtype=torch.uint8))
        link = _make_deferred(kind, dy, _shared(("x3", Ho, Kc), lambda: _t(N, Ho, Ho, Kc)), mask,
                              _shared(("params", Kc), lambda: _t(4 * Kc, dtype=torch.float32)))
    state.ext, state.planned = _Ext(), []
    before = {k: kc.STATS[k] for k in APPLY_STATS[1:]}
    try:
        _conv_bwd(gy, x, w, stride, pad, need_dx, p, add, xf, ln, link)
    except _Stop:
        pass
    except RuntimeError:  # conv_bwd refuses a normalize-on-load product with no fp32 slot: nothing is dispatched
        state.planned = []
    counted = [k for k in APPLY_STATS[1:] if kc.STATS[k] != before[k]]
    applied = state.ext.applied
    assert len(counted) <= 1 and sum(kc.STATS[k] - before[k] for k in counted) == applied <= 1, case
    family = state.planned[-1] if state.planned else None
    return FAMILIES.index(family), applied, APPLY_STATS.index(counted[0] if counted else None)


def _stop(*a, **kw):
    raise _Stop("aten")


def decision_table(monkeypatch):
    """The table as the fixture stores it: three digits per case, in ``grid()``'s order."""
    state = types.SimpleNamespace(ext=None, planned=[])
    plan = kc._plan_bwd

    def noting(*a, **kw):
        state.planned.append(plan(*a, **kw))
        return state.planned[-1]

    monkeypatch.setattr(kc, "_plan_bwd", noting)
    monkeypatch.setattr(kc, "_load", lambda: state.ext)
    monkeypatch.setattr(kc, "_hip", lambda *ts: True)
    monkeypatch.setattr(kc, "_aten_bwd", _stop)
    monkeypatch.setattr(K.MaskedGrad, "materialize", lambda self: self.dy.clone())
    stats, routes, out = dict(kc.STATS), kc.ROUTES.copy(), []
    try:
        for sw, cases in itertools.groupby(grid(), key=lambda case: case[0]):
            for name, on in zip(SWITCHES, sw):
                monkeypatch.setenv(name, "1" if on else "0")
            out += ["%d%d%d" % decide(case, state) for case in cases]
    finally:
        kc.STATS.update(stats)
        kc.ROUTES.clear()
        kc.ROUTES.update(routes)
    return "".join(out)


def grid_digest():
    return hashlib.sha256(repr(list(grid())).encode()).hexdigest()


def test_decision_table_equals_the_recorded_one(monkeypatch):
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["families"] == FAMILIES and gold["apply_stats"] == APPLY_STATS and gold["switches"] == list(SWITCHES)
    assert gold["grid_sha256"] == grid_digest(), "the grid changed: the fixture is for another list of cases"
    table = decision_table(monkeypatch)
    assert len(table) == len(gold["table"]) == 3 * gold["cases"]
    wrong = [(i, case, table[3 * i:3 * i + 3], gold["table"][3 * i:3 * i + 3])
             for i, case in enumerate(grid()) if table[3 * i:3 * i + 3] != gold["table"][3 * i:3 * i + 3]]
    assert not wrong, (len(wrong), wrong[:5])
    # the grid reaches every family (but "aten": ``_hip`` says yes and every channel count is a multiple of 8), keeps
    # and drops links, and counts under every counter
    seen = {table[3 * i:3 * i + 3] for i in range(gold["cases"])}
    assert {FAMILIES[int(s[0])] for s in seen} == set(FAMILIES) - {"aten"} and {int(s[2]) for s in seen} == {0, 1, 2, 3}
