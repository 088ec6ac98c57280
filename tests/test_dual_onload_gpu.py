"""The stage-1 entry block's two BatchNorm backwards applied on load: the fused 1x1 backward's final form
(bwd1x1_fused.hip with addend / winner_x / winner_bits / winner_mean) against fp64 and, on load, against itself fed the
apply pass's gradient; bn_bwd_dual_params against bn_bwd_dual; and the block behind the stem's BatchNorm +
ReLU + max pool with K8S_AMD_DUAL_ONLOAD on and off."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _C():
    from k8s_amd.ops._ext import load

    return load()


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-6)).item()


# 32-row tiles: (200) a few tiles, most workgroups idle; (677) a ragged tile; (66000) 2063 tiles -- every workgroup wraps
# the ring several times and the walk ends ragged
SHAPES = [(200, 64, 256), (677, 64, 256), (66000, 64, 256)]
RS = 32
_CASES = {}


def _pack(bits):
    weights = (2 ** torch.arange(8, device=bits.device)).to(torch.int32)
    return (bits.view(bits.shape[0], -1, 8).to(torch.int32) * weights).sum(-1).to(torch.uint8).view(-1).contiguous()


def _run(C_, c, dscale):
    """The plain final form fed bn_bwd_apply's gradient and the on-load final form, dW overwritten and accumulated,
    with the D part of params scaled by ``dscale``; fp64 references on the bf16 operands."""
    M, K = c["dy"].shape
    C = c["x"].shape[1]
    dev = c["dy"].device
    params = c["params"].clone()
    params[2 * K:3 * K] *= dscale
    dxr = C_.bn_bwd_apply(c["dy"], c["xr"], c["mask"], params)
    out = {"dxr": dxr}
    for acc in (False, True):
        for form in ("plain", "onload"):
            dw = c["base"].clone() if acc else torch.full((K, C), 7.0, device=dev)
            sums = torch.zeros(C_.conv_stat_replicas, 2, C, device=dev)
            addend = c["addend"].clone()
            fin = {"addend": addend, "winner_x": c["xw"], "winner_bits": c["wbits"], "winner_mean": c["mean"]}
            if form == "plain":
                o = C_.bwd1x1_fused(dxr, c["x"], c["w"], None, None, None, None, None, dw, sums, acc, **fin)
            else:
                o = C_.bwd1x1_fused(c["dy"], c["x"], c["w"], None, None, None, None, None, dw, sums, acc,
                                    x3=c["xr"], mask=c["mask"], params=params, **fin)
            assert o.data_ptr() == addend.data_ptr() and o.shape == addend.shape  # in place over the addend
            out[form, acc] = (o, dw - c["base"] if acc else dw, sums.double().sum(0))
    g64 = dxr.double()
    out["out_ref"] = g64 @ c["w"].double() + c["addend"].double()
    out["dw_ref"] = g64.t() @ c["x"].double()
    for form in ("plain", "onload"):  # the sums are over the stored result
        gd = torch.where(c["bits"], out[form, False][0].double(), torch.zeros((), device=dev, dtype=torch.float64))
        out[form, "s0"] = gd.sum(0)
        out[form, "s1"] = (gd * (c["xw"].double() - c["mean"].double())).sum(0)
    return out


def _case(cuda, M, C, K):
    """Inputs (the recipe of tests/test_bn3_onload_gpu.py plus the addend and the pool winners) and, per D scale (1 and
    1000), every output and reference: computed once per shape."""
    key = (M, C, K)
    if key in _CASES:
        return _CASES[key]
    C_ = _C()
    g = torch.Generator(device=cuda).manual_seed(4000 + M + C)
    c = {"dy": torch.randn(M, K, device=cuda, generator=g).bfloat16(),
         "xr": (torch.randn(M, K, device=cuda, generator=g) * 1.5 + 0.7).bfloat16(),
         "w": (torch.randn(K, C, device=cuda, generator=g) * 0.05).bfloat16(),
         "x": (torch.randn(M, C, device=cuda, generator=g) * 1.5 + 0.2).bfloat16(),
         "addend": torch.randn(M, C, device=cuda, generator=g).bfloat16(),
         "xw": (torch.randn(M, C, device=cuda, generator=g) * 1.5 + 0.4).bfloat16(),
         "base": torch.randn(K, C, device=cuda, generator=g)}
    mbits = torch.rand(M, K, device=cuda, generator=g) < 0.5
    bits = torch.rand(M, C, device=cuda, generator=g) < 0.5
    last = (M - 1) // RS * RS  # first row of the ragged last tile
    assert M % RS and last + 1 < M
    for r0 in (1, last):  # a row of zeros and a row of ones inside the first tile and inside the last
        mbits[r0], bits[r0] = False, False
        mbits[r0 + 1], bits[r0 + 1] = True, True
    c["mask"], c["wbits"], c["bits"] = _pack(mbits), _pack(bits), bits
    sign = torch.where(torch.rand(K, device=cuda, generator=g) < 0.5, -1.0, 1.0)
    c["params"] = torch.cat([torch.rand(K, device=cuda, generator=g) + 0.5,            # sc
                             sign * (torch.rand(K, device=cuda, generator=g) * 0.2 + 0.05),  # B
                             sign * (torch.rand(K, device=cuda, generator=g) * 0.3 + 0.1),   # D: never zero
                             torch.zeros(K, device=cuda)]).contiguous()
    c["mean"] = c["xw"].float().mean(0)
    _CASES[key] = {1: _run(C_, c, 1.0), 1000: _run(C_, c, 1000.0), "inputs": c}
    return _CASES[key]


def _check(out, form):
    """out (one bf16 rounding), dW written and accumulated, both sums: the bounds of tests/test_bwd1x1_fused_gpu.py."""
    for acc in (False, True):
        o, dw, sums = out[form, acc]
        r = (_rel(o, out["out_ref"]), _rel(dw, out["dw_ref"]), _rel(sums[0], out[form, "s0"]),
             _rel(sums[1], out[form, "s1"]))
        print(form, "acc", acc, "out rel %.3g dw rel %.3g sums rel %.3g %.3g" % r)
        assert r[0] < 4e-3
        assert r[1] < 5e-3
        assert r[2] < 1e-3
        assert r[3] < 1e-3


@pytest.mark.parametrize("M,C,K", SHAPES)
def test_plain_final_vs_fp64(cuda, M, C, K):
    """out = bf16(bf16(gy . w) + addend) within one bf16 rounding of fp64 (the issue's 4e-3), dW = gy^T . x with x as
    stored, sums over g = bit ? stored out : 0."""
    out = _case(cuda, M, C, K)[1]
    _check(out, "plain")
    assert torch.equal(out["plain", False][0], out["plain", True][0])
    assert out["plain", False][0].float().abs().max().item() > 0


@pytest.mark.parametrize("M,C,K", SHAPES)
def test_onload_final_vs_plain(cuda, M, C, K):
    """The on-load form against the plain form fed bn_bwd_apply's dxr: out bit for bit, dW and the sums within the
    plain form's bounds."""
    out = _case(cuda, M, C, K)[1]
    for acc in (False, True):
        assert torch.equal(out["onload", acc][0], out["plain", acc][0]), acc
    _check(out, "onload")


@pytest.mark.parametrize("M,C,K", SHAPES)
def test_onload_final_padded_rows(cuda, M, C, K):
    """D scaled by 1000: a padded row of the ragged last tile that leaked fma(B, xr, D) -- or its repeated addend --
    into dW or the sums would dominate them."""
    out = _case(cuda, M, C, K)[1000]
    for acc in (False, True):
        assert torch.equal(out["onload", acc][0], out["plain", acc][0]), acc
    _check(out, "onload")


def test_final_rejects_bad_operands(cuda):
    C_ = _C()
    c = _case(cuda, 200, 64, 256)["inputs"]
    M = 200
    dw = torch.zeros(256, 64, device=cuda)
    sums = torch.zeros(C_.conv_stat_replicas, 2, 64, device=cuda)
    none5 = (None,) * 5

    def fin():
        return {"addend": c["addend"].clone(), "winner_x": c["xw"], "winner_bits": c["wbits"],
                "winner_mean": c["mean"]}

    gy = C_.bn_bwd_apply(c["dy"], c["xr"], c["mask"], c["params"])
    C_.bwd1x1_fused(gy, c["x"], c["w"], *none5, dw, sums, False, **fin())  # the well-formed call
    for bad in ({"addend": None}, {"winner_x": None}, {"winner_bits": None}, {"winner_mean": None},
                {"addend": c["addend"][:, :32].contiguous()}, {"addend": c["addend"][:-1].contiguous()},
                {"addend": c["addend"].float()}, {"winner_x": c["xw"][:-1].contiguous()},
                {"winner_x": c["xw"].float()}, {"winner_bits": c["wbits"][:-1].clone()},
                {"winner_bits": c["wbits"].to(torch.int8)}, {"winner_mean": c["mean"][:32].contiguous()},
                {"winner_mean": c["mean"].double()}, {"addend": c["addend"].t().contiguous().t()}):
        with pytest.raises(RuntimeError):
            C_.bwd1x1_fused(gy, c["x"], c["w"], *none5, dw, sums, False, **{**fin(), **bad})
    # mixed with the xform operands
    xform = torch.zeros(128, device=cuda)
    vec = torch.ones(64, device=cuda)
    with pytest.raises(RuntimeError):
        C_.bwd1x1_fused(gy, c["x"], c["w"], xform, vec, vec, vec, vec, dw, sums, False, **fin())
    with pytest.raises(RuntimeError):
        C_.bwd1x1_fused(gy, c["x"], c["w"], xform, None, None, None, None, dw, sums, False, **fin())
    # neither kind of x side
    with pytest.raises(RuntimeError):
        C_.bwd1x1_fused(gy, c["x"], c["w"], *none5, dw, sums, False)
    # the final form at C = 128
    gy2 = torch.zeros(M, 512, device=cuda).bfloat16()
    x2, w2 = torch.zeros(M, 128, device=cuda).bfloat16(), torch.zeros(512, 128, device=cuda).bfloat16()
    dw2 = torch.zeros(512, 128, device=cuda)
    sums2 = torch.zeros(C_.conv_stat_replicas, 2, 128, device=cuda)
    assert C_.bwd1x1_fused_ok(M, 128, 512) and not C_.bwd1x1_final_ok(M, 128, 512) and C_.bwd1x1_final_ok(M, 64, 256)
    with pytest.raises(RuntimeError):
        C_.bwd1x1_fused(gy2, x2, w2, *none5, dw2, sums2, False, addend=torch.zeros_like(x2),
                        winner_x=torch.zeros_like(x2), winner_bits=torch.zeros(M * 16, device=cuda, dtype=torch.uint8),
                        winner_mean=torch.zeros(128, device=cuda))


def test_dual_params_then_apply_twice_is_dual_from_sums(cuda):
    """bn_bwd_dual_params + bn_bwd_apply per half = bn_bwd_dual, bit for bit: dx, dxr and both BatchNorms' dgamma /
    dbeta (M = 677, K = 256); from the producer's sums and without them."""
    C_ = _C()
    c = _case(cuda, 677, 64, 256)["inputs"]
    M, K = c["dy"].shape
    g = torch.Generator(device=cuda).manual_seed(9)
    x, xr = c["xr"], (torch.randn(M, K, device=cuda, generator=g) * 0.8 - 0.3).bfloat16()

    def vecs():
        gg = torch.Generator(device=cuda).manual_seed(10)
        return [torch.randn(K, device=cuda, generator=gg) * 0.3, torch.rand(K, device=cuda, generator=gg) + 0.5,
                torch.rand(K, device=cuda, generator=gg) + 0.5, torch.randn(K, device=cuda, generator=gg) * 0.2,
                torch.zeros(K, device=cuda), torch.zeros(K, device=cuda)]  # mean invstd gamma beta dgamma dbeta

    R = C_.conv_stat_replicas
    sums = torch.randn(R, 2, K, device=cuda, generator=g)
    sums2 = torch.randn(R, 2, K, device=cuda, generator=g)
    for pre in ((sums, sums2), (None, None)):
        a, ar, b, br = vecs(), vecs(), vecs(), vecs()
        dx, dxr = C_.bn_bwd_dual(c["dy"], c["mask"], x, *a, xr, *ar, *pre)
        params, params_r = C_.bn_bwd_dual_params(c["dy"], c["mask"], x, *b, xr, *br, *pre)
        assert torch.equal(C_.bn_bwd_apply(c["dy"], x, c["mask"], params), dx)
        assert torch.equal(C_.bn_bwd_apply(c["dy"], xr, c["mask"], params_r), dxr)
        for i in (4, 5):
            assert torch.equal(a[i], b[i]) and torch.equal(ar[i], br[i])
            assert a[i].abs().max().item() > 0 and ar[i].abs().max().item() > 0
    with pytest.raises(RuntimeError):  # the two sums come together
        C_.bn_bwd_dual_params(c["dy"], c["mask"], x, *vecs(), xr, *vecs(), sums, None)


# ---------------------------------------------------------------- block level
class _CopyGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g.clone()


def _block_forward(blk, x):
    return blk(x)


def _fallback_forward(blk, x):
    """Bottleneck.forward of an entry block with a gradient copy between each convolution and the dual BatchNorm."""
    from k8s_amd.ops import nn as K

    dlink = K.GradLink(shared=True)
    b3, b3r = K.ApplyLink(), K.ApplyLink()
    dn = blk.down(x, grad_link=dlink, apply_link=b3r)
    t = blk.conv1(x, grad_link=dlink)
    t = K.bn_relu_conv(t, blk.bn1, blk.conv2)
    y3, s3 = K.bn_relu_conv(t, blk.bn2, blk.conv3, out_link=b3)
    return K.bn_act_dual((_CopyGrad.apply(y3), s3), blk.bn3, (_CopyGrad.apply(dn[0]), dn[1]), blk.down_bn,
                         apply_link=b3, apply_link_r=b3r)


def _step(cuda, forward=_block_forward):
    """One forward + backward of the stem's BatchNorm + ReLU + max pool (32x32 -> 16x16, 64 channels) feeding the
    stage-1 entry block, N = 2: the input gradient, the parameter gradients, what ``ops.conv`` counted."""
    from k8s_amd.models.resnet import BN, Bottleneck
    from k8s_amd.ops import conv as kc
    from k8s_amd.ops import nn as K
    from k8s_amd.parallel.flat import ParamStore

    torch.manual_seed(3)
    x0 = (torch.randn(2, 32, 32, 64, device=cuda) * 1.5 + 0.2).bfloat16()
    gy = torch.randn(2, 16, 16, 256, device=cuda).bfloat16()
    store = ParamStore()
    stem = BN(store, "stem", 64)
    blk = Bottleneck(store, "b", 64, 64, 1, True)
    store.finalize(cuda, seed=21)
    stem, blk = stem.to(cuda).train(), blk.to(cuda).train()
    gen = torch.Generator(device=cuda).manual_seed(22)
    with torch.no_grad():
        for bn in (stem, blk.bn1, blk.bn2, blk.bn3, blk.down_bn):
            bn.gamma.master.uniform_(0.5, 1.5, generator=gen)
            bn.beta.master.normal_(0.0, 0.3, generator=gen)
    xf = x0.float().reshape(-1, 64)
    sums = torch.stack([xf.sum(0), (xf * xf).sum(0)]).reshape(1, 2, 64).contiguous()
    stats, routes = dict(kc.STATS), kc.ROUTES.copy()
    store.begin_step()
    x = x0.clone().requires_grad_(True)
    forward(blk, K.bn_relu_maxpool((x, sums), stem)).backward(gy)
    store.zero_unwritten()
    counts = {k: kc.STATS[k] - stats[k] for k in kc.STATS}
    return x.grad.clone(), {p.name: p.grad.clone() for p in store.params}, counts, dict(kc.ROUTES - routes)


def _agree(a, b):
    (dx1, per1), (dx2, per2) = a[:2], b[:2]
    assert _rel(dx1, dx2) < 1e-2
    assert len(per1) == 14
    for n in per1:
        assert _rel(per1[n], per2[n]) < 1e-2, n


def _tally(c):
    return c["dual_onload"], c["dual_apply"], c["bn3_onload"]


def test_entry_block_dual_onload_on_off(cuda, monkeypatch):
    """K8S_AMD_DUAL_ONLOAD on and off: the gradients agree, the route tallies are equal, and with the switch on the
    dual BatchNorm's backward defers both halves, conv3's and the downsample's backwards take them on load, and no
    apply pass runs."""
    runs = {}
    for on in ("1", "0"):
        monkeypatch.setenv("K8S_AMD_DUAL_ONLOAD", on)
        runs[on] = _step(cuda)
    (_, _, c1, r1), (_, _, c0, r0) = runs["1"], runs["0"]
    assert r1 == r0 and r1["tile_final_sums"] == 1 and r1["fused_1x1"] == 1, (r1, r0)
    assert _tally(c1) == (1, 0, 1) and _tally(c0) == (0, 0, 0)
    assert (c1["fused_final"], c0["fused_final"]) == (1, 0)
    assert c1["hip_wgrad"] == c0["hip_wgrad"] and c1["hip_dgrad"] == c0["hip_dgrad"]
    assert c1["bn_bstats"] == c0["bn_bstats"]
    _agree(runs["1"], runs["0"])


def test_entry_block_dual_fallback(cuda, monkeypatch):
    """Both links filled, but each convolution's backward receives a copy of dy, which its link does not cover: each
    runs the apply pass on what it received, and the gradients are those of the switch-off run."""
    monkeypatch.setenv("K8S_AMD_DUAL_ONLOAD", "1")
    fb = _step(cuda, _fallback_forward)
    monkeypatch.setenv("K8S_AMD_DUAL_ONLOAD", "0")
    off = _step(cuda)
    assert _tally(fb[2]) == (1, 2, 0)
    assert fb[3] == off[3]
    _agree(fb, off)


def test_entry_block_no_pool_link_no_deferral(cuda, monkeypatch):
    """Without the stem's pool link (K8S_AMD_BN_BSTATS_POOL=0) the downsample convolution cannot take the final form,
    so it does not offer and the dual BatchNorm's backward does not defer."""
    from k8s_amd.ops import nn as K

    monkeypatch.setenv("K8S_AMD_DUAL_ONLOAD", "1")
    monkeypatch.setattr(K, "BSTATS_POOL", False)
    c = _step(cuda)[2]
    assert _tally(c) == (0, 0, 0) and c["fused_final"] == 0
