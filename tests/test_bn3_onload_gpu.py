"""The residual BatchNorm's backward applied on load by the fused 1x1 backward (bwd1x1_fused.hip with x3 / mask /
params): against the same kernel fed the dx3 that the apply pass writes, against fp32 references, and through a
stage-1 bottleneck with K8S_AMD_BN3_ONLOAD on and off."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _C():
    from k8s_amd.ops._ext import load

    return load()


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-6)).item()


# (M, C, K) of tests/test_bwd1x1_fused_gpu.py, for the reasons given there; every one ends in a ragged tile (64 rows
# at K = 256, 32 at K = 512), whose padded rows must not contribute fma(B, x3, D)
SHAPES = [(200, 64, 256), (677, 64, 256), (1000, 128, 512), (66000, 64, 256), (66000, 128, 512)]
_CASES = {}


def _run(C_, c, dscale):
    """Both forms of the kernel, dW overwritten and accumulated, with the D part of params scaled by ``dscale``."""
    M, K = c["dy"].shape
    C = c["x"].shape[1]
    params = c["params"].clone()
    params[2 * K:3 * K] *= dscale
    dx3 = C_.bn_bwd_apply(c["dy"], c["x3"], c["mask"], params)
    bn = (c["xform"], c["gamma"], c["beta"], c["mean"], c["invstd"])
    out = {"dx3": dx3}
    for acc in (False, True):
        for form in ("ref", "new"):
            dw = c["base"].clone() if acc else torch.full((K, C), 7.0, device=dx3.device)
            sums = torch.zeros(C_.conv_stat_replicas, 2, C, device=dx3.device)
            if form == "ref":
                dz = C_.bwd1x1_fused(dx3, c["x"], c["w"], *bn, dw, sums, acc)
            else:
                dz = C_.bwd1x1_fused(c["dy"], c["x"], c["w"], *bn, dw, sums, acc, x3=c["x3"], mask=c["mask"],
                                     params=params)
            out[form, acc] = (dz, dw - c["base"] if acc else dw, sums.sum(0))
    # fp32 references on the materialised bf16 dx3 (tests/test_bwd1x1_fused_gpu.py)
    x, scale, shift = c["x"], c["xform"][:C], c["xform"][C:]
    zf = (x.double() * scale.double() + shift.double()).float()
    z = zf.clamp_min(0.0).bfloat16().float()
    on = zf.bfloat16().float() > 0
    gd = torch.where(on, out["new", False][0].float(), torch.zeros((), device=x.device))
    out["dw_ref"] = dx3.float().t() @ z
    out["s0"] = gd.sum(0)
    out["s1"] = (gd * (x.float() - c["mean"])).sum(0)
    return out


def _case(cuda, M, C, K):
    """Inputs and, per D scale (1 and 1000), every output and reference: computed once per shape."""
    key = (M, C, K)
    if key in _CASES:
        return _CASES[key]
    C_ = _C()
    g = torch.Generator(device=cuda).manual_seed(2000 + M + C)
    c = {"dy": torch.randn(M, K, device=cuda, generator=g).bfloat16(),
         "x3": (torch.randn(M, K, device=cuda, generator=g) * 1.5 + 0.7).bfloat16(),
         "w": (torch.randn(K, C, device=cuda, generator=g) * 0.05).bfloat16(),
         "x": (torch.randn(M, C, device=cuda, generator=g) * 1.5 + 0.2).bfloat16(),
         "base": torch.randn(K, C, device=cuda, generator=g)}
    bits = torch.rand(M, K, device=cuda, generator=g) < 0.5
    rs = 64 if K == 256 else 32
    last = (M - 1) // rs * rs  # first row of the ragged last tile
    assert M % rs and last + 1 < M
    for r0 in (1, last):  # a row of zeros and a row of ones inside the first tile and inside the last
        bits[r0] = False
        bits[r0 + 1] = True
    weights = (2 ** torch.arange(8, device=cuda)).to(torch.int32)
    c["mask"] = (bits.view(M, K // 8, 8).to(torch.int32) * weights).sum(-1).to(torch.uint8).view(-1).contiguous()
    sign = torch.where(torch.rand(K, device=cuda, generator=g) < 0.5, -1.0, 1.0)
    c["params"] = torch.cat([torch.rand(K, device=cuda, generator=g) + 0.5,            # sc
                             sign * (torch.rand(K, device=cuda, generator=g) * 0.2 + 0.05),  # B
                             sign * (torch.rand(K, device=cuda, generator=g) * 0.3 + 0.1),   # D: never zero
                             torch.zeros(K, device=cuda)]).contiguous()
    x = c["x"]
    c["mean"] = x.float().mean(0)
    c["invstd"] = torch.rsqrt(x.float().var(0, unbiased=False) + 1e-5)
    c["gamma"] = torch.rand(C, device=cuda, generator=g) + 0.5
    c["beta"] = torch.randn(C, device=cuda, generator=g) * 0.2
    scale = c["gamma"] * c["invstd"]
    c["xform"] = torch.cat([scale, torch.addcmul(c["beta"], -c["mean"], scale)]).contiguous()
    _CASES[key] = {1: _run(C_, c, 1.0), 1000: _run(C_, c, 1000.0), "bits": bits, "inputs": c}
    return _CASES[key]


@pytest.mark.parametrize("M,C,K", SHAPES)
def test_apply_pass_reference(cuda, M, C, K):
    """The materialised dx3 the other checks build on is bf16(sc * (mask ? dy : 0) + B * x3 + D)."""
    case = _case(cuda, M, C, K)
    c, p = case["inputs"], case["inputs"]["params"].double()
    g = torch.where(case["bits"], c["dy"].double(), torch.zeros((), device=cuda, dtype=torch.float64))
    ref = p[:K] * g + (p[K:2 * K] * c["x3"].double() + p[2 * K:3 * K])
    r = _rel(case[1]["dx3"], ref)
    print("dx3 rel", r)
    assert r < 4e-3  # one bf16 rounding: 2^-9 per element at most


@pytest.mark.parametrize("M,C,K", SHAPES)
def test_onload_dz_bitwise(cuda, M, C, K):
    """dz of the on-load form = dz of the plain form fed the apply pass's dx3, bit for bit, dW written or accumulated:
    the same expression, the same rounding, the same code after the tile."""
    out = _case(cuda, M, C, K)[1]
    for acc in (False, True):
        assert torch.equal(out["new", acc][0], out["ref", acc][0]), acc
    assert out["new", False][0].float().abs().max().item() > 0


@pytest.mark.parametrize("M,C,K", SHAPES)
def test_onload_dw_and_sums(cuda, M, C, K):
    """dW (5e-3) and both BatchNorm-backward sums (1e-3) vs fp32 on the materialised bf16 dx3: the plain form's bounds,
    only the order of the atomics separating the two forms."""
    out = _case(cuda, M, C, K)[1]
    for acc in (False, True):
        _, dw, sums = out["new", acc]
        r, r0, r1 = _rel(dw, out["dw_ref"]), _rel(sums[0], out["s0"]), _rel(sums[1], out["s1"])
        print("acc", acc, "dw rel", r, "sums rel", r0, r1)
        assert r < 5e-3
        assert r0 < 1e-3
        assert r1 < 1e-3


@pytest.mark.parametrize("M,C,K", SHAPES)
def test_onload_padded_rows(cuda, M, C, K):
    """D scaled by 1000: a padded row of the ragged last tile that leaked fma(B, x3, D) into the tile would dominate
    dW and the sums. Same references, same bounds; dz stays bitwise."""
    out = _case(cuda, M, C, K)[1000]
    for acc in (False, True):
        dz, dw, sums = out["new", acc]
        assert torch.equal(dz, out["ref", acc][0]), acc
        r, r0, r1 = _rel(dw, out["dw_ref"]), _rel(sums[0], out["s0"]), _rel(sums[1], out["s1"])
        print("acc", acc, "dw rel", r, "sums rel", r0, r1)
        assert r < 5e-3
        assert r0 < 1e-3
        assert r1 < 1e-3


def test_onload_rejects_bad_operands(cuda):
    C_ = _C()
    c = _case(cuda, 200, 64, 256)["inputs"]
    bn = (c["xform"], c["gamma"], c["beta"], c["mean"], c["invstd"])
    dw = torch.zeros(256, 64, device=cuda)
    sums = torch.zeros(C_.conv_stat_replicas, 2, 64, device=cuda)
    ok = {"x3": c["x3"], "mask": c["mask"], "params": c["params"]}
    for bad in ({"x3": c["x3"][:, :128].contiguous()}, {"mask": c["mask"][:-1].clone()},
                {"params": c["params"][:2 * 256].clone()}, {"x3": None}, {"x3": c["x3"].float()}):
        with pytest.raises(RuntimeError):
            C_.bwd1x1_fused(c["dy"], c["x"], c["w"], *bn, dw, sums, False, **{**ok, **bad})


def _bottleneck(cuda):
    from k8s_amd.models.resnet import Bottleneck
    from k8s_amd.parallel.flat import ParamStore

    store = ParamStore()
    blk = Bottleneck(store, "b", 256, 64, 1, False)
    store.finalize(cuda, seed=21)
    blk = blk.to(cuda).train()
    gen = torch.Generator(device=cuda).manual_seed(22)
    with torch.no_grad():
        for bn in (blk.bn1, blk.bn2, blk.bn3):
            bn.gamma.master.uniform_(0.5, 1.5, generator=gen)
            bn.beta.master.normal_(0.0, 0.3, generator=gen)
    return store, blk


def _step(cuda, forward):
    """One forward + backward of a stage-1-shaped identity bottleneck (tests/test_bwd1x1_fused_gpu.py's); returns
    the input gradient, the parameter gradients and what ``ops.conv`` counted."""
    from k8s_amd.ops import conv as kc

    torch.manual_seed(3)
    x0 = torch.randn(2, 8, 8, 256, device=cuda).bfloat16()
    gy = torch.randn(2, 8, 8, 256, device=cuda).bfloat16()
    store, blk = _bottleneck(cuda)
    stats, routes = dict(kc.STATS), dict(kc.ROUTES)
    store.begin_step()
    x = x0.clone().requires_grad_(True)
    forward(blk, x).backward(gy)
    store.zero_unwritten()
    counts = {k: kc.STATS[k] - stats[k] for k in ("hip_wgrad", "hip_dgrad", "bn3_onload", "bn3_apply")}
    counts["fused_1x1"] = kc.ROUTES["fused_1x1"] - routes.get("fused_1x1", 0)
    return x.grad.clone(), {p.name: p.grad.clone() for p in store.params}, counts


def _agree(a, b):
    (dx1, per1, _), (dx2, per2, _) = a, b
    assert _rel(dx1, dx2) < 1e-2
    assert len(per1) == 9
    for n in per1:
        assert _rel(per1[n], per2[n]) < 1e-2, n


def test_bottleneck_bn3_onload_on_off(cuda, monkeypatch):
    """K8S_AMD_BN3_ONLOAD on and off: the gradients agree, the products are counted the same, and with the switch on
    conv3's backward, on the fused_1x1 route either way, takes bn3's backward on load (STATS["bn3_onload"]) and no
    apply pass runs for bn3 (STATS["bn3_apply"])."""
    runs = {}
    for on in ("1", "0"):
        monkeypatch.setenv("K8S_AMD_BN3_ONLOAD", on)
        runs[on] = _step(cuda, lambda blk, x: blk(x))
    c1, c0 = runs["1"][2], runs["0"][2]
    assert c1["hip_wgrad"] == c0["hip_wgrad"] == 3
    assert c1["hip_dgrad"] == c0["hip_dgrad"] == 3
    assert (c1["fused_1x1"], c1["bn3_onload"], c1["bn3_apply"]) == (1, 1, 0)
    assert (c0["fused_1x1"], c0["bn3_onload"], c0["bn3_apply"]) == (1, 0, 1)
    _agree(runs["1"], runs["0"])


def test_bottleneck_bn3_fallback(cuda, monkeypatch):
    """The link filled, but conv3's backward receives a copy of dy, which the link does not cover: it runs the apply
    pass on what it received and the plain fused form, and the gradients are those of the switch-off run."""
    from k8s_amd.ops import nn as K

    class _CopyGrad(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return t.view_as(t)

        @staticmethod
        def backward(ctx, g):
            return g.clone()

    def forward(blk, x):  # Bottleneck.forward of an identity block, the copy between conv3 and bn3
        link = K.GradLink()
        b3 = K.ApplyLink()
        t = blk.conv1(x, grad_link=link)
        t = K.bn_relu_conv(t, blk.bn1, blk.conv2)
        y3, sums = K.bn_relu_conv(t, blk.bn2, blk.conv3, out_link=b3)
        return blk.bn3((_CopyGrad.apply(y3), sums), residual=x, relu=True, res_link=link, apply_link=b3)

    monkeypatch.setenv("K8S_AMD_BN3_ONLOAD", "1")
    fb = _step(cuda, forward)
    monkeypatch.setenv("K8S_AMD_BN3_ONLOAD", "0")
    off = _step(cuda, lambda blk, x: blk(x))
    assert (fb[2]["fused_1x1"], fb[2]["bn3_onload"], fb[2]["bn3_apply"]) == (1, 0, 1)
    assert fb[2]["hip_wgrad"] == off[2]["hip_wgrad"] and fb[2]["hip_dgrad"] == off[2]["hip_dgrad"]
    _agree(fb, off)
