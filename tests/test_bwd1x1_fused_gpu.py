"""The fused backward of a normalize-on-load 1x1 convolution (bwd1x1_fused.hip: dz, dW and the BatchNorm-backward sums
in one pass over gy and x) against fp32 references, and a stage-1 bottleneck with the path on and off."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _C():
    from k8s_amd.ops._ext import load

    return load()


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-6)).item()


# (M, C, K): fewer rows than workgroups; several tiles and a ragged last one for both LDS layouts; at least two tiles
# per persistent workgroup on 256 CUs (the ring's slot reuse and the accumulators' carry-over)
SHAPES = [(200, 64, 256), (677, 64, 256), (1000, 128, 512), (66000, 64, 256), (66000, 128, 512)]
_CASES = {}


def _case(cuda, M, C, K):
    """Inputs, the kernel's outputs for both `acc` settings and the fp32 references, computed once per shape."""
    key = (M, C, K)
    if key in _CASES:
        return _CASES[key]
    C_ = _C()
    assert C_.bwd1x1_fused_ok(M, C, K)
    g = torch.Generator(device=cuda).manual_seed(1000 + M + C)
    gy = torch.randn(M, K, device=cuda, generator=g).bfloat16()
    w = (torch.randn(K, C, device=cuda, generator=g) * 0.05).bfloat16()
    x = (torch.randn(M, C, device=cuda, generator=g) * 1.5 + 0.2).bfloat16()
    mean = x.float().mean(0)
    invstd = torch.rsqrt(x.float().var(0, unbiased=False) + 1e-5)
    gamma = torch.rand(C, device=cuda, generator=g) + 0.5
    beta = torch.randn(C, device=cuda, generator=g) * 0.2
    scale = gamma * invstd
    shift = torch.addcmul(beta, -mean, scale)
    xform = torch.cat([scale, shift]).contiguous()

    sums = torch.zeros(C_.conv_stat_replicas, 2, C, device=cuda)
    dw = torch.full((K, C), 7.0, device=cuda)
    dz = C_.bwd1x1_fused(gy, x, w, xform, gamma, beta, mean, invstd, dw, sums, False)
    base = torch.randn(K, C, device=cuda, generator=g)
    dw_acc = base.clone()
    sums_acc = torch.zeros_like(sums)
    dz_acc = C_.bwd1x1_fused(gy, x, w, xform, gamma, beta, mean, invstd, dw_acc, sums_acc, True)

    # z as the on-load path rounds it: the fma through float64 (exact product; see tests/test_gemm_conv_gpu.py)
    zf = (x.double() * scale.double() + shift.double()).float()
    z = zf.clamp_min(0.0).bfloat16().float()
    on = zf.bfloat16().float() > 0  # the forward's ReLU decision
    gd = torch.where(on, dz.float(), torch.zeros_like(dz.float()))
    ref = {
        "dz": gy.float() @ w.float(),
        "dw": gy.float().t() @ z,
        "s0": gd.sum(0),
        "s1": (gd * (x.float() - mean)).sum(0),
    }
    out = {"dz": dz, "dw": dw, "sums": sums.sum(0), "dz_acc": dz_acc, "dw_acc": dw_acc, "base": base,
           "sums_acc": sums_acc.sum(0)}
    _CASES[key] = (out, ref)
    return _CASES[key]


@pytest.mark.parametrize("M,C,K", SHAPES)
def test_fused_dz(cuda, M, C, K):
    """dz = gy . w, rounded to bf16 once; the same bits whether dW is written or accumulated."""
    out, ref = _case(cuda, M, C, K)
    r = _rel(out["dz"], ref["dz"])
    print("dz rel", r)
    assert r < 1e-2
    assert torch.equal(out["dz"], out["dz_acc"])


@pytest.mark.parametrize("M,C,K", SHAPES)
def test_fused_dw_overwrites(cuda, M, C, K):
    """acc=False into a buffer pre-filled with 7.0: dW vs fp32 on the materialised bf16 z."""
    out, ref = _case(cuda, M, C, K)
    r = _rel(out["dw"], ref["dw"])
    print("dw rel", r)
    assert r < 5e-3


@pytest.mark.parametrize("M,C,K", SHAPES)
def test_fused_dw_accumulates(cuda, M, C, K):
    """acc=True onto a random base: the difference vs the same reference."""
    out, ref = _case(cuda, M, C, K)
    r = _rel(out["dw_acc"] - out["base"], ref["dw"])
    print("dw acc rel", r)
    assert r < 5e-3


@pytest.mark.parametrize("M,C,K", SHAPES)
def test_fused_bn_sums(cuda, M, C, K):
    """Both sums vs fp32 sums over the stored dz with the forward's ReLU decision."""
    out, ref = _case(cuda, M, C, K)
    for tot in (out["sums"], out["sums_acc"]):
        r0, r1 = _rel(tot[0], ref["s0"]), _rel(tot[1], ref["s1"])
        print("sums rel", r0, r1)
        assert r0 < 1e-3
        assert r1 < 1e-3


def test_fused_rejects_other_shapes(cuda):
    C_ = _C()
    assert not C_.bwd1x1_fused_ok(1000, 64, 512)
    assert not C_.bwd1x1_fused_ok(1000, 256, 1024)
    assert not C_.bwd1x1_fused_ok(0, 64, 256)
    assert not C_.bwd1x1_fused_ok(2 ** 31, 64, 256)
    gy = torch.zeros(64, 512, device=cuda).bfloat16()
    x = torch.zeros(64, 64, device=cuda).bfloat16()
    w = torch.zeros(512, 64, device=cuda).bfloat16()
    v = torch.ones(64, device=cuda)
    with pytest.raises(RuntimeError):
        C_.bwd1x1_fused(gy, x, w, torch.ones(128, device=cuda), v, v, v, v, torch.zeros(512, 64, device=cuda),
                        torch.zeros(C_.conv_stat_replicas, 2, 64, device=cuda), False)


def test_bottleneck_fused_on_off(cuda, monkeypatch):
    """A stage-1-shaped bottleneck (256 -> 64 -> 256, N = 2, 8 x 8), forward and backward with K8S_AMD_BWD1X1_FUSED on
    and off: every parameter gradient and the input gradient agree, and the products are counted the same."""
    from k8s_amd.models.resnet import Bottleneck
    from k8s_amd.ops import conv as kc
    from k8s_amd.parallel.flat import ParamStore

    torch.manual_seed(3)
    x0 = torch.randn(2, 8, 8, 256, device=cuda).bfloat16()
    gy = torch.randn(2, 8, 8, 256, device=cuda).bfloat16()
    runs = []
    for on in (True, False):
        monkeypatch.setenv("K8S_AMD_BWD1X1_FUSED", "1" if on else "0")
        store = ParamStore()
        blk = Bottleneck(store, "b", 256, 64, 1, False)
        store.finalize(cuda, seed=21)
        blk = blk.to(cuda).train()
        gen = torch.Generator(device=cuda).manual_seed(22)
        with torch.no_grad():
            for bn in (blk.bn1, blk.bn2, blk.bn3):
                bn.gamma.master.uniform_(0.5, 1.5, generator=gen)
                bn.beta.master.normal_(0.0, 0.3, generator=gen)
        before = dict(kc.STATS)
        store.begin_step()
        x = x0.clone().requires_grad_(True)
        blk(x).backward(gy)
        store.zero_unwritten()
        counts = {k: kc.STATS[k] - before[k] for k in ("hip_wgrad", "hip_dgrad")}
        runs.append((x.grad.clone(), {p.name: p.grad.clone() for p in store.params}, counts))
    (dx1, per1, c1), (dx2, per2, c2) = runs
    assert c1["hip_wgrad"] == c2["hip_wgrad"] == 3
    assert c1["hip_dgrad"] == c2["hip_dgrad"] == 3
    assert c1 == c2
    assert _rel(dx1, dx2) < 1e-2
    assert len(per1) == 9
    for n in per1:
        assert _rel(per1[n], per2[n]) < 1e-2, n
