"""Inference path on the GPU: the tile kernel's folded-BatchNorm epilogue (``conv_bn_act_infer``), the evaluation
metrics kernel (``xent_eval``) and ``ResNet.forward_infer`` against fp32 references."""
import pytest
import torch
import torch.nn.functional as F

from k8s_amd.models import resnet_ref
from k8s_amd.models.resnet import ResNet, resnet_tiny
from k8s_amd.ops import conv as kconv
from k8s_amd.ops import nn as K
from k8s_amd.parallel.flat import ParamStore

pytestmark = pytest.mark.gpu

# tests/test_gemm_conv_gpu.py CONV_CASES + SMALL_C_CASES (N, H, W, C, K, R, stride, pad) and the one-pixel case: M and
# K_out tails, K_out <= 64 (the 256 x 64 tile), K_out = 72 / 40 / 16 / 8, both buffer counts, all three A sources
CASES = [
    (4, 14, 14, 64, 64, 3, 1, 1),
    (2, 28, 28, 128, 128, 3, 2, 1),
    (3, 7, 7, 512, 2048, 1, 1, 0),
    (2, 16, 16, 256, 128, 1, 2, 0),
    (2, 9, 11, 64, 72, 3, 1, 1),
    (2, 32, 32, 8, 64, 7, 2, 3),
    (2, 15, 13, 24, 40, 3, 1, 1),
    (1, 9, 9, 8, 16, 1, 1, 0),
    (1, 1, 1, 64, 8, 1, 1, 0),
]
# the (source, tile, buffers) instantiations those leave out: K-major double-buffered (C > 512) on both tiles, the
# per-tile im2col single-buffered on the 256 x 64 tile, the per-unit im2col double-buffered (R*S*C > 512) on both tiles
# and single-buffered on the 128 x 128 tile
EXTRA_CASES = [
    (1, 5, 5, 1024, 64, 1, 1, 0),
    (1, 5, 5, 1024, 72, 1, 1, 0),
    (2, 8, 8, 64, 64, 1, 2, 0),
    (1, 6, 6, 24, 72, 5, 1, 2),
    (1, 6, 6, 24, 40, 5, 1, 2),
    (1, 9, 9, 8, 72, 3, 1, 1),
]


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-6)).item()


def _ref(x, w, scale, shift, st, pad, res, relu):
    """fp32 convolution of the same bf16 inputs, then * scale + shift (+ res), then ReLU."""
    y = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), None, st, pad).permute(0, 2, 3, 1)
    y = y * scale + shift
    if res is not None:
        y = y + res.float()
    return torch.relu(y) if relu else y


def _infer(*a, **kw):
    with torch.no_grad():
        before = dict(kconv.STATS)
        y = K.conv_bn_act_infer(*a, **kw)
        assert kconv.STATS["hip_infer"] == before["hip_infer"] + 1 and kconv.STATS["aten_infer"] == before["aten_infer"]
    return y


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", CASES + EXTRA_CASES)
def test_epilogue_against_fp32(cuda, case, relu, with_res):
    N, H, W, C, Ko, R, st, pad = case
    torch.manual_seed(5)
    x = torch.randn(N, H, W, C, device=cuda).bfloat16()
    w = (torch.randn(Ko, R, R, C, device=cuda) * 0.05).bfloat16()
    scale = torch.rand(Ko, device=cuda) + 0.5
    shift = torch.randn(Ko, device=cuda) * 0.5
    Ho, Wo = (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1
    res = torch.randn(N, Ho, Wo, Ko, device=cuda).bfloat16() if with_res else None
    y = _infer(x, w, scale, shift, st, pad, residual=res, relu=relu)
    ref = _ref(x, w, scale, shift, st, pad, res, relu)
    assert y.shape == ref.shape and y.dtype == torch.bfloat16
    err = _rel(y, ref)
    print("case %s relu %d res %d: rel err %.3e" % (case, relu, with_res, err))
    assert err < 1e-2, err


def _onehot_case(cuda, N, H, W, C, Ko, R, st, pad, tap):
    """Output channel k copies input channel perm[k] at filter tap ``tap``; small-integer data, scale in {0.5, 1, 2},
    shift in [-2, 2]: every value is exact in bf16, so the kernel must equal the fp32 reference bit for bit."""
    g = torch.Generator(device="cpu").manual_seed(11)
    perm = torch.randperm(Ko, generator=g) % C
    w = torch.zeros(Ko, R, R, C)
    w[torch.arange(Ko), tap[0], tap[1], perm] = 1.0
    x = torch.randint(-8, 9, (N, H, W, C), generator=g).float()
    k = torch.arange(Ko)
    scale = torch.tensor([0.5, 1.0, 2.0])[k % 3]
    shift = (k % 5 - 2).float()
    Ho, Wo = (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1
    res = torch.randint(-8, 9, (N, Ho, Wo, Ko), generator=g).float()
    return (x.to(cuda).bfloat16(), w.to(cuda).bfloat16(), scale.to(cuda), shift.to(cuda), res.to(cuda).bfloat16())


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case,tap", [
    ((2, 9, 11, 64, 72, 1, 1, 0), (0, 0)),   # 1x1, M = 198
    ((2, 9, 11, 64, 40, 1, 1, 0), (0, 0)),
    ((2, 9, 11, 64, 72, 3, 1, 1), (0, 2)),   # 3x3, off-centre tap: the zero padding shows
    ((2, 32, 32, 8, 64, 7, 2, 3), (1, 5)),   # the 7x7 / s2 stem shape
])
def test_exact_indexing(cuda, case, tap, relu):
    N, H, W, C, Ko, R, st, pad = case
    x, w, scale, shift, res = _onehot_case(cuda, N, H, W, C, Ko, R, st, pad, tap)
    for r in (None, res):
        y = _infer(x, w, scale, shift, st, pad, residual=r, relu=relu)
        ref = _ref(x, w, scale, shift, st, pad, r, relu)
        assert torch.equal(y.float(), ref), (y.float() - ref).abs().max().item()


@pytest.mark.parametrize("case", [(2, 9, 11, 64, 72, 1, 1, 0), (2, 9, 11, 64, 72, 3, 1, 1), (1, 9, 9, 8, 16, 1, 1, 0),
                                  (2, 15, 13, 24, 40, 3, 1, 1)])
def test_output_tile_edges(cuda, case):
    """Output and residual each sit in front of a band of NaN rows in one larger buffer: the band after the output
    stays untouched, the band after the residual is never read into y (M % 64 != 0: no NaN in y)."""
    from k8s_amd.ops._ext import load

    N, H, W, C, Ko, R, st, pad = case
    torch.manual_seed(7)
    x = torch.randn(N, H, W, C, device=cuda).bfloat16()
    w = (torch.randn(Ko, R, R, C, device=cuda) * 0.05).bfloat16()
    scale, shift = torch.rand(Ko, device=cuda) + 0.5, torch.randn(Ko, device=cuda)
    Ho, Wo = (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1
    M, band = N * Ho * Wo, 256
    assert M % 64 != 0
    rbuf = torch.full((M + band, Ko), float("nan"), device=cuda, dtype=torch.bfloat16)
    rbuf[:M] = torch.randn(M, Ko, device=cuda).bfloat16()
    res = rbuf[:M].view(N, Ho, Wo, Ko)
    ybuf = torch.full((M + band, Ko), float("nan"), device=cuda, dtype=torch.bfloat16)
    y = ybuf[:M].view(N, Ho, Wo, Ko)
    load().conv_infer(x, w, st, pad, scale, shift, res, True, out=y)
    assert not torch.isnan(y).any()
    assert torch.isnan(rbuf[M:]).all() and torch.isnan(ybuf[M:]).all()
    assert _rel(y, _ref(x, w, scale, shift, st, pad, res, True)) < 1e-2


# ------------------------------------------------------------------------------------------------ model
def _randomise_bns(model, store):
    """bn3's gamma is zero-initialised (it would hide the whole residual branch) and fresh running statistics are
    (0, 1): give every BatchNorm its own gamma, beta, running mean and running variance."""
    g = torch.Generator(device="cpu").manual_seed(3)
    with torch.no_grad():
        for bn in model.batch_norms():
            c = bn.running_mean.numel()
            dev = bn.running_mean.device
            bn.gamma.master.copy_((torch.rand(c, generator=g) * 0.5 + 0.75).to(dev))
            bn.beta.master.copy_((torch.randn(c, generator=g) * 0.1).to(dev))
            bn.running_mean.copy_((torch.randn(c, generator=g) * 0.1).to(dev))
            bn.running_var.copy_((torch.rand(c, generator=g) + 0.5).to(dev))
    store.refresh_lowp()


def _model_check(cuda, model, store, size, s2d):
    _randomise_bns(model, store)
    torch.manual_seed(1)
    img = torch.randn(4, size, size, 3, device=cuda).bfloat16()
    x8 = model.prepare_input(img, s2d=False).contiguous()
    x = model.prepare_input(img, s2d=s2d).contiguous()
    params = {p.name: p.master.detach().float().clone() for p in store.params}
    with torch.no_grad():
        twin = resnet_ref.forward(model, params, x8.float().permute(0, 3, 1, 2), training=False)
    snap = lambda: (store.master.clone(), store.grad.clone(), [b.clone() for b in model.buffers()])  # noqa: E731
    before = snap()
    stats0 = dict(kconv.STATS)
    fused = model.forward_infer(x)
    routed = sum(3 + (b.down is not None) for b in model.blocks) + (0 if x.shape[-1] == 16 else 1)
    assert kconv.STATS["hip_infer"] - stats0["hip_infer"] == routed
    assert kconv.STATS["aten_infer"] == stats0["aten_infer"]
    after = snap()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert all(torch.equal(a, b) for a, b in zip(before[2], after[2]))
    # a broadcast copy of the flat folded tensor gives the same logits
    flat, _ = model.fold_bn()
    assert torch.equal(model.forward_infer(x, flat.clone()), fused)
    model.eval()
    with torch.no_grad():
        plain = model(x)
    model.train()
    err_plain, err_fused = _rel(plain, twin), _rel(fused, twin)
    print("forward_infer vs fp32 eval twin: plain %.3e fused %.3e" % (err_plain, err_fused))
    assert fused.shape == twin.shape
    assert err_fused <= 2 * err_plain, "err_fused %.3e > 2 x err_plain %.3e" % (err_fused, err_plain)


@pytest.mark.parametrize("s2d", [False, True])
def test_forward_infer_resnet(cuda, s2d):
    store = ParamStore()
    model = ResNet(store, (2, 2, 1, 1), 10, width=64).finalize(cuda)
    _model_check(cuda, model, store, 64, s2d)


def test_forward_infer_resnet_tiny(cuda):
    store = ParamStore()
    model = resnet_tiny(store).finalize(cuda)
    _model_check(cuda, model, store, 32, False)


def test_conv_infer_contract(cuda):
    """Outside the contract the binding raises: it never silently takes another path."""
    from k8s_amd.ops._ext import load

    x = torch.randn(1, 4, 4, 8, device=cuda).bfloat16()
    w = torch.randn(12, 1, 1, 8, device=cuda).bfloat16()  # K % 8 != 0
    scale, shift = torch.ones(12, device=cuda), torch.zeros(12, device=cuda)
    with pytest.raises(RuntimeError):
        load().conv_infer(x, w, 1, 0, scale, shift, None, True)
    with pytest.raises(RuntimeError):  # residual of another shape
        load().conv_infer(x, w[:8].contiguous(), 1, 0, scale[:8].contiguous(), shift[:8].contiguous(),
                          torch.zeros(1, 4, 4, 16, device=cuda).bfloat16(), True)
    assert not kconv.infer_ok(x, w, scale, shift)  # (the op then takes the counted ATen composite: test_eval_cpu)
    with pytest.raises(AssertionError):  # an inference op: refuses to run with autograd on
        K.conv_bn_act_infer(x, w[:8].contiguous(), scale[:8].contiguous(), shift[:8].contiguous(), 1, 0)


# ------------------------------------------------------------------------------------------------ xent_eval
def _rank_def(logits, labels, ignore_index=-100):
    lf = logits.float()
    V = lf.shape[1]
    out = torch.full((lf.shape[0],), V, dtype=torch.int32)
    for r in range(lf.shape[0]):
        y = int(labels[r])
        if y == ignore_index:
            continue
        out[r] = int((lf[r] > lf[r, y]).sum()) + int((lf[r, :y] == lf[r, y]).sum())
    return out


def _close(a, b, tol):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    assert err <= tol * max(1.0, scale), "max err %g (scale %g)" % (err, scale)


@pytest.mark.parametrize("R,V,dtype,ld", [(64, 1000, torch.bfloat16, None), (16, 1003, torch.float32, None),
                                          (8, 10, torch.bfloat16, None), (32, 1000, torch.bfloat16, 1024)])
def test_xent_eval(cuda, R, V, dtype, ld):
    torch.manual_seed(2)
    full = (torch.randn(R, ld or V, device=cuda) * 3).to(dtype)
    labels = torch.randint(0, V, (R,), device=cuda)
    labels[1] = -100  # an ignored row
    # a row whose label is tied with three other columns, on both sides of it
    y = V // 2
    labels[2] = y
    full[2, [y - 3, y - 1, y, y + 2 if y + 2 < V else 0]] = full[2].float().max().to(dtype)
    if ld:
        full[:, V:] = 50.0  # padding columns beat every class: they must not be counted
    loss, rank = K.xent_eval(full, labels, valid=V if ld else None)
    logits = full[:, :V]
    assert rank.dtype == torch.int32 and loss.dtype == torch.float32
    want = _rank_def(logits.cpu(), labels.cpu())
    assert torch.equal(rank.cpu(), want)
    assert int(rank[1]) == V and float(loss[1]) == 0.0
    safe = labels.clamp_min(0)
    ref = F.cross_entropy(logits.float(), safe, reduction="none")
    ref[1] = 0.0
    _close(loss, ref, 1e-3)
    # the kernel and the CPU oracle agree (the trainer's CPU path)
    from k8s_amd.ops import reference

    lo, ro = reference.xent_eval(logits.cpu(), labels.cpu())
    assert torch.equal(ro, want)
    _close(lo, ref, 1e-3)
