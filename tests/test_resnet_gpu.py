"""End-to-end ResNet step on the GPU through the HIP kernels, checked against the CPU fp32 path."""
import pytest
import torch
import torch.nn.functional as F

from k8s_amd.models.resnet import resnet_tiny
from k8s_amd.ops import nn as K
from k8s_amd.ops.optim import FusedSGD
from k8s_amd.parallel.ddp import GradReducer
from k8s_amd.parallel.flat import ParamStore

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def no_aten_products():
    """every conv and linear product of these models runs on our kernels (no ATen
    fallback is counted), so the tests exercise the HIP path end to end."""
    from k8s_amd.ops import conv, gemm

    before = dict(conv.STATS)
    gemm.FALLBACKS.clear()
    yield
    aten = {k: conv.STATS[k] - before[k] for k in conv.STATS if k.startswith("aten_")}
    assert not any(aten.values()), aten
    assert gemm.FALLBACKS == {}, gemm.FALLBACKS


def _run(dev, dtype, steps=3):
    torch.manual_seed(0)
    store = ParamStore()
    m = resnet_tiny(store).finalize(dev)
    m.train()
    red = GradReducer(store)
    opt = FusedSGD(store, lr=0.05)
    g = torch.Generator().manual_seed(5)
    x = m.prepare_input(torch.randn(8, 32, 32, 3, generator=g)).to(dev, dtype).contiguous()
    y = torch.randint(0, 10, (8,), generator=g).to(dev)
    losses = []
    for _ in range(steps):
        red.begin_step()
        loss = K.cross_entropy(m(x), y)
        loss.backward()
        red.finish()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, store


def test_resnet_tiny_gpu_matches_cpu(cuda):
    lg, sg = _run(cuda, torch.bfloat16)
    lc, sc = _run("cpu", torch.float32)
    assert all(abs(a - b) < 0.15 * max(1.0, abs(b)) for a, b in zip(lg, lc)), (lg, lc)
    assert lg[-1] < lg[0]


def test_resnet_gradients_match_plain_pytorch_gpu(cuda):
    """bf16 NHWC kernel path (implicit-GEMM convs with fused BN statistics, fused BN+ReLU+residual, residual
    gradient accumulated in conv1's dgrad epilogue) vs an fp32 torch.nn.functional twin on the same weights."""
    from k8s_amd.models.resnet import ResNet
    from k8s_amd.models.resnet_ref import reference_grads
    from k8s_amd.ops import nn as K
    from k8s_amd.parallel.flat import ParamStore

    torch.manual_seed(0)
    store = ParamStore()
    m = ResNet(store, (2, 2, 1, 1), 10, width=64).finalize(cuda, seed=3)
    m.train()
    images = torch.randn(8, 64, 64, 3, device=cuda).bfloat16()
    x = m.prepare_input(images)  # the space-to-depth stem input on the GPU
    assert x.shape[-1] == 16
    x8 = m.prepare_input(images, s2d=False)  # the plain 7x7 stem's input for the reference twin
    y = torch.randint(0, 10, (8,), device=cuda)
    store.begin_step()
    loss = K.cross_entropy(m(x), y)
    loss.backward()
    store.zero_unwritten()
    ref_loss, ref = reference_grads(m, store, x8, y)
    _, stock = reference_grads(m, store, x8, y, autocast_bf16=True)  # stock bf16 autocast: the noise floor
    assert abs(loss.float().item() - ref_loss.item()) < 3e-2 * max(1.0, abs(ref_loss.item()))
    bad = []
    for p in store.params:
        r = ref[p.name].float()
        err = (p.grad.float() - r).norm().item() / (r.norm().item() + 1e-6)
        floor = (stock[p.name].float() - r).norm().item() / (r.norm().item() + 1e-6)
        if err > 2.0 * floor + 0.03:
            bad.append((p.name, round(err, 3), round(floor, 3)))
    assert not bad, bad


def test_stem_space_to_depth_matches_7x7(cuda):
    """stem_conv_s2d (4x4 conv over the 2x2 space-to-depth image) vs the 7x7 / stride-2 / pad-3 convolution of
    the same weight: forward output and the weight gradient mapped back to the 7x7 layout."""
    import torch.nn.functional as F

    from k8s_amd.parallel.flat import ParamStore, init_normal

    torch.manual_seed(2)
    store = ParamStore()
    p = store.new("conv1.weight", (64, 7, 7, 8), init_normal(0.05))
    store.finalize(cuda)
    with torch.no_grad():
        p.master[..., 3:].zero_()
    store.refresh_lowp()
    img = torch.randn(4, 32, 32, 3, device=cuda).bfloat16()
    xs = K.stem_s2d_input(img)
    assert xs.shape == (4, 19, 19, 16)
    store.begin_step()
    y, _ = K.stem_conv_s2d(xs, p)
    g = torch.randn_like(y)
    y.backward(g)
    w = p.master.detach().bfloat16().float().permute(0, 3, 1, 2)[:, :3].clone().requires_grad_(True)
    ref = F.conv2d(img.float().permute(0, 3, 1, 2), w, None, 2, 3)
    ref.backward(g.float().permute(0, 3, 1, 2))
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()  # noqa: E731
    assert rel(y.permute(0, 3, 1, 2), ref) < 1e-2
    dw = p.grad.view(p.shape)
    assert rel(dw[..., :3].permute(0, 3, 1, 2), w.grad) < 1e-2
    assert dw[..., 3:].abs().max().item() == 0.0


@pytest.mark.parametrize("N,H,W", [(2, 224, 224), (3, 64, 64), (2, 70, 64)])
def test_stem_conv_kernel_matches_fp32(cuda, N, H, W):
    """The LDS-tiled s2d stem convolution (stem.hip) against the fp32 PyTorch conv of the same s2d input and 4x4
    weight, and its BatchNorm statistics against the sums of the stored bf16 outputs (H = 70: 35 output rows, a
    partial last row tile)."""
    torch.manual_seed(3)
    C = K._C()
    img = torch.randn(N, H, W, 3, device=cuda).bfloat16()
    xs = K.stem_s2d_input(img)
    w4 = (torch.randn(64, 4, 4, 16, device=cuda) * 0.1).bfloat16()
    s1 = torch.zeros(C.conv_stat_replicas, 2, 64, device=cuda)
    y1 = C.stem_conv_fwd(xs, w4, s1)
    ref = F.conv2d(xs.float().permute(0, 3, 1, 2), w4.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert y1.shape == ref.shape
    assert ((y1.float() - ref).norm() / ref.norm()).item() < 5e-3
    t1 = s1.sum(0)
    yf = y1.float().reshape(-1, 64)
    assert ((t1[0] - yf.sum(0)).abs().max() / yf.sum(0).abs().max()).item() < 1e-3
    assert ((t1[1] - (yf * yf).sum(0)).abs().max() / (yf * yf).sum(0).max()).item() < 1e-3


@pytest.mark.parametrize("N,H,W", [(2, 224, 224), (3, 70, 64)])
def test_stem_wgrad_kernel_matches_fp32(cuda, N, H, W):
    """The LDS-tiled persistent s2d stem weight gradient (stem.hip) against the fp32 PyTorch weight gradient."""
    torch.manual_seed(4)
    C = K._C()
    img = torch.randn(N, H, W, 3, device=cuda).bfloat16()
    xs = K.stem_s2d_input(img)
    Ho, Wo = xs.shape[1] - 3, xs.shape[2] - 3
    dy = torch.randn(N, Ho, Wo, 64, device=cuda).bfloat16()
    d1 = torch.empty(64, 4, 4, 16, device=cuda)
    C.stem_wgrad(xs, dy, d1)
    ref = torch.nn.grad.conv2d_weight(xs.float().permute(0, 3, 1, 2), (64, 16, 4, 4),
                                      dy.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert ((d1 - ref).norm() / ref.norm()).item() < 1e-3


def test_downsample_bn_dual_matches_separate(cuda):
    """bn3 + downsample BN fused into one apply pass (ops.nn.bn_act_dual, ops.nn.BN_DUAL) vs the separate BNs with
    the MaskLink hand-over, both against the fp32 torch twin with non-trivial BN affines (bn3 starts at gamma 0 in
    the model): the fused path's gradient error may not exceed the separate path's beyond bf16 noise, and both
    update the same running statistics. (The two bf16 paths round differently -- the fused pass adds the downsample
    branch in fp32, not through a bf16 tensor -- so they are compared through the reference, not to each other.)"""
    from k8s_amd.models.resnet import ResNet
    from k8s_amd.models.resnet_ref import reference_grads

    def run(dual):
        old = K.BN_DUAL
        K.BN_DUAL = dual
        try:
            torch.manual_seed(0)
            store = ParamStore()
            m = ResNet(store, (1, 2, 1, 1), 10, width=64).finalize(cuda, seed=3)
            with torch.no_grad():
                gen = torch.Generator(device="cpu").manual_seed(11)
                for p in store.params:
                    if "bn" in p.name or "downsample.1" in p.name:
                        p.master.copy_((torch.rand(p.shape, generator=gen) * 0.8 + 0.6 if p.name.endswith("weight")
                                        else torch.randn(p.shape, generator=gen) * 0.1).to(cuda))
            store.refresh_lowp()
            m.train()
            images = torch.randn(16, 64, 64, 3, generator=torch.Generator(device="cpu").manual_seed(1)).to(cuda)
            x = m.prepare_input(images.bfloat16())
            x8 = m.prepare_input(images.bfloat16(), s2d=False)
            y = torch.arange(16, device=cuda) % 10
            store.begin_step()
            loss = K.cross_entropy(m(x), y)
            loss.backward()
            store.zero_unwritten()
            stats = {n: b.clone() for n, b in m.named_buffers() if "running" in n}
            _, ref = reference_grads(m, store, x8, y)
            err = {}
            for p in store.params:
                r = ref[p.name].float()
                err[p.name] = (p.grad.float() - r).norm().item() / (r.norm().item() + 1e-6)
            return loss.item(), err, stats
        finally:
            K.BN_DUAL = old

    l1, e1, s1 = run(True)
    l0, e0, s0 = run(False)
    assert abs(l1 - l0) < 1e-2 * max(1.0, abs(l0)), (l1, l0)
    # relative bound only, floored at 0.5 % (about one bf16 ulp): below that the two paths' errors are forward-
    # rounding noise (the fc bias gradient measured 0.42 % vs 0.66 % after a reordering of the conv epilogue's
    # statistics sums), not a wrong gradient; a wrong gradient on a small-norm parameter shows as tens of percent
    bad = [(n, round(e1[n], 4), round(e0[n], 4)) for n in e0 if e1[n] > 1.5 * max(e0[n], 5e-3)]
    assert not bad, bad
    for n, r in s0.items():
        # the first block's inputs are identical in both runs; later blocks see the other rounding of the residual
        tol = 1e-3 if n.startswith("blocks.0.") else 3e-2
        assert torch.allclose(s1[n], r, rtol=tol, atol=1e-3), (n, (s1[n] - r).abs().max().item())


@pytest.mark.parametrize("half", [1024, 1536])
def test_resnet50_large_batch_indexing_matches_half_batch(cuda, half):
    """Every kernel at the 288-GB-sized batches (2048 / 3072 images: 56 x 56 activations past 2^31 bytes, and past
    2^31 elements at 3072) against the same step at half the batch: a batch made of two copies of the half batch has
    the same BatchNorm statistics, loss and parameter gradients (everything else is per sample), so any 32-bit
    offset overflow in a kernel shows up as a mismatch."""
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(11)
    imgs = torch.randn(half, 224, 224, 3, generator=g).to(cuda).bfloat16()
    y = torch.randint(0, 1000, (half,), generator=g).to(cuda)

    def run(images, labels):
        from k8s_amd.models.resnet import resnet50

        store = ParamStore()
        m = resnet50(store).finalize(cuda, seed=5)
        m.train()
        x = m.prepare_input(images).contiguous()
        store.begin_step()
        loss = K.cross_entropy(m(x), labels)
        loss.backward()
        store.zero_unwritten()
        out = (float(loss.float().item()), store.grad.clone())
        del m, store, x
        torch.cuda.empty_cache()
        return out

    l1, g1 = run(imgs, y)
    l2, g2 = run(torch.cat([imgs, imgs]), torch.cat([y, y]))
    assert abs(l1 - l2) < 1e-3 * max(1.0, abs(l1)), (l1, l2)
    rel = ((g1 - g2).norm() / (g1.norm() + 1e-12)).item()
    assert rel < 2e-2, rel


def test_bn_backward_sums_in_dgrad_epilogue_match_reduction(cuda):
    """BatchNorm-backward sums taken in the data-gradient epilogues (ops.nn.BnStatLink: the residual BNs in the
    identity-block conv1 dgrad, gemm_short.hip EPI 3 / 4; the on-load bn2 in conv3's tile-kernel dgrad, gemm.hip LeanBnBwd)
    against the BatchNorms' own reduction sweeps (ops.nn.BN_BSTATS off), whole model, both against the fp32 torch twin:
    the fused path's error may not exceed the separate path's beyond summation-order noise. (Compared through the
    reference, not to each other: in this net -- every BatchNorm gamma in [0.6, 1.4], bn3 included -- an fp32-ulp
    difference deep in the backward grows to ~5 % at the stem's bn1 bias by the time it gets there.)"""
    from k8s_amd.models.resnet import ResNet
    from k8s_amd.models.resnet_ref import reference_grads
    from k8s_amd.ops import conv as kc

    ONLOAD_STATS = ("bn3_onload", "bn3_apply", "dual_onload", "dual_apply", "fused_final", "conv1_onload",
                    "conv1_apply", "conv1_fused")

    def run(on):
        old = K.BN_BSTATS
        K.BN_BSTATS = on
        try:
            torch.manual_seed(0)
            store = ParamStore()
            m = ResNet(store, (3, 3, 1, 1), 10, width=64).finalize(cuda, seed=3)
            with torch.no_grad():
                gen = torch.Generator(device="cpu").manual_seed(11)
                for p in store.params:
                    if "bn" in p.name or "downsample.1" in p.name:
                        p.master.copy_((torch.rand(p.shape, generator=gen) * 0.8 + 0.6 if p.name.endswith("weight")
                                        else torch.randn(p.shape, generator=gen) * 0.1).to(cuda))
            store.refresh_lowp()
            m.train()
            # batch 4: every conv's statistics replica gets one tile, so the forward is bitwise repeatable
            images = torch.randn(4, 64, 64, 3, generator=torch.Generator(device="cpu").manual_seed(1)).to(cuda)
            x = m.prepare_input(images.bfloat16())
            x8 = m.prepare_input(images.bfloat16(), s2d=False)
            y = torch.arange(4, device=cuda) % 10
            n0, r0, s0 = kc.STATS["bn_bstats"], kc.ROUTES.copy(), dict(kc.STATS)
            store.begin_step()
            loss = K.cross_entropy(m(x), y)
            loss.backward()
            store.zero_unwritten()
            n, routes = kc.STATS["bn_bstats"] - n0, dict(kc.ROUTES - r0)
            onload = {k: kc.STATS[k] - s0[k] for k in ONLOAD_STATS}
            _, ref = reference_grads(m, store, x8, y)
            err = {}
            for p in store.params:
                r = ref[p.name].float()
                err[p.name] = (p.grad.float() - r).norm().item() / (r.norm().item() + 1e-6)
            return loss.item(), err, n, routes, onload
        finally:
            K.BN_BSTATS = old

    l1, e1, n1, routes, onload = run(True)
    l0, e0, n0, _, _ = run(False)
    # s1b0 (dual), s1b1, s2b1, the stage-1/2 bn2 sums in conv3's dgrad, the s1b2 / s2b2 outputs' two-dgrad sums
    assert n0 == 0 and n1 >= 8, (n0, n1)
    # the route every data gradient of the step takes (ops.conv.ROUTES), recorded at the commit before the dispatch was
    # split into planners by tallying its branches: a changed count is a layer moved to another kernel
    assert routes == {"fused_1x1": 6, "gemm_plain": 2, "implicit_flipped": 5, "parity": 4, "parity_complete_sums": 2,
                      "short_entry_pending": 2, "short_mask_sums": 4, "tile_final_sums": 1, "tile_relu_sums": 2}, routes
    # ... and the BatchNorm apply passes deferred to the producing convolution (ops.nn.ApplyLink), recorded at the
    # commit before the link kinds were made explicit: every offer is taken on load, none turns into a fallback apply
    assert onload == {"bn3_onload": 5, "bn3_apply": 0, "dual_onload": 1, "dual_apply": 0, "fused_final": 1,
                      "conv1_onload": 2, "conv1_apply": 0, "conv1_fused": 2}, onload
    assert l1 == l0, (l1, l0)  # the forward is untouched (and deterministic at this size)
    bad = [(k, round(e1[k], 4), round(e0[k], 4)) for k in e0 if e1[k] > 1.5 * e0[k] + 0.02]
    assert not bad, bad


@pytest.mark.parametrize("H,cin,width", [(56, 256, 64), (28, 512, 128), (14, 1024, 256)])
def test_bn_backward_sums_bottleneck_3x3_and_residual(cuda, H, cin, width):
    """One identity bottleneck at a staged-window 3x3 size behind a residual BatchNorm: bn1's sums in the 3x3 conv2
    data-gradient epilogue (conv3x3.hip) and the input BN's sums in conv1's masked-addend dgrad (gemm_short.hip,
    where its contract holds) against the separate reductions (ops.nn.BN_BSTATS off): every gradient, the input's
    included, within fp32 summation-order noise."""
    from k8s_amd.models.resnet import BN, Bottleneck, Conv
    from k8s_amd.ops import conv as kc

    def run(on):
        old = K.BN_BSTATS
        K.BN_BSTATS = on
        try:
            torch.manual_seed(0)
            store = ParamStore()
            pre, bn = Conv(store, "pre", cin, cin, 1), BN(store, "prebn", cin)
            blk = Bottleneck(store, "blk", cin, width, 1, False)
            store.finalize(cuda, seed=5)
            with torch.no_grad():
                gen = torch.Generator(device="cpu").manual_seed(11)
                for p in store.params:
                    if "bn" in p.name:
                        p.master.copy_((torch.rand(p.shape, generator=gen) * 0.8 + 0.6 if p.name.endswith("weight")
                                        else torch.randn(p.shape, generator=gen) * 0.1).to(cuda))
            store.refresh_lowp()
            bn.to(cuda)
            blk.to(cuda)
            g = torch.Generator(device="cpu").manual_seed(2)
            x0 = torch.randn(2, H, H, cin, generator=g).to(cuda).bfloat16().requires_grad_(True)
            r = torch.randn(2, H, H, cin, generator=g).to(cuda).bfloat16()
            gy = torch.randn(2, H, H, cin, generator=g).to(cuda)
            n0 = kc.STATS["bn_bstats"]
            store.begin_step()
            out = blk(bn(pre(x0), residual=r, relu=True))
            (out.float() * gy).sum().backward()
            store.zero_unwritten()
            grads = {p.name: p.grad.float().clone() for p in store.params}
            grads["x0"] = x0.grad.float().clone()
            return grads, kc.STATS["bn_bstats"] - n0
        finally:
            K.BN_BSTATS = old

    g1, n1 = run(True)
    g0, n0 = run(False)
    assert n0 == 0 and n1 >= 1, (n0, n1)
    bad = []
    for name, r in g0.items():
        err = (g1[name] - r).norm().item() / (r.norm().item() + 1e-6)
        if err > 1e-2:
            bad.append((name, round(err, 4)))
    assert not bad, bad


def test_bn_backward_sums_with_second_consumer(cuda):
    """A BatchNorm + ReLU output read by a 3x3 convolution (whose data gradient can take the BatchNorm-backward sums)
    and by a second consumer: autograd adds the two gradients of y -- in place onto the convolution's dx, or into
    another tensor -- so sums taken over the convolution's part alone must not be used (ops.nn.BnStatLink.take).
    ops.nn.BN_BSTATS on against off: x's gradient and the BatchNorm's parameter gradients agree, whichever path ran."""
    from k8s_amd.models.resnet import BN, Conv

    def run(on):
        old = K.BN_BSTATS
        K.BN_BSTATS = on
        try:
            torch.manual_seed(0)
            store = ParamStore()
            bn, conv = BN(store, "bn", 256), Conv(store, "conv", 256, 256, 3)
            store.finalize(cuda, seed=5)
            with torch.no_grad():
                gen = torch.Generator(device="cpu").manual_seed(11)
                bn.gamma.master.copy_((torch.rand(256, generator=gen) * 0.8 + 0.6).to(cuda))
                bn.beta.master.copy_((torch.randn(256, generator=gen) * 0.1).to(cuda))
            store.refresh_lowp()
            bn.to(cuda)
            g = torch.Generator(device="cpu").manual_seed(2)
            x = torch.randn(2, 14, 14, 256, generator=g).to(cuda).bfloat16().requires_grad_(True)
            ga = torch.randn(2, 14, 14, 256, generator=g).to(cuda)
            gb = torch.randn(2, 14, 14, 256, generator=g).to(cuda)
            store.begin_step()
            y = bn(x, relu=True)
            a, _ = conv(y)
            ((a.float() * ga).sum() + (y.float() * gb).sum()).backward()
            store.zero_unwritten()
            return {"x": x.grad.float().clone(), "gamma": bn.gamma.grad.float().clone(),
                    "beta": bn.beta.grad.float().clone()}
        finally:
            K.BN_BSTATS = old

    g1, g0 = run(True), run(False)
    for name, r in g0.items():
        err = (g1[name] - r).norm().item() / (r.norm().item() + 1e-6)
        assert err < 1e-2, (name, err)


def test_fused_subsample_matches_separate_pass(cuda):
    """bn3's apply pass writing y[:, ::2, ::2] for the next (downsample) block (ops.nn.SubLink) against the separate
    subsample pass: bitwise the same loss and gradients (the same bf16 values reach the downsample convolution), and
    the fused tensor actually used."""
    from k8s_amd.models.resnet import ResNet

    def run(fused):
        old = K.SUB2_FUSED
        K.SUB2_FUSED = fused
        try:
            torch.manual_seed(0)
            store = ParamStore()
            m = ResNet(store, (2, 2, 2, 1), 10, width=64).finalize(cuda, seed=3)
            m.train()
            images = torch.randn(4, 64, 64, 3, generator=torch.Generator(device="cpu").manual_seed(1)).to(cuda)
            x = m.prepare_input(images.bfloat16())
            y = torch.arange(4, device=cuda) % 10
            store.begin_step()
            loss = K.cross_entropy(m(x), y)
            loss.backward()
            store.zero_unwritten()
            return loss.item(), {p.name: p.grad.float().clone() for p in store.params}
        finally:
            K.SUB2_FUSED = old

    l1, g1 = run(True)
    l0, g0 = run(False)
    assert l1 == l0
    for name, r in g0.items():
        assert torch.equal(g1[name], r), name
