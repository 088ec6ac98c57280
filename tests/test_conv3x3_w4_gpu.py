"""3x3 convolutions on the 4-wave GEMM with gathered A rows (gemm256.hip ConvGather): forward (stride 1 and 2) with
the BatchNorm-statistics epilogue and the stride-1 data gradient with the BatchNorm-backward sums, against F.conv2d and
its autograd in fp32 on the bf16-rounded inputs. The bindings are called directly, so the fill-the-chip policy does not
apply; every M is a whole number of 256-row tiles with the image boundaries at varying places inside a tile.

The bounds are those of tests/test_gemm_conv_gpu.py for the same comparisons: _rel < 1e-2 for the forward and the data
gradient, < 1e-3 for the statistics and the BatchNorm-backward sums (against fp32 sums over the stored bf16 output). The
padding is also checked per element, where every value is exact in bf16."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _C():
    from k8s_amd.ops._ext import load

    return load()


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-6)).item()


def _nchw(t):
    return t.float().permute(0, 3, 1, 2)


# (N, H, W, C, Kout, stride)
FWD_S1 = [(64, 14, 14, 64, 256, 1), (256, 7, 7, 128, 256, 1), (256, 7, 7, 256, 512, 1), (32, 4, 8, 64, 256, 1)]
FWD_S2 = [(64, 28, 28, 64, 256, 2), (256, 14, 14, 64, 256, 2), (256, 13, 13, 64, 256, 2)]


def _check_stats(stats, y):
    tot, yf = stats.sum(0), y.float().reshape(-1, y.shape[-1])
    print("stats:", _rel(tot[0], yf.sum(0)), _rel(tot[1], (yf * yf).sum(0)))
    assert _rel(tot[0], yf.sum(0)) < 1e-3
    assert _rel(tot[1], (yf * yf).sum(0)) < 1e-3


def _forward_case(cuda, N, H, W, C, K, st):
    C_ = _C()
    assert C_.conv3x3_w4_ok(N, H, W, C, K, st)
    x = torch.randn(N, H, W, C, device=cuda).bfloat16()
    w = (torch.randn(K, 3, 3, C, device=cuda) * 0.05).bfloat16()
    ref = F.conv2d(_nchw(x), _nchw(w), None, st, 1).permute(0, 2, 3, 1)
    y = C_.conv3x3_w4_fwd(x, w, st)
    assert y.shape == ref.shape and y.dtype == torch.bfloat16
    print("fwd:", _rel(y, ref))
    assert _rel(y, ref) < 1e-2
    stats = torch.zeros(C_.conv_stat_replicas, 2, K, device=cuda)
    ys = C_.conv3x3_w4_fwd(x, w, st, stats)
    assert torch.equal(ys, y)  # the fused form stores the plain form's bits
    _check_stats(stats, y)


@pytest.mark.parametrize("N,H,W,C,K,st", FWD_S1 + FWD_S2)
def test_forward_matches_conv2d(cuda, N, H, W, C, K, st):
    torch.manual_seed(0)
    _forward_case(cuda, N, H, W, C, K, st)


def _bn_operands(cuda, shape):
    """The BatchNorm + ReLU that produced the convolution's input: its x, and gamma / beta / mean / invstd."""
    c = shape[-1]
    x = (torch.randn(*shape, device=cuda) * 1.5 + 0.2).bfloat16()
    xf = x.float().reshape(-1, c)
    mean, invstd = xf.mean(0), torch.rsqrt(xf.var(0, unbiased=False) + 1e-5)
    gamma, beta = torch.rand(c, device=cuda) + 0.5, torch.randn(c, device=cuda) * 0.2
    return x, gamma, beta, mean, invstd


def _check_bn_sums(sums, dx, x, gamma, beta, mean, invstd):
    c = dx.shape[-1]
    scale = gamma * invstd
    z = (x.float() * scale + torch.addcmul(beta, -mean, scale)).bfloat16().float()  # the forward's ReLU decision
    g = torch.where(z > 0, dx.float(), torch.zeros_like(dx.float())).reshape(-1, c)
    tot, xc = sums.sum(0), x.float().reshape(-1, c) - mean
    print("bn sums:", _rel(tot[0], g.sum(0)), _rel(tot[1], (g * xc).sum(0)))
    assert _rel(tot[0], g.sum(0)) < 1e-3
    assert _rel(tot[1], (g * xc).sum(0)) < 1e-3


def _dgrad_case(cuda, N, H, W, C, K):
    """The data gradient of a convolution with C input and K output channels: the GEMM's N is C."""
    C_ = _C()
    assert C_.conv3x3_w4_ok(N, H, W, K, C, 1)
    gy = torch.randn(N, H, W, K, device=cuda).bfloat16()
    w = (torch.randn(K, 3, 3, C, device=cuda) * 0.05).bfloat16()
    xr = torch.zeros(N, C, H, W, device=cuda, requires_grad=True)
    F.conv2d(xr, _nchw(w), None, 1, 1).backward(_nchw(gy))
    ref = xr.grad.permute(0, 2, 3, 1)
    wt = C_.conv_dgrad_wtrans(w)
    dx = C_.conv3x3_w4_dgrad(gy, wt)
    assert dx.shape == ref.shape
    print("dgrad:", _rel(dx, ref))
    assert _rel(dx, ref) < 1e-2
    x, gamma, beta, mean, invstd = _bn_operands(cuda, (N, H, W, C))
    sums = torch.zeros(C_.conv_stat_replicas, 2, C, device=cuda)
    dxs = C_.conv3x3_w4_dgrad(gy, wt, x, gamma, beta, mean, invstd, sums)
    assert torch.equal(dxs, dx)
    _check_bn_sums(sums, dx, x, gamma, beta, mean, invstd)


@pytest.mark.parametrize("N,H,W,K,C,st", FWD_S1)  # the stride-1 shapes with C and Kout exchanged
def test_dgrad_matches_autograd(cuda, N, H, W, K, C, st):
    torch.manual_seed(1)
    _dgrad_case(cuda, N, H, W, C, K)


def _tap_counts(H, W, st, cuda):
    """[Ho, Wo]: how many of an output pixel's 9 taps lie inside the H x W image (3x3, pad 1, stride st)."""
    return F.conv2d(torch.ones(1, 1, H, W, device=cuda), torch.ones(1, 1, 3, 3, device=cuda), None, st, 1)[0, 0]


@pytest.mark.parametrize("N,H,W,st", [(256, 7, 7, 1), (32, 4, 8, 1), (256, 14, 14, 2), (256, 13, 13, 2),
                                      (32, 8, 16, 2), (32, 7, 15, 2)])
def test_forward_padding_per_element(cuda, N, H, W, st):
    """x = 1, w = 1, C = 64: every output is exactly 64 x (its taps inside the image) -- 256, 384 and 576 are exact in
    bf16 -- at stride 1 and 2, with 7x7 and 4x8 outputs. A tap that, shifted, lands in the neighbouring row or image
    must read zeros."""
    C_ = _C()
    x = torch.ones(N, H, W, 64, device=cuda, dtype=torch.bfloat16)
    w = torch.ones(256, 3, 3, 64, device=cuda, dtype=torch.bfloat16)
    want = (64 * _tap_counts(H, W, st, cuda))[None, :, :, None]
    stats = torch.zeros(C_.conv_stat_replicas, 2, 256, device=cuda)
    for y in (C_.conv3x3_w4_fwd(x, w, st), C_.conv3x3_w4_fwd(x, w, st, stats)):
        assert torch.equal(y.float(), want.expand_as(y))


@pytest.mark.parametrize("N,H,W", [(256, 7, 7), (32, 4, 8)])
def test_dgrad_padding_per_element(cuda, N, H, W):
    """dy = 1, w = 1, 64 output channels: every dx is exactly 64 x (the taps that reach it from inside the image)."""
    C_ = _C()
    gy = torch.ones(N, H, W, 64, device=cuda, dtype=torch.bfloat16)
    wt = C_.conv_dgrad_wtrans(torch.ones(64, 3, 3, 256, device=cuda, dtype=torch.bfloat16))
    want = (64 * _tap_counts(H, W, 1, cuda))[None, :, :, None]
    dx = C_.conv3x3_w4_dgrad(gy, wt)
    assert torch.equal(dx.float(), want.expand_as(dx))


def _wgrad_ref(x, dy, K, C, st):
    wr = torch.zeros(K, C, 3, 3, device=x.device, requires_grad=True)
    F.conv2d(_nchw(x), wr, None, st, 1).backward(_nchw(dy))
    return wr.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize("N,H,W,C,K,st", [(64, 14, 14, 256, 256, 1), (256, 7, 7, 256, 512, 1), (64, 28, 28, 256, 256, 2)])
def test_wgrad_matches_autograd(cuda, N, H, W, C, K, st):
    """The weight gradient with gathered B rows, stored and accumulated (bound 5e-3, as test_gemm_conv_gpu's). The
    12 544 pixels split into 22 K ranges of 576 with a last one of 448."""
    C_ = _C()
    torch.manual_seed(4)
    assert C_.conv3x3_w4_wgrad_ok(N, H, W, C, K, st)
    ho, wo = (H - 1) // st + 1, (W - 1) // st + 1
    x = torch.randn(N, H, W, C, device=cuda).bfloat16()
    dy = torch.randn(N, ho, wo, K, device=cuda).bfloat16()
    ref = _wgrad_ref(x, dy, K, C, st)
    dw = torch.full((K, 3, 3, C), 7.0, device=cuda)
    C_.conv3x3_w4_wgrad(x, dy, dw, st, False)
    print("wgrad:", _rel(dw, ref))
    assert _rel(dw, ref) < 5e-3
    base = torch.randn(K, 3, 3, C, device=cuda)
    acc = base.clone()
    C_.conv3x3_w4_wgrad(x, dy, acc, st, True)
    assert _rel(acc - base, ref) < 5e-3


@pytest.mark.parametrize("N,H,W,st", [(256, 7, 7, 1), (64, 4, 8, 1), (64, 14, 14, 2), (64, 13, 13, 2)])
def test_wgrad_padding_per_element(cuda, N, H, W, st):
    """dy = 1, x = 1: dw[k][r][s][c] is exactly the number of output pixels whose tap (r, s) lies inside the image
    (at most 12 544 here, far below 2^24: every partial sum is an exact fp32 integer)."""
    C_ = _C()
    ho, wo = (H - 1) // st + 1, (W - 1) // st + 1
    x = torch.ones(N, H, W, 256, device=cuda, dtype=torch.bfloat16)
    dy = torch.ones(N, ho, wo, 256, device=cuda, dtype=torch.bfloat16)
    ref = _wgrad_ref(x, dy, 256, 256, st)
    assert ref.max().item() <= N * ho * wo < 2 ** 24
    dw = torch.empty(256, 3, 3, 256, device=cuda)
    C_.conv3x3_w4_wgrad(x, dy, dw, st, False)
    assert torch.equal(dw, ref)


def test_wgrad_routing_and_switch(cuda, monkeypatch):
    """conv_wgrad takes the route for a chip-filling 3x3 layer, K8S_AMD_CONV3X3_W4=0 restores the kernels it had."""
    C_ = _C()
    torch.manual_seed(5)
    N, H, C, K = 256, 7, 256, 256
    x = torch.randn(N, H, H, C, device=cuda).bfloat16()
    dy = torch.randn(N, H, H, K, device=cuda).bfloat16()
    assert C_.conv3x3_w4_wgrad_use(N, H, H, C, K, 1)
    direct, on, off = (torch.empty(K, 3, 3, C, device=cuda) for _ in range(3))
    C_.conv3x3_w4_wgrad(x, dy, direct, 1, False)
    C_.conv_wgrad(x, dy, on, 1, 1, 1, 0, False)
    monkeypatch.setenv("K8S_AMD_CONV3X3_W4", "0")
    assert not C_.conv3x3_w4_wgrad_use(N, H, H, C, K, 1)
    C_.conv_wgrad(x, dy, off, 1, 1, 1, 0, False)
    assert torch.equal(on, direct)  # the same launch
    # another kernel's fp32 summation order: 12 544 terms, fp32 eps 6e-8 x sqrt(12 544) ~ 7e-6 of a typical element
    assert _rel(off, direct) < 1e-4


@pytest.mark.parametrize("epi", ["stats", "bn_sums"])
@pytest.mark.parametrize("C", [64, 128])
def test_stream_k_tail(cuda, epi, C):
    """A grid of one wave and a quarter: 4x4 images, N = 16 (P + P / 4) with P = planner_cus(), 256 output channels.
    With C = 128 (K = 1152) gemm256_plan splits the quarter wave's tiles 2 ways along K -- the tail, fixed up in the
    kernel through the launch's workspace, each split starting inside the reduction (at tap 4, channel slice 1). With
    C = 64 (K = 576) no split of the reduction is 512 deep and a multiple of 64, so that launch has no tail: it checks
    the same grid without one. The result repeats bit for bit."""
    C_ = _C()
    torch.manual_seed(2)
    P = C_.planner_cus()
    N, H, W, K = 16 * (P + P // 4), 4, 4, 256
    assert C_.conv3x3_w4_tail_splits(N, H, W, C, K, 1) == (2 if C == 128 else 1)
    x = torch.randn(N, H, W, C, device=cuda).bfloat16()
    w = (torch.randn(K, 3, 3, C, device=cuda) * 0.05).bfloat16()
    ref = F.conv2d(_nchw(x), _nchw(w), None, 1, 1).permute(0, 2, 3, 1)
    plain = C_.conv3x3_w4_fwd(x, w, 1)
    assert _rel(plain, ref) < 1e-2
    assert torch.equal(C_.conv3x3_w4_fwd(x, w, 1), plain)
    if epi == "stats":
        stats = torch.zeros(C_.conv_stat_replicas, 2, K, device=cuda)
        assert torch.equal(C_.conv3x3_w4_fwd(x, w, 1, stats), plain)
        _check_stats(stats, plain)
    else:  # the same product as a data gradient: x is dy, w the transformed weight
        bx, gamma, beta, mean, invstd = _bn_operands(cuda, (N, H, W, K))
        sums = torch.zeros(C_.conv_stat_replicas, 2, K, device=cuda)
        assert torch.equal(C_.conv3x3_w4_dgrad(x, w, bx, gamma, beta, mean, invstd, sums), plain)
        _check_bn_sums(sums, plain, bx, gamma, beta, mean, invstd)


def test_routing_and_switch(cuda, monkeypatch):
    """With the planners sized for 4 CUs a 49-tile grid fills the chip: the forward and the stride-1 data gradient of a
    7x7 layer take the new route names -- the data gradient with the BatchNorm-backward sums no route took there before
    -- K8S_AMD_CONV3X3_W4=0 restores the parent's, and both give the same result within the bounds above. A 14x14 layer
    stays on the staged-window kernel, where the route did not measure faster."""
    from k8s_amd.ops import conv as kc
    from k8s_amd.ops import nn as K_

    C_ = _C()
    torch.manual_seed(3)
    N, H, C, K = 256, 7, 256, 256
    x = torch.randn(N, H, H, C, device=cuda).bfloat16()
    w = (torch.randn(K, 3, 3, C, device=cuda) * 0.05).bfloat16()
    gy = torch.randn(N, H, H, K, device=cuda).bfloat16()
    bx, gamma, beta, mean, invstd = _bn_operands(cuda, (N, H, H, C))

    def link():
        ln = K_.BnStatLink()
        ln.fill_relu(bx, mean, invstd, gamma, beta)
        return ln

    def run():
        s0, r0 = dict(kc.STATS), kc.ROUTES.copy()
        stats = torch.zeros(C_.conv_stat_replicas, 2, K, device=cuda)
        y = kc.conv_fwd(x, w, 1, 1, stats)
        dx = kc._dgrad_hip(C_, gy, w, 1)
        ln = link()
        dxs = kc._dgrad_hip(C_, gy, w, 1, None, ln)
        return (y, dx, dxs, stats, ln.sums), kc.STATS["w4_3x3_fwd"] - s0["w4_3x3_fwd"], dict(kc.ROUTES - r0)

    C_.set_planner_cus(4)
    try:
        assert C_.conv3x3_w4_use(N, H, H, C, K, 1, False) and not C_.conv3x3_w4_use(N, H, H, C, K, 2, True)
        assert C_.conv3x3_w4_use(64, 28, 28, C, K, 2, False)
        assert not C_.conv3x3_w4_use(64, 14, 14, C, K, 1, False) and not C_.conv3x3_w4_use(64, 14, 14, C, K, 1, True)
        on, fwd_on, routes_on = run()
        monkeypatch.setenv("K8S_AMD_CONV3X3_W4", "0")
        assert not C_.conv3x3_w4_use(N, H, H, C, K, 1, False)
        off, fwd_off, routes_off = run()
    finally:
        C_.set_planner_cus(0)
    assert fwd_on == 1 and routes_on == {"w4_3x3_flipped": 1, "w4_3x3_relu_sums": 1}
    assert fwd_off == 0 and routes_off == {"implicit_flipped": 2}
    for a, b in zip(on[:3], off[:3]):  # two kernels, two summation orders: bf16 rounding apart
        assert _rel(a, b) < 1e-2
    assert torch.equal(on[1], on[2])
    assert _rel(on[3].sum(0), off[3].sum(0)) < 1e-3  # the statistics of outputs a bf16 rounding apart
    assert off[4] is None
    _check_bn_sums(on[4], on[2], bx, gamma, beta, mean, invstd)
