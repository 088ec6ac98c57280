"""An identity bottleneck's conv1 backward with bn1's apply pass formed on load (conv1_fused.hip): against the route it
replaces run in the same process (bn_bwd_apply, then gemm_short's masked-addend data gradient with the sums, then the
weight gradient ``ops.conv._wgrad_hip`` picks) and against fp64 references, and through a stage-1 identity bottleneck
with K8S_AMD_CONV1_FUSED on and off."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _C():
    from k8s_amd.ops._ext import load

    return load()


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _unpack(mask, shape):
    b = (mask.view(-1, 1).to(torch.int32) >> torch.arange(8, device=mask.device, dtype=torch.int32)) & 1
    return b.view(shape).bool()


# [N, H, W] of the rows: less than one 32-row tile; exact tiles; a ragged last tile (most workgroups get no tile); more
# tiles than workgroups (the ring wraps, a workgroup walks more than one tile). Both widths.
ROWS = [(1, 3, 3), (1, 8, 8), (2, 7, 7), (6, 40, 40)]
WIDTHS = [64, 128]
_CASES = {}


def _case(cuda, nhw, W):
    """Inputs, the parent route's outputs, the new route's (dW written, accumulated, and a second run) and the fp64
    references: computed once per shape."""
    key = (nhw, W)
    if key in _CASES:
        return _CASES[key]
    from k8s_amd.ops import conv as kc

    C_ = _C()
    Nb, H, Wd = nhw
    M, N = Nb * H * Wd, 4 * W
    g = torch.Generator(device=cuda).manual_seed(4000 + M + W)
    rn = lambda *s: torch.randn(*s, device=cuda, generator=g)
    dz1 = rn(M, W).bfloat16()
    x1 = (rn(M, W) * 1.5).bfloat16()  # about half below the ReLU threshold (shift below is small)
    w = (rn(W, N) * 0.05).bfloat16()
    xin = (rn(M, N) * 1.2 + 0.3).bfloat16()
    dy = rn(M, N).bfloat16()
    x3 = (rn(M, N) * 1.5 + 0.2).bfloat16()
    amask = torch.randint(0, 256, (M * N // 8,), device=cuda, dtype=torch.uint8, generator=g)
    bits = torch.randint(0, 256, (M * N // 8,), device=cuda, dtype=torch.uint8, generator=g)
    mean = rn(N) * 0.3
    sign = torch.where(torch.rand(W, device=cuda, generator=g) < 0.5, -1.0, 1.0)
    params = torch.cat([torch.rand(W, device=cuda, generator=g) + 0.5,                  # sc (the forward's scale)
                        sign * (torch.rand(W, device=cuda, generator=g) * 0.2 + 0.05),   # B
                        sign * (torch.rand(W, device=cuda, generator=g) * 0.3 + 0.1),    # D: never zero
                        rn(W) * 0.2]).contiguous()                                       # shift
    base = rn(W, N)
    R = C_.conv_stat_replicas
    c = dict(M=M, N=N, dz1=dz1, x1=x1, w=w, xin=xin, dy=dy, x3=x3, amask=amask, bits=bits, mean=mean, params=params)

    # ---- the parent's three launches
    dx1 = C_.bn_bwd_apply(dz1, x1, None, params)
    sums_p = torch.zeros(R, 2, N, device=cuda)
    dx_p = C_.dgrad_short_bnstats(dx1, w, dy, amask, x3, bits, mean, sums_p)
    dw_p = torch.full((W, 1, 1, N), 7.0, device=cuda)
    kc._wgrad_hip(C_, dx1.view(Nb, H, Wd, W), xin.view(Nb, H, Wd, N), dw_p, 1, 0, False)
    dw_pa = base.clone().view(W, 1, 1, N)
    kc._wgrad_hip(C_, dx1.view(Nb, H, Wd, W), xin.view(Nb, H, Wd, N), dw_pa, 1, 0, True)
    c.update(dx1=dx1, dx_p=dx_p, dw_p=dw_p.view(W, N), dw_pa=dw_pa.view(W, N), sums_p=sums_p.sum(0), base=base)

    # ---- the new route: dW written, accumulated onto `base`, and written again
    def new(acc):
        dw = base.clone() if acc else torch.full((W, N), 7.0, device=cuda)
        sums = torch.zeros(R, 2, N, device=cuda)
        dx = C_.conv1_fused(dz1, x1, params, w, xin, dy, amask, x3, bits, mean, sums, dw, acc)
        return dx, dw, sums.sum(0)

    c["new"], c["acc"], c["again"] = new(False), new(True), new(False)

    # ---- fp64 references
    on = (x1.double() * params[:W].double() + params[3 * W:].double()).float().bfloat16().float() > 0
    c["on"] = on.float().mean().item()
    pd = params.double()
    gz = torch.where(on, dz1.double(), torch.zeros((), device=cuda, dtype=torch.float64))
    c["dx1_64"] = pd[:W] * gz + (pd[W:2 * W] * x1.double() + pd[2 * W:3 * W])
    add = torch.where(_unpack(amask, (M, N)), dy.double(), torch.zeros((), device=cuda, dtype=torch.float64))
    c["dx_64"] = dx1.double() @ w.double() + add        # from the stored bf16 dx1 both routes multiply
    c["dw_64"] = dx1.double().t() @ xin.double()
    _CASES[key] = c
    return c


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("nhw", ROWS)
def test_apply_pass_reference(cuda, nhw, W):
    """The dx1 the parent route materialises (and the references build on) is bf16(sc g + B x1 + D), g = dz1 where
    bf16(x1 sc + shift) > 0; about half of x1 is below the threshold."""
    c = _case(cuda, nhw, W)
    r = _rel(c["dx1"], c["dx1_64"])
    print("dx1 rel", r)
    assert r < 4e-3  # one bf16 rounding: 2^-9 per element at most
    assert 0.3 < c["on"] < 0.7


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("nhw", ROWS)
def test_dx_bitwise_parent(cuda, nhw, W):
    """dx = the parent route's dx bit for bit (the same apply expression, the same MFMA chunks in the same order, the
    same two roundings), dW written or accumulated; and no further from fp64 than the parent's."""
    c = _case(cuda, nhw, W)
    for k in ("new", "acc"):
        assert torch.equal(c[k][0], c["dx_p"]), k
    e_new, e_par = (c["new"][0].double() - c["dx_64"]).abs().max().item(), \
        (c["dx_p"].double() - c["dx_64"]).abs().max().item()
    print("dx max err vs fp64: new", e_new, "parent", e_par)
    assert e_new <= e_par
    assert c["new"][0].float().abs().max().item() > 0


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("nhw", ROWS)
def test_dw_error_within_twice_parent(cuda, nhw, W):
    """dW against fp64 (relative Frobenius error): at most twice the parent weight gradient's own error on the same
    inputs -- both are fp32 sums of the same M products, grouped differently. Written, and accumulated onto the same
    random base (a second deposit into a gradient slot: the route serves it), each against the parent's same form."""
    c = _case(cuda, nhw, W)
    for k, par, ref in (("new", c["dw_p"], c["dw_64"]), ("acc", c["dw_pa"], c["base"].double() + c["dw_64"])):
        e, e_par = _rel(c[k][1], ref), _rel(par, ref)
        print(k, "dW rel err vs fp64", e, "parent", e_par)
        assert e <= 2 * e_par


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("nhw", ROWS)
def test_sums_of_stored_dx(cuda, nhw, W):
    """Both BatchNorm-backward sums against fp64 sums over the stored dx, g = bit ? dx : 0: gemm_short's EPI 3 bound
    (tests/test_gemm_conv_gpu.py, 1e-4)."""
    c = _case(cuda, nhw, W)
    M, N = c["M"], c["N"]
    dx, _, tot = c["new"]
    gd = torch.where(_unpack(c["bits"], (M, N)), dx.double(), torch.zeros((), device=cuda, dtype=torch.float64))
    r0, r1 = _rel(tot[0], gd.sum(0)), _rel(tot[1], (gd * (c["x3"].double() - c["mean"].double())).sum(0))
    print("sums rel", r0, r1)
    assert r0 < 1e-4
    assert r1 < 1e-4


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("nhw", ROWS)
def test_two_runs_bitwise(cuda, nhw, W):
    c = _case(cuda, nhw, W)
    assert torch.equal(c["new"][0], c["again"][0])
    assert torch.equal(c["new"][1], c["again"][1])


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("nhw", ROWS)
def test_params_half_matches_full_backward(cuda, nhw, C):
    """The hand-over's two halves with the ReLU recomputed from x (mask None), per row count and width: bn_bwd_params
    gives the dgamma / dbeta of the full bn_bwd bit for bit -- from a producer's sums and from its own reduce sweep --
    and bn_bwd_apply on its table the same dx."""
    C_ = _C()
    M = nhw[0] * nhw[1] * nhw[2]
    g = torch.Generator(device=cuda).manual_seed(41 + M + C)
    rn = lambda *s: torch.randn(*s, device=cuda, generator=g)
    x = (rn(M, C) * 1.5 + 0.3).bfloat16()
    dy = rn(M, C).bfloat16()
    mean = x.float().mean(0)
    invstd = torch.rsqrt(x.float().var(0, unbiased=False) + 1e-5)
    gamma, beta = torch.rand(C, device=cuda, generator=g) + 0.5, rn(C) * 0.1
    for with_sums in (True, False):
        sums = None
        if with_sums:
            sums = torch.zeros(C_.conv_stat_replicas, 2, C, device=cuda)
            sums[:2] = rn(2, 2, C)
        dg1, db1, dg2, db2 = (torch.empty(C, device=cuda) for _ in range(4))
        dx1, _ = C_.bn_bwd(dy, x, None, mean, invstd, gamma, beta, True, dg1, db1, False, None, sums)
        params = C_.bn_bwd_params(dy, x, None, sums, mean, invstd, gamma, beta, dg2, db2)
        assert torch.equal(dg1, dg2) and torch.equal(db1, db2), with_sums
        assert torch.equal(C_.bn_bwd_apply(dy, x, None, params), dx1), with_sums


def test_rejects_bad_operands(cuda):
    C_ = _C()
    c = _case(cuda, (2, 7, 7), 64)
    R = C_.conv_stat_replicas
    ok = dict(dz1=c["dz1"], x1=c["x1"], params=c["params"], w=c["w"], xin=c["xin"], add_src=c["dy"],
              add_mask=c["amask"], x=c["x3"], mask=c["bits"], mean=c["mean"],
              sums=torch.zeros(R, 2, 256, device=cuda), dw=torch.zeros(64, 256, device=cuda), accumulate=False)
    for bad in ({"x1": c["x1"][:, :32].contiguous()}, {"mask": c["bits"][:-1].clone()},
                {"params": c["params"][:3 * 64].clone()}, {"xin": c["xin"].float()},
                {"w": c["w"][:, :128].contiguous()}):
        with pytest.raises(RuntimeError):
            C_.conv1_fused(**{**ok, **bad})
    assert not C_.conv1_fused_ok(98, 256, 1024) and not C_.conv1_fused_ok(98, 64, 512)


# --------------------------------------------------------------------------- block level, switch on against off
def _block(cuda):
    from k8s_amd.models.resnet import BN, Bottleneck
    from k8s_amd.parallel.flat import ParamStore

    store = ParamStore()
    pre = BN(store, "pre", 256)
    blk = Bottleneck(store, "b", 256, 64, 1, False)
    store.finalize(cuda, seed=31)
    pre, blk = pre.to(cuda).train(), blk.to(cuda).train()
    gen = torch.Generator(device=cuda).manual_seed(32)
    with torch.no_grad():
        for bn in (pre, blk.bn1, blk.bn2, blk.bn3):
            bn.gamma.master.uniform_(0.5, 1.5, generator=gen)
            bn.beta.master.normal_(0.0, 0.3, generator=gen)
    return store, pre, blk


class _Calls:
    """Counts the extension's apply-pass and weight-gradient entry points (the launches ``STATS`` does not name)."""
    NAMES = ("bn_bwd", "bn_bwd_apply", "bn_bwd_params", "conv_wgrad", "gemm", "conv1_fused", "dgrad_short_bnstats")

    def __init__(self, monkeypatch, C_):
        self.n = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(C_, name, self._wrap(name, getattr(C_, name)))

    def _wrap(self, name, fn):
        def call(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return call


def _step(cuda, monkeypatch, forward):
    """One forward + backward of a residual BatchNorm (the previous block's bn3: a mask-kind link on its output)
    followed by a stage-1-shaped identity bottleneck at batch 2, 8x8."""
    from k8s_amd.ops import conv as kc

    torch.manual_seed(5)
    x0 = torch.randn(2, 8, 8, 256, device=cuda).bfloat16()
    r0 = torch.randn(2, 8, 8, 256, device=cuda).bfloat16()
    gy = torch.randn(2, 8, 8, 256, device=cuda).bfloat16()
    store, pre, blk = _block(cuda)
    with monkeypatch.context() as mp:
        calls = _Calls(mp, _C())
        stats, routes = dict(kc.STATS), dict(kc.ROUTES)
        store.begin_step()
        x = x0.clone().requires_grad_(True)
        forward(blk, pre(x, residual=r0, relu=True)).backward(gy)
        store.zero_unwritten()
    counts = {k: kc.STATS[k] - stats[k] for k in ("hip_wgrad", "hip_dgrad", "conv1_onload", "conv1_apply")}
    counts["stat_conv1_fused"] = kc.STATS["conv1_fused"] - stats["conv1_fused"]
    counts["short_mask_sums"] = kc.ROUTES["short_mask_sums"] - routes.get("short_mask_sums", 0)
    counts.update(calls.n)
    return x.grad.clone(), {p.name: p.grad.clone() for p in store.params}, counts


def _agree(a, b, equal=()):
    """Gradients within 1e-2 (relative Frobenius); those named in ``equal`` ("x" or a parameter; "*": all) bit for
    bit."""
    (dx1, per1, _), (dx2, per2, _) = a, b
    assert len(per1) == 11
    for n, (u, v) in {"x": (dx1, dx2), **{n: (per1[n], per2[n]) for n in per1}}.items():
        if n in equal or "*" in equal:
            assert torch.equal(u, v), n
        assert _rel(u, v) < 1e-2, n


def test_block_conv1_fused_on_off(cuda, monkeypatch):
    """Switch on: conv1's backward is one conv1_fused launch (no masked-addend gemm_short, no weight-gradient launch of
    its own) and bn1 runs only its params half -- one full BatchNorm backward (params + apply) fewer. Switch off: the
    parent's launches. The gradients agree."""
    runs = {}
    for on in ("1", "0"):
        monkeypatch.setenv("K8S_AMD_CONV1_FUSED", on)
        runs[on] = _step(cuda, monkeypatch, lambda blk, x: blk(x))
    c1, c0 = runs["1"][2], runs["0"][2]
    print(c1, c0)
    assert c1["hip_wgrad"] == c0["hip_wgrad"] == 3 and c1["hip_dgrad"] == c0["hip_dgrad"] == 3
    # the data gradient keeps its contract's route name either way (ops.conv.ROUTES); STATS names the kernel
    assert c1["short_mask_sums"] == c0["short_mask_sums"] == 1
    assert (c1["conv1_fused"], c1["stat_conv1_fused"], c1["conv1_onload"], c1["conv1_apply"]) == (1, 1, 1, 0)
    # (switch off: bn1's own backward ran the apply pass for a link that was offered -- counted like bn3_apply)
    assert (c0["conv1_fused"], c0["stat_conv1_fused"], c0["conv1_onload"], c0["conv1_apply"]) == (0, 0, 0, 1)
    assert c1["bn_bwd"] == c0["bn_bwd"] - 1 and c1["bn_bwd_apply"] == c0["bn_bwd_apply"]  # one apply pass fewer
    assert c1["bn_bwd_params"] == c0["bn_bwd_params"] + 1
    assert c1["dgrad_short_bnstats"] == c0["dgrad_short_bnstats"] - 1
    # conv1's weight gradient had a launch of its own (the streaming / implicit kernel or a plain split-K GEMM)
    assert c1["conv_wgrad"] + c1["gemm"] == c0["conv_wgrad"] + c0["gemm"] - 1
    # bit for bit: what is computed before conv1's backward runs, and what reads only its dx (which is gemm_short's bit
    # for bit): the block's bn1 / bn2 / bn3 and conv2 / conv3. Not: conv1's dW (another summation order) and, behind
    # the previous BatchNorm, x.grad and that BatchNorm's dgamma / dbeta, which read conv1's sums (fp32 sums over the
    # same stored dx in another order)
    same = [n for n in runs["1"][1] if n.startswith("b.") and not n.startswith("b.conv1")]
    assert len(same) == 8
    _agree(runs["1"], runs["0"], equal=same)


def test_block_conv1_fallback(cuda, monkeypatch):
    """bn1 defers, but conv1's backward is handed a copy of dz1, which the link does not cover: it runs the apply pass
    on what it received and the parent's two kernels, and every gradient equals the switch-off run's bit for bit."""
    from k8s_amd.ops import nn as K

    class _CopyGrad(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return t.view_as(t)

        @staticmethod
        def backward(ctx, g):
            return g.clone()

    def forward(blk, x):  # Bottleneck.forward of an identity block, the copy between conv1 and bn1
        link, b1, b3 = K.GradLink(), K.ApplyLink(), K.ApplyLink()
        y1, sums = blk.conv1(x, grad_link=link, apply_link=b1)
        t = K.bn_relu_conv((_CopyGrad.apply(y1), sums), blk.bn1, blk.conv2, in_link=b1)
        t = K.bn_relu_conv(t, blk.bn2, blk.conv3, out_link=b3)
        return blk.bn3(t, residual=x, relu=True, res_link=link, apply_link=b3)

    monkeypatch.setenv("K8S_AMD_CONV1_FUSED", "1")
    fb = _step(cuda, monkeypatch, forward)
    monkeypatch.setenv("K8S_AMD_CONV1_FUSED", "0")
    off = _step(cuda, monkeypatch, lambda blk, x: blk(x))
    c = fb[2]
    assert (c["conv1_fused"], c["stat_conv1_fused"], c["conv1_onload"], c["conv1_apply"], c["short_mask_sums"]) == (
        0, 0, 1, 1, 1)  # deferred, then applied after all by conv1's backward
    assert c["bn_bwd_apply"] == off[2]["bn_bwd_apply"] + 1 and c["bn_bwd"] == off[2]["bn_bwd"] - 1
    assert c["hip_wgrad"] == off[2]["hip_wgrad"] and c["hip_dgrad"] == off[2]["hip_dgrad"]
    # after bn_bwd_params + bn_bwd_apply (= bn_bwd bit for bit, test_params_half_matches_full_backward) exactly the
    # parent's kernels run, and at this size every statistics replica receives one add: everything is equal
    _agree(fb, off, equal=("*",))
