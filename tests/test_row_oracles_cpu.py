"""The fp64 oracles of tests/row_oracles.py, CPU tier.

Three things: each oracle agrees with torch autograd in fp64 to 1e-12; an fp32 torch evaluation of every oracle on the
GPU tests' input recipes stays inside every bound form those tests use (so a failure on the GPU means the kernel, not
the reference); and the comparisons bite -- a dropped row, a missing smoothing offset, a GELU constant off in the
fourth digit and the -inf update of the online softmax as it stood are each caught on the CPU.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_oracles as O  # noqa: E402

CPU = torch.device("cpu")
F32, F64 = torch.float32, torch.float64


def _same(a, b, what):
    err = (a - b).abs().max().item()
    scale = b.abs().max().item()
    assert err <= 1e-12 * max(scale, 1e-300), "%s: max err %g at scale %g" % (what, err, scale)


# ------------------------------------------------------------------------------------- oracles against autograd
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("edge", [None, "small", "offset", "equal", "gamma"])
def test_norm_oracle_matches_autograd(rms, res, edge):
    x, r, g, b, dy, dres = O.norm_inputs(37, 136, rms, res, CPU, edge=edge)
    xin = (x.double() + r.double() if res else x.double()).requires_grad_(True)
    gp = g.double().requires_grad_(True)
    bp = None if rms else b.double().requires_grad_(True)
    if rms:
        yt = xin * torch.rsqrt((xin * xin).mean(-1, keepdim=True) + O.EPS) * gp
    else:
        yt = F.layer_norm(xin, (136,), gp, bp, O.EPS)
    yt.backward(dy.double())
    f = O.norm_fwd(x, r, g, b, O.EPS, rms)
    _same(f["y"], yt.detach(), "y")
    if res:
        assert torch.equal(f["xsum"], (x.float() + r.float()).bfloat16())
    # the backward takes x as the kernel does: the stored sum. Feed it the unrounded sum here to compare with autograd.
    o = O.norm_bwd(dy, xin.detach(), g, f["mean"], f["rstd"], dres, rms)
    _same(o["dx"], xin.grad + (dres.double() if res else 0), "dx")
    _same(o["dgamma"], gp.grad, "dgamma")
    if not rms:
        _same(o["dbeta"], bp.grad, "dbeta")
    _same(o["dsum"], xin.grad.sum(0), "dsum")
    _same(o["abs_dbeta"], dy.double().abs().sum(0), "abs_dbeta")
    _same(o["abs_dx"], xin.grad.abs().sum(0), "abs_dx")
    assert (o["abs_dsum"] >= o["abs_dx"]).all()  # the parts of dx before they cancel
    _same(o["abs_dgamma"], (dy.double() * f["xhat"]).abs().sum(0), "abs_dgamma")


@pytest.mark.parametrize("dt", [torch.bfloat16, F32])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("V", [5, 1001])
def test_xent_oracle_matches_autograd(dt, smoothing, V):
    R = 6
    x = O.xent_logits(R, V, dt, CPU)
    lab = O.xent_labels(R, V, CPU)
    xd = x.double().requires_grad_(True)
    lt = F.cross_entropy(xd, lab, ignore_index=-100, label_smoothing=smoothing, reduction="none")
    w = torch.linspace(0.2, 1.7, R, dtype=F64)
    (lt * w).sum().backward()
    f = O.xent_fwd(x, lab, -100, smoothing)
    _same(f["loss"], lt.detach(), "loss")
    _same(f["lse"], torch.logsumexp(x.double(), -1), "lse")
    assert f["loss"][3] == 0 and not f["valid"][3]
    o = O.xent_bwd(x, lab, f["lse"], w, -100, smoothing)
    _same(o["grad"], xd.grad, "grad per-row scale")
    assert torch.equal(o["grad"][3], torch.zeros(V, dtype=F64))
    xd.grad = None
    sc = torch.tensor([0.37])  # fp32, as the kernel's dscale is
    lt = F.cross_entropy(xd, lab, ignore_index=-100, label_smoothing=smoothing, reduction="none")
    (lt.sum() * float(sc)).backward()
    _same(O.xent_bwd(x, lab, f["lse"], sc, -100, smoothing)["grad"], xd.grad, "grad scalar scale")


def test_xent_oracle_is_safe_for_masked_classes():
    x = O.xent_logits(4, 40, F32, CPU)
    x[:, :16] = float("-inf")
    x[2, 20::3] = float("-inf")
    lab = torch.tensor([17, 39, 16, -100])
    f = O.xent_fwd(x, lab, -100, 0.0)
    for i in range(4):
        keep = torch.isfinite(x[i])
        _same(f["lse"][i], torch.logsumexp(x[i][keep].double(), 0), "lse of the finite classes")
    assert torch.isfinite(f["loss"]).all()
    o = O.xent_bwd(x, lab, f["lse"], torch.tensor([1.0]), -100, 0.0)
    assert torch.isfinite(o["grad"]).all() and torch.equal(o["grad"][:, :16], torch.zeros(4, 16, dtype=F64))
    assert torch.isfinite(O.xent_grad_bound(o, False)).all()
    assert (O.xent_grad_bound(o, False)[:3, :16] <= O.FP32_TINY).all()  # a masked class: nothing but the flush floor


@pytest.mark.parametrize("blk", [0, 64])
def test_swiglu_oracle_matches_autograd(blk):
    T, Fh = 5, 128
    gu, dy = O.swiglu_inputs(T, Fh, CPU)
    cols = torch.arange(Fh)
    gcol = (cols // blk) * 2 * blk + cols % blk if blk else cols  # the kernel's documented layout
    ucol = gcol + (blk if blk else Fh)
    gud = gu.double().requires_grad_(True)
    yt = F.silu(gud[:, gcol]) * gud[:, ucol]
    yt.backward(dy.double())
    _same(O.swiglu_fwd(gu, blk), yt.detach(), "y")
    _same(O.swiglu_bwd(gu, dy, blk), gud.grad, "dgu")


def test_gelu_and_relu_oracles_match_autograd():
    dy, pre = O.act_inputs(37, 64, CPU)
    p = pre.double().requires_grad_(True)
    F.gelu(p, approximate="tanh").backward(dy.double())
    _same(O.gelu_tanh_bwd(dy, pre), p.grad, "gelu")
    y = torch.relu(pre)
    p.grad = None
    torch.relu(p).backward(dy.double())
    _same(O.relu_bwd(dy, y), p.grad, "relu")


@pytest.mark.parametrize("T,H,D", [(7, 3, 16), (9, 2, 64)])
def test_rope_oracle_is_a_complex_rotation(T, H, D):
    x, pos, table = O.rope_inputs(T, H, D, 50, CPU)
    assert int(pos.max()) == 49
    out, ab = O.rope(x, pos, table, H)
    xs = x.double().reshape(T, H, D)
    z = torch.complex(xs[..., : D // 2], xs[..., D // 2:])
    tb = table.double()[pos.long()]
    w = z * torch.complex(tb[..., 0], tb[..., 1])[:, None, :]
    _same(out, torch.cat([w.real, w.imag], -1).reshape(T, H * D), "rope")
    back, _ = O.rope(out, pos, table, H, inverse=True)
    assert (back - x.double()).abs().max() < 1e-6  # the fp32 table's cos^2 + sin^2 is 1 to 1e-7
    assert (ab >= out.abs() - 1e-15).all()


# ------------------------------------------------------------------------------- fp32 evaluation inside the bounds
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("R,D,edge", [(257, 520, None), (64, 8192, None), (257, 520, "small"), (257, 520, "offset"),
                                      (257, 520, "equal"), (257, 520, "gamma"), (4099, 136, None)])
def test_fp32_norm_stays_inside_the_bounds(rms, R, D, edge):
    x, r, g, b, dy, _ = O.norm_inputs(R, D, rms, True, CPU, edge=edge)
    f64, f32 = O.norm_fwd(x, r, g, b, O.EPS, rms), O.norm_fwd(x, r, g, b, O.EPS, rms, dtype=F32)
    if not rms:
        O.assert_within(f32["mean"], f64["mean"], 8 * O.U * f64["mean_abs"], "mean")
    O.assert_within(f32["rstd"], f64["rstd"], 32 * O.U * f64["rstd"], "rstd")
    O.assert_rounded(f32["y"].bfloat16(), f64["y"], O.norm_y_delta(f64, g, 0.0), "y (derived part of delta alone)")
    xs = f64["xsum"]
    mean, rstd = f32["mean"], f32["rstd"]
    o64, o32 = O.norm_bwd(dy, xs, g, mean, rstd, None, rms), O.norm_bwd(dy, xs, g, mean, rstd, None, rms, dtype=F32)
    for k in ("dgamma", "dbeta", "dsum"):
        O.assert_fp32_sum(o32[k], o64[k], o64["abs_" + k], what=k)


@pytest.mark.parametrize("dt", [torch.bfloat16, F32])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("V,mul,shift", [(5, 4, 0), (1001, 4, 0), (2059, 4, 0), (30522, 4, 0), (1001, 4, 1000),
                                         (1001, 4, -1000), (1001, 120, 0)])
def test_fp32_xent_stays_inside_the_bounds(dt, smoothing, V, mul, shift):
    R = 6
    x = O.xent_logits(R, V, dt, CPU, mul=float(mul), shift=float(shift))
    lab = O.xent_labels(R, V, CPU)
    f64, f32 = O.xent_fwd(x, lab, -100, smoothing), O.xent_fwd(x, lab, -100, smoothing, dtype=F32)
    O.assert_within(f32["lse"], f64["lse"], O.lse_bound(f64["lse"]), "lse")
    O.assert_within(f32["loss"], f64["loss"], O.loss_bound(f64, smoothing), "loss")
    w = torch.linspace(0.2, 1.7, R)
    lse = f32["lse"]  # the saved fp32 lse is an input of the backward on both sides
    o64, o32 = O.xent_bwd(x, lab, lse, w, -100, smoothing), O.xent_bwd(x, lab, lse, w, -100, smoothing, dtype=F32)
    O.assert_within(o32["grad"].to(dt), o64["grad"], O.xent_grad_bound(o64, dt == torch.bfloat16), "grad")


@pytest.mark.parametrize("T,H,D", [(7, 3, 16), (96, 4, 128)])
@pytest.mark.parametrize("inverse", [False, True])
def test_fp32_rope_stays_inside_the_bound(T, H, D, inverse):
    x, pos, table = O.rope_inputs(T, H, D, 512, CPU)
    o64, ab = O.rope(x, pos, table, H, inverse)
    o32, _ = O.rope(x, pos, table, H, inverse, dtype=F32)
    O.assert_rounded(o32, o64, 2 * O.U * ab, "rope fp32")
    O.assert_rounded(o32.bfloat16(), o64, 2 * O.U * ab, "rope bf16")


def test_fp32_elementwise_stays_inside_measured_delta_and_nearest():
    gu, dy = O.swiglu_inputs(96, 2056, CPU)
    for blk in (0, 8):
        w64, w32 = O.swiglu_bwd(gu, dy, blk), O.swiglu_bwd(gu, dy, blk, dtype=F32)
        O.assert_rounded(w32.bfloat16(), w64, O.measured_delta(w32, w64) / 16, "swiglu_bwd")
    d, pre = O.act_inputs(1025, 776, CPU)
    w64, w32 = O.gelu_tanh_bwd(d, pre), O.gelu_tanh_bwd(d, pre, dtype=F32)
    O.assert_nearest(w32.bfloat16(), w64, O.measured_delta(w32, w64) / 16, "gelu_bwd")
    s, a = O.colsum(w32.bfloat16())
    O.assert_fp32_sum(w32.bfloat16().float().sum(0), s, a, what="column sums of the stored g")


# ------------------------------------------------------------------------------------- the comparisons bite
def test_a_dropped_row_fails_the_sum_bound():
    R, D = 16411, 136
    x, _, g, b, dy, _ = O.norm_inputs(R, D, False, False, CPU)
    f = O.norm_fwd(x, None, g, b, O.EPS, False, dtype=F32)
    o = O.norm_bwd(dy, x, g, f["mean"], f["rstd"], None, False)
    short = O.norm_bwd(dy[:-1], x[:-1], g, f["mean"][:-1], f["rstd"][:-1], None, False, dtype=F32)
    for k in ("dgamma", "dbeta", "dsum"):
        with pytest.raises(AssertionError, match="worst element"):
            O.assert_fp32_sum(short[k], o[k], o["abs_" + k], what=k)


@pytest.mark.parametrize("V", [30522, 128256])
def test_a_missing_smoothing_offset_fails_the_gradient_bound(V):
    x = O.xent_logits(4, V, torch.bfloat16, CPU)
    lab = O.xent_labels(4, V, CPU)
    lse = O.xent_fwd(x, lab, -100, 0.1, dtype=F32)["lse"]
    o = O.xent_bwd(x, lab, lse, torch.tensor([0.37]), -100, 0.1)
    wrong = (o["grad"] + o["off"] * 0.37 * o["sc_abs"].sign()).float().bfloat16()  # the kernel without `- off`
    with pytest.raises(AssertionError, match="worst element"):
        O.assert_within(wrong, o["grad"], O.xent_grad_bound(o, True), "grad")


def test_a_gelu_constant_off_in_the_fourth_digit_fails_nearest():
    d, pre = O.act_inputs(8200, 776, CPU)
    w64, w32 = O.gelu_tanh_bwd(d, pre), O.gelu_tanh_bwd(d, pre, dtype=F32)
    delta = O.gelu_tanh_bwd_delta(d, pre)
    O.assert_within(w32, w64, delta, "the fp32 evaluation before rounding")
    O.assert_nearest(w32.bfloat16(), w64, delta, "gelu_bwd")
    k1 = O.GELU_K1
    try:
        O.GELU_K1 = 0.0447
        wrong = O.gelu_tanh_bwd(d, pre, dtype=F32).bfloat16()
    finally:
        O.GELU_K1 = k1
    O.assert_rounded(wrong, w64, O.measured_delta(w32, w64))  # one bf16 ulp and a whole-tensor delta hide it
    with pytest.raises(AssertionError, match=r"\((\d{3,}) of") as e:  # hundreds of elements, not a lucky one
        O.assert_nearest(wrong, w64, delta, "gelu_bwd")
    print(e.value)


def test_online_softmax_with_a_minus_inf_running_maximum():
    """The per-thread update of xent.hip in fp32, as it stood and as it is: [-inf, 1, 2] gave NaN."""
    ninf = torch.tensor(float("-inf"))

    def run(vals, fixed):
        m, s = ninf.clone(), torch.tensor(0.0)
        for v in vals:
            nm = torch.maximum(m, v)
            sm = torch.tensor(0.0) if (fixed and nm == ninf) else nm
            s = s * torch.exp(m - sm) + torch.exp(v - sm)
            m = nm
        return m + torch.log(s)

    vals = [ninf, torch.tensor(1.0), torch.tensor(2.0)]
    assert torch.isnan(run(vals, fixed=False))
    want = torch.logsumexp(torch.stack(vals).double(), 0)
    assert abs(float(run(vals, fixed=True)) - float(want)) < 1e-6
    finite = [torch.tensor(0.5), torch.tensor(1.0), torch.tensor(-3.0)]
    assert float(run(finite, fixed=True)) == float(run(finite, fixed=False))  # finite rows: the same bits
