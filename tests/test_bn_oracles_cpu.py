"""The fp64 oracles and bounds of tests/bn_oracles.py, CPU tier.

Four things. Each oracle agrees with fp64 autograd through torch.nn.functional.batch_norm (+ residual + ReLU, + max
pool) to 1e-10. An fp32 evaluation of every oracle, at every edge and at the GPU tier's shapes, stays inside every bound
that tier asserts (the same check_* functions), so no bound was fitted to a kernel. An fp32 evaluation written in the
kernels' own order -- the sums form var = q / count - mean^2, the table form dx = sc g + B x + D, shifted and strided
partial sums -- stays inside too. And the bounds bite: one mutant per assertion family is caught.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_oracles as B  # noqa: E402

CPU = torch.device("cpu")
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
EPS, MOM = B.EPS, B.MOMENTUM


def _same(a, b, what):
    err = (a - b).abs().max().item()
    scale = b.abs().max().item()
    assert err <= 1e-10 * max(scale, 1e-300), "%s: max err %g at scale %g" % (what, err, scale)


# ------------------------------------------------------------------------------------- oracles against autograd
@pytest.mark.parametrize("relu,res", [(True, False), (True, True), (False, False), (False, True)])
@pytest.mark.parametrize("edge", B.EDGES)
def test_bn_oracle_matches_autograd(edge, relu, res):
    M, C = 37, 24
    d = B.bn_inputs((M, C), CPU, edge=edge, res=res)
    xd, gd, bd = (d[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
    rd = d["res"].double().requires_grad_(True) if res else None
    rm0, rv0 = torch.randn(C, dtype=F64) * 0.1, torch.rand(C, dtype=F64) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    yt = F.batch_norm(xd, rm, rv, gd, bd, True, MOM, EPS)
    if res:
        yt = yt + rd
    if relu:
        yt = torch.relu(yt)
    yt.backward(d["dy"].double())
    st = B.bn_stats(d["x"], EPS)
    r = B.run_update(rm0, rv0, st, MOM)
    _same(r["run_mean"], rm, "run_mean")
    _same(r["run_var"], rv, "run_var")
    f = B.bn_apply(d["x"], st["mean"], st["invstd"], d["gamma"], d["beta"], d["res"], relu)
    _same(f["y"], yt.detach(), "y")
    assert (f["y_abs"] >= f["y"].abs() - 1e-12).all()
    o = B.bn_bwd(d["dy"], d["x"], f["bits"] if relu else None, st["mean"], st["invstd"], d["gamma"], d["beta"])
    _same(o["dx"], xd.grad, "dx")
    _same(o["dgamma"], gd.grad, "dgamma")
    _same(o["dbeta"], bd.grad, "dbeta")
    if res:
        _same(o["g"], rd.grad, "dres")
    sc, Bc, D, shift = o["table"]
    # the kernels' affine form is the same function: against the scale of its largest term, which is what cancels
    aff = sc * o["g"] + Bc * d["x"].double() + D
    assert (aff - o["dx"]).abs().max() <= 1e-10 * o["t_abs"].max()
    _same(shift, d["beta"].double() - st["mean"] * d["gamma"].double() * st["invstd"], "shift")
    assert (o["t_abs"] >= o["dx"].abs() - 1e-9).all()


def test_bn_single_row_guard():
    """M = 1: the unbiased running variance would divide by zero; the biased one (0) is used instead."""
    x = torch.tensor([[0.5, -2.0, 3.0, 0.0, 1.0, 1.5, -0.25, 8.0]], dtype=BF16)
    st = B.bn_stats(x, EPS)
    ss = B.bn_stats_from_sums(B.sums_from(x, 3), 1, EPS)
    for s in (st, ss):
        assert torch.equal(s["unbiased"], torch.zeros(8, dtype=F64)) and torch.equal(s["mean"], x[0].double())
        assert torch.isfinite(B.run_update(torch.zeros(8), torch.ones(8), s)["run_var"]).all()


def test_bn_dual_oracle_matches_autograd():
    M, C = 29, 16
    d = B.bn_inputs((M, C), CPU, dual=True)
    leaves = [d[k].double().requires_grad_(True) for k in ("x", "gamma", "beta", "x2", "gamma2", "beta2")]
    yt = torch.relu(F.batch_norm(leaves[0], None, None, leaves[1], leaves[2], True, MOM, EPS) +
                    F.batch_norm(leaves[3], None, None, leaves[4], leaves[5], True, MOM, EPS))
    yt.backward(d["dy"].double())
    s1, s2 = B.bn_stats(d["x"]), B.bn_stats(d["x2"])
    second = (d["x2"], s2["mean"], s2["invstd"], d["gamma2"], d["beta2"])
    f = B.bn_apply(d["x"], s1["mean"], s1["invstd"], d["gamma"], d["beta"], None, True, second)
    _same(f["y"], yt.detach(), "y")
    oa = B.bn_bwd(d["dy"], d["x"], f["bits"], s1["mean"], s1["invstd"], d["gamma"], d["beta"])
    ob = B.bn_bwd(d["dy"], d["x2"], f["bits"], s2["mean"], s2["invstd"], d["gamma2"], d["beta2"])
    for o, (xg, gg, bg) in ((oa, leaves[:3]), (ob, leaves[3:])):
        _same(o["dx"], xg.grad, "dx")
        _same(o["dgamma"], gg.grad, "dgamma")
        _same(o["dbeta"], bg.grad, "dbeta")


@pytest.mark.parametrize("N,H,W", [(2, 5, 7), (1, 8, 8), (1, 1, 2), (2, 4, 3)])
def test_pool_oracle_matches_autograd(N, H, W):
    C = 8  # (torch refuses to train on one value per channel, so the single-pixel image is left to the GPU tier)
    d = B.bn_inputs((N, H, W, C), CPU, seed=13)
    xd, gd, bd = (d[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
    z = torch.relu(F.batch_norm(xd.reshape(-1, C), None, None, gd, bd, True, MOM, EPS)).reshape(N, H, W, C)
    p = F.max_pool2d(z.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    # small integers: sums of up to four of them are exact in bf16, so the oracle's rounding of dz changes nothing here
    dpool = torch.randint(-8, 9, p.shape).to(BF16)
    p.backward(dpool.double())
    win = B.pool_windows(z.detach(), float("-inf"))
    top = win.max(3).values
    _same(top, p.detach(), "pooled")
    pos = torch.arange(9).reshape(1, 1, 1, 9, 1)
    idx = torch.where(win == top.unsqueeze(3), pos, torch.full_like(pos, 9)).min(3).values.to(torch.uint8)
    st = B.bn_stats(d["x"])
    o = B.pool_bn_bwd(dpool, idx, d["x"], z.detach() > 0, st["mean"], st["invstd"], d["gamma"], d["beta"])
    _same(o["dx"], xd.grad, "dx")
    _same(o["dgamma"], gd.grad, "dgamma")
    _same(o["dbeta"], bd.grad, "dbeta")
    o2 = B.pool_bn_bwd(dpool, idx, d["x"], z.detach() > 0, st["mean"], st["invstd"], d["gamma"], d["beta"],
                       from_sums=True)
    _same(o2["dgamma"], gd.grad, "dgamma over the pooled gradient")
    # every pooled gradient lands on exactly one pixel
    assert torch.equal(B.pool_route(dpool, idx, H, W, rounded=False).sum((1, 2)), dpool.double().sum((1, 2)))


@pytest.mark.parametrize("nrep", [1, 5, 32])
def test_replica_sums_hold_the_statistics(nrep):
    """sums_from / bwd_sums_from deal every row to exactly one replica, in the [nrep, 2, C] layout."""
    M, C = 45, 16
    d = B.bn_inputs((M, C), CPU)
    st, ss = B.bn_stats(d["x"]), B.bn_stats_from_sums(B.sums_from(d["x"], nrep), M)
    assert B.sums_from(d["x"], nrep).shape == (nrep, 2, C)
    for k in ("mean", "var", "invstd", "unbiased"):
        assert (ss[k] - st[k]).abs().max() <= 1e-5 * st[k].abs().max(), k
    assert (ss["s_abs"] <= st["mean_abs"] * (1 + 1e-6)).all()
    bits = torch.rand(M, C) > 0.4
    o = B.bn_bwd(d["dy"], d["x"], bits, st["mean"].float(), st["invstd"].float(), d["gamma"], d["beta"])
    s = B.bwd_sums_from(o["g"], d["x"], st["mean"].float(), nrep)
    assert (s[:, 0].double().sum(0) - o["dbeta"]).abs().max() <= 1e-5 * o["abs_dbeta"].max()
    assert (s[:, 1].double().sum(0) * st["invstd"].float().double() - o["dgamma"]).abs().max() <= \
        1e-5 * o["abs_dgamma"].max()
    s2 = B.bwd_sums_from(o["g"], d["x"], st["mean"].float(), nrep, second=True)
    assert torch.isnan(s2[:, 0]).all() and torch.equal(s2[:, 1], s[:, 1])
    assert torch.equal(B.unpack_bits(B.pack_bits(bits), bits.shape), bits)


# ------------------------------------------------------------------------------- fp32 evaluations inside the bounds
def _seq_sum(t):
    """Sum over dim 0 by one fp32 addition after another."""
    acc = torch.zeros_like(t[0])
    for row in t:
        acc = acc + row
    return acc


def _strided_sum(t, stride=8):
    """The kernels' shape of a reduction: `stride` interleaved subsets summed in sequence each, then folded."""
    return _seq_sum(torch.stack([_seq_sum(t[r::stride]) if t[r::stride].shape[0] else torch.zeros_like(t[0])
                                 for r in range(stride)]))


def _kernel_order_stats(x, nblocks=5):
    """bn_stats_kernel / bn_stats_final_kernel in fp32: blocks of rows, each shifted by the mean of its first four rows
    (its last row again where it has fewer), (mean, M2) per block, then Chan merges."""
    xs = x.float()
    M = xs.shape[0]
    rpb = -(-M // nblocks)
    cnt, mean, m2 = 0.0, torch.zeros(xs.shape[1]), torch.zeros(xs.shape[1])
    for r0 in range(0, M, rpb):
        blk = xs[r0:r0 + rpb]
        n = float(blk.shape[0])
        shift = _seq_sum(blk[[min(u, blk.shape[0] - 1) for u in range(4)]]) * 0.25
        dlt = blk - shift
        s, q = _strided_sum(dlt), _strided_sum(dlt * dlt)
        bm = s / n
        bq = q - s * bm
        bm = bm + shift
        tot = cnt + n
        dd = bm - mean
        mean = mean + dd * n / tot
        m2 = m2 + bq + dd * dd * cnt * n / tot
        cnt = tot
    var = m2 / cnt
    return mean, torch.rsqrt(var + EPS), (m2 / (cnt - 1) if cnt > 1 else var)


def _kernel_order_stats_sums(sums, count):
    """bn_finalize_sums_kernel in fp32."""
    s, q = _seq_sum(sums[:, 0]), _seq_sum(sums[:, 1])
    c = torch.tensor(float(count))
    mean = s / c
    var = (q / c - mean * mean).clamp(min=0.0)
    return mean, torch.rsqrt(var + EPS), (var * c / (c - 1) if count > 1 else var)


def _kernel_order_apply(x, mean, invstd, gamma, beta, res, relu):
    sc = gamma * invstd
    y = x.float() * sc + (beta - mean * sc)
    if res is not None:
        y = y + res.float()
    return (y.clamp(min=0.0) if relu else y).bfloat16()


def _kernel_order_bwd(dy, x, bits, mean, invstd, gamma, beta, sums=None, no_b_mean=False):
    """bn_bwd_reduce / final / apply in fp32: strided partial sums (or the given replica sums), the table, the affine
    dx. no_b_mean: the mutant whose D lacks - B mean."""
    g = dy.float() * bits.float() if bits is not None else dy.float()
    xs = x.float()
    M = xs.shape[0]
    if sums is None:
        a, b = _strided_sum(g), _strided_sum(g * (xs - mean) * invstd)
    else:
        a, b = _seq_sum(sums[:, 0]), _seq_sum(sums[:, 1]) * invstd
    inv_m = torch.tensor(1.0) / torch.tensor(float(M))
    k1, k2 = a * inv_m, b * inv_m
    sc = gamma * invstd
    Bc = -sc * invstd * k2
    D = -sc * k1 if no_b_mean else -sc * k1 - Bc * mean
    dx = sc * g + (Bc * xs + D)
    return {"dx": dx.bfloat16(), "dres": g.bfloat16(), "dgamma": b, "dbeta": a,
            "params": torch.cat([sc, Bc, D, beta - mean * sc])}


def _case(M, C, edge, res=False, relu=True, seed=3):
    d = B.bn_inputs((M, C), CPU, edge=edge, res=res, seed=seed)
    torch.manual_seed(11)
    d["rm0"], d["rv0"] = torch.randn(C) * 0.1, torch.rand(C) + 0.5
    return d


def _check_all(d, mean, invstd, unbiased, st, own, y, bwd, relu=True):
    """Everything the GPU tier asserts on one forward + backward, on the given fp32 results."""
    x, g, b, r = d["x"], d["gamma"], d["beta"], d["res"]
    if own:
        B.check_stats_own(mean, invstd, st)
    else:
        B.check_stats_sums(mean, invstd, st)
    rm = (1 - MOM) * d["rm0"] + MOM * mean
    rv = (1 - MOM) * d["rv0"] + MOM * unbiased
    B.check_running(rm, rv, d["rm0"], d["rv0"], st, own)
    o64 = B.bn_apply(x, mean, invstd, g, b, r, relu)
    yk = y(mean, invstd)
    B.check_fwd(yk, B.pack_bits(yk > 0), o64, B.bn_apply(x, mean, invstd, g, b, r, relu, dtype=F32))
    bits = (yk > 0) if relu else None
    w64 = B.bn_bwd(d["dy"], x, bits, mean, invstd, g, b)
    got = bwd(bits, mean, invstd, w64)
    bounds = B.bn_bwd_bounds(w64)
    B.check_bwd(got["dx"], got["dres"], got["dgamma"], got["dbeta"], w64, bounds=bounds)
    B.check_table(got["params"], w64, bounds)


@pytest.mark.parametrize("edge", B.EDGES)
@pytest.mark.parametrize("M,C", B.SHAPES)
def test_fp32_oracle_inside_bounds(M, C, edge):
    """The textbook formulas in fp32 (torch's own summation order), own statistics and statistics from 1 / 32 replica
    sums, with and without a residual."""
    for res in (False, True):
        d = _case(M, C, edge, res)
        x, g, b = d["x"], d["gamma"], d["beta"]

        def y(mean, invstd):
            return B.bn_apply(x, mean, invstd, g, b, d["res"], True, dtype=F32)["y"].bfloat16()

        def bwd(bits, mean, invstd, w64):
            o = B.bn_bwd(d["dy"], x, bits, mean, invstd, g, b, dtype=F32)
            return {"dx": o["dx"].bfloat16(), "dres": o["g"].bfloat16(), "dgamma": o["dgamma"], "dbeta": o["dbeta"],
                    "params": o["table"].reshape(-1)}

        s32 = B.bn_stats(x, EPS, dtype=F32)
        _check_all(d, s32["mean"], s32["invstd"], s32["unbiased"], B.bn_stats(x, EPS), True, y, bwd)
        for nrep in (1, 32):
            sums = B.sums_from(x, nrep)
            s32 = B.bn_stats_from_sums(sums, M, EPS, dtype=F32)
            s64 = B.bn_stats_from_sums(sums, M, EPS)
            _check_all(d, s32["mean"], s32["invstd"], s32["unbiased"], s64, False, y, bwd)


@pytest.mark.parametrize("edge", B.EDGES)
@pytest.mark.parametrize("M,C", [s for s in B.SHAPES if s[0] * s[1] <= 2 ** 16])
def test_fp32_kernel_order_inside_bounds(M, C, edge):
    """The kernels' own order in fp32: shifted blocks and Chan merges, or q / count - mean^2 from 32 replica sums added
    one after another; y = x scale + shift; strided partial sums (or replica sums) for the backward, and the table form
    dx = sc g + (B x + D). At 'offset' this is the evaluation whose error grows with mean^2 / var, and the bounds' terms
    ex2 + mean^2 and |B x| + |B mean| are what holds it."""
    d = _case(M, C, edge)
    x, g, b = d["x"], d["gamma"], d["beta"]

    def y(mean, invstd):
        return _kernel_order_apply(x, mean, invstd, g, b, None, True)

    def bwd(bits, mean, invstd, w64):
        return _kernel_order_bwd(d["dy"], x, bits, mean, invstd, g, b)

    def bwd_sums(bits, mean, invstd, w64):
        return _kernel_order_bwd(d["dy"], x, bits, mean, invstd, g, b, B.bwd_sums_from(w64["g"], x, mean, 32))

    mean, invstd, unb = _kernel_order_stats(x)
    _check_all(d, mean, invstd, unb, B.bn_stats(x, EPS), True, y, bwd)
    sums = B.sums_from(x, 32)
    mean, invstd, unb = _kernel_order_stats_sums(sums, M)
    _check_all(d, mean, invstd, unb, B.bn_stats_from_sums(sums, M, EPS), False, y, bwd_sums)


def test_sums_form_loses_what_its_bound_says_and_the_shifted_form_does_not():
    """At mean 32, std 1 the fp32 sums form is off by far more than 32 u in invstd (so the own-reduce bound would
    refuse it: the two forms need their two bounds), and the shifted form is not."""
    x = B.bn_inputs((4099, 8), CPU, edge="offset")["x"]
    st = B.bn_stats(x, EPS)
    _, invstd_sums, _ = _kernel_order_stats_sums(B.sums_from(x, 32), 4099)
    assert ((invstd_sums.double() - st["invstd"]).abs() > 32 * B.U * st["invstd"]).any()
    mean, invstd, _ = _kernel_order_stats(x)
    B.check_stats_own(mean, invstd, st)


# ------------------------------------------------------------------------------------- the bounds bite: mutants
M0, C0 = 333, 72


def _good(edge=None):
    """A correct fp32 kernel-order evaluation and the oracles it is checked against."""
    d = _case(M0, C0, edge)
    x, g, b = d["x"], d["gamma"], d["beta"]
    mean, invstd, unb = _kernel_order_stats(x)
    y = _kernel_order_apply(x, mean, invstd, g, b, None, True)
    return d, mean, invstd, unb, y


def test_mutant_dropped_row():
    """One of 333 rows missing from a reduction: mean moves by 1 / 333 of a deviation, dgamma / dbeta by one term."""
    d, mean, invstd, unb, y = _good()
    x = d["x"]
    st = B.bn_stats(x, EPS)
    B.check_stats_own(mean, invstd, st)
    m1, i1, _ = _kernel_order_stats(x[:-1])
    with pytest.raises(AssertionError, match="mean"):
        B.check_stats_own(m1 * (M0 - 1) / M0 + 0 * mean, invstd, st)  # the row's share never added
    with pytest.raises(AssertionError, match="invstd"):
        B.check_stats_own(mean, i1, st)
    bits = y > 0
    w64 = B.bn_bwd(d["dy"], x, bits, mean, invstd, d["gamma"], d["beta"])
    ok = _kernel_order_bwd(d["dy"], x, bits, mean, invstd, d["gamma"], d["beta"])
    B.check_bwd(ok["dx"], ok["dres"], ok["dgamma"], ok["dbeta"], w64)
    dy1 = d["dy"].clone()
    dy1[M0 // 2] = 0  # the reduction skips the row
    bad = _kernel_order_bwd(dy1, x, bits, mean, invstd, d["gamma"], d["beta"])
    with pytest.raises(AssertionError, match="dbeta"):
        B.check_bwd(None, None, ok["dgamma"], bad["dbeta"], w64)
    with pytest.raises(AssertionError, match="dgamma"):
        B.check_bwd(None, None, bad["dgamma"], ok["dbeta"], w64)


def test_mutant_dropped_channel_group():
    """The last 8 channels of y / dx never written (what torch.empty held: NaN here, then stale finite values)."""
    d, mean, invstd, unb, y = _good()
    x, g, b = d["x"], d["gamma"], d["beta"]
    o64 = B.bn_apply(x, mean, invstd, g, b, None, True)
    o32 = B.bn_apply(x, mean, invstd, g, b, None, True, dtype=F32)
    B.check_fwd(y, None, o64, o32)
    w64 = B.bn_bwd(d["dy"], x, y > 0, mean, invstd, g, b)
    ok = _kernel_order_bwd(d["dy"], x, y > 0, mean, invstd, g, b)
    for stale in (float("nan"), 0.0):
        ybad, dxbad = y.clone(), ok["dx"].clone()
        ybad[:, -8:] = stale
        dxbad[:, -8:] = stale
        with pytest.raises(AssertionError, match="y"):
            B.check_fwd(ybad, None, o64, o32)
        with pytest.raises(AssertionError, match="dx"):
            B.check_bwd(dxbad, None, ok["dgamma"], ok["dbeta"], w64)
    dgbad = ok["dgamma"].clone()
    dgbad[-8:] = float("nan")
    with pytest.raises(AssertionError, match="dgamma"):
        B.check_bwd(None, None, dgbad, ok["dbeta"], w64)


@pytest.mark.parametrize("edge", [None, "offset"])
def test_mutant_count_off_by_one(edge):
    d = _case(M0, C0, edge)
    sums = B.sums_from(d["x"], 32)
    st = B.bn_stats_from_sums(sums, M0, EPS)
    mean, invstd, _ = _kernel_order_stats_sums(sums, M0)
    B.check_stats_sums(mean, invstd, st)
    mean1, invstd1, _ = _kernel_order_stats_sums(sums, M0 + 1)
    with pytest.raises(AssertionError, match="mean"):
        B.check_stats_sums(mean1, invstd, st)
    if edge is None:  # at 'offset' the sums form cannot tell: its own rounding is as large (var_bound_sums)
        with pytest.raises(AssertionError, match="invstd"):
            B.check_stats_sums(mean, invstd1, st)


def test_mutant_biased_run_var():
    d, mean, invstd, unb, y = _good()
    st = B.bn_stats(d["x"], EPS)
    rm = (1 - MOM) * d["rm0"] + MOM * mean
    B.check_running(rm, (1 - MOM) * d["rv0"] + MOM * unb, d["rm0"], d["rv0"], st, True)
    biased = unb * (M0 - 1) / M0
    with pytest.raises(AssertionError, match="run_var"):
        B.check_running(rm, (1 - MOM) * d["rv0"] + MOM * biased, d["rm0"], d["rv0"], st, True)
    with pytest.raises(AssertionError, match="run_mean"):
        B.check_running(d["rm0"] + MOM * mean, (1 - MOM) * d["rv0"] + MOM * unb, d["rm0"], d["rv0"], st, True)


@pytest.mark.parametrize("edge", [None, "offset", "mixed"])
def test_mutant_table_without_b_mean(edge):
    d, mean, invstd, unb, y = _good(edge)
    x, g, b = d["x"], d["gamma"], d["beta"]
    w64 = B.bn_bwd(d["dy"], x, y > 0, mean, invstd, g, b)
    bounds = B.bn_bwd_bounds(w64)
    ok = _kernel_order_bwd(d["dy"], x, y > 0, mean, invstd, g, b)
    B.check_table(ok["params"], w64, bounds)
    bad = _kernel_order_bwd(d["dy"], x, y > 0, mean, invstd, g, b, no_b_mean=True)
    with pytest.raises(AssertionError, match="table D"):
        B.check_table(bad["params"], w64, bounds)
    with pytest.raises(AssertionError, match="dx"):
        B.check_bwd(bad["dx"], None, ok["dgamma"], ok["dbeta"], w64, bounds=bounds)
    # one wrong entry of any row, in one channel of 72
    for row in range(4):
        p = ok["params"].clone()
        p[row * C0 + 17] *= 1 + 1e-3
        with pytest.raises(AssertionError, match="table"):
            B.check_table(p, w64, bounds)


def test_mutant_mask_bit_shifted():
    d, mean, invstd, unb, y = _good()
    x, g, b = d["x"], d["gamma"], d["beta"]
    o64 = B.bn_apply(x, mean, invstd, g, b, None, True)
    o32 = B.bn_apply(x, mean, invstd, g, b, None, True, dtype=F32)
    mask = B.pack_bits(y > 0)
    B.check_fwd(y, mask, o64, o32)
    with pytest.raises(AssertionError, match="mask"):
        B.check_fwd(y, (mask << 1) | (mask >> 7), o64, o32)
    # and a backward that reads the bits one position off: dres, dx and the sums all show it
    w64 = B.bn_bwd(d["dy"], x, y > 0, mean, invstd, g, b)
    bad = _kernel_order_bwd(d["dy"], x, torch.roll(y > 0, 1, 1), mean, invstd, g, b)
    ok = _kernel_order_bwd(d["dy"], x, y > 0, mean, invstd, g, b)
    with pytest.raises(AssertionError, match="dres"):
        B.check_bwd(ok["dx"], bad["dres"], ok["dgamma"], ok["dbeta"], w64)
    with pytest.raises(AssertionError, match="dx"):
        B.check_bwd(bad["dx"], None, ok["dgamma"], ok["dbeta"], w64)


def test_mutant_dual_second_input_swapped():
    d = B.bn_inputs((M0, C0), CPU, dual=True)
    s1, s2 = B.bn_stats(d["x"], dtype=F32), B.bn_stats(d["x2"], dtype=F32)
    bits = torch.rand(M0, C0) > 0.5
    args2 = (s2["mean"], s2["invstd"], d["gamma2"], d["beta2"])
    ob = B.bn_bwd(d["dy"], d["x2"], bits, *args2)
    ok = _kernel_order_bwd(d["dy"], d["x2"], bits, *args2)
    B.check_bwd(ok["dx"], None, ok["dgamma"], ok["dbeta"], ob)
    bad = _kernel_order_bwd(d["dy"], d["x"], bits, *args2)  # the first BatchNorm's input with the second's statistics
    with pytest.raises(AssertionError, match="dgamma"):
        B.check_bwd(None, None, bad["dgamma"], ok["dbeta"], ob)
    with pytest.raises(AssertionError, match="dx"):
        B.check_bwd(bad["dx"], None, ok["dgamma"], ok["dbeta"], ob)
