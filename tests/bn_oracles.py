"""fp64 oracles of the BatchNorm kernels (batchnorm.hip), their error bounds and the per-element checks.

Textbook BatchNorm over [M, C] rows (channels last) written out in torch, evaluated in `dtype` (fp64 unless asked
otherwise) on the device the inputs live on. Each oracle takes the kernels' exact inputs (bf16 / fp32 / uint8 tensors,
cast up) and returns the results plus the sums of absolute terms its bounds are made of. Nothing here imports k8s_amd:
the package's CPU reference shares the kernels' formulas.

The `check_*` functions hold the assertions. The GPU tier hands them a kernel's outputs, the CPU tier an fp32 evaluation
of the oracle, an fp32 evaluation in the kernels' order, or a mutant: one set of bounds for all of them, none fitted to
a kernel. u = 2^-24 throughout.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from row_oracles import (BF16_ULP, F64, U, assert_fp32_sum, assert_nearest, assert_rounded,  # noqa: F401
                         assert_within, measured_delta)

EPS = 1e-5
MOMENTUM = 0.1
EDGES = [None, "offset", "const", "tiny", "mixed", "zero_g"]
CONST_VALUE = 0.75  # the constant channel's value (bf16-exact, non-zero)
# (M, C) of the GPU tier, each the smallest that reaches one edge of the kernels' geometry (test_bn_kernels_gpu.py says
# which); the CPU tier evaluates the oracles in fp32 at the same ones
SHAPES = [(1, 8), (7, 8), (9, 24), (63, 64), (64, 72), (98, 80), (333, 24), (333, 72), (1000, 256), (4099, 8),
          (4099, 64), (98, 2048), (7, 2048), (9, 2048), (64, 256), (64, 2056)]


def edge_channel(C):
    """The channel the 'const' and 'zero_g' edges act on."""
    return min(3, C - 1)


# ----------------------------------------------------------------------------------------------- packed masks
def unpack_bits(mask, shape):
    """uint8 [numel / 8], bit j of byte e = element 8 e + j  ->  bool tensor of `shape`."""
    sh = torch.arange(8, device=mask.device, dtype=torch.uint8)
    return ((mask.reshape(-1, 1) >> sh) & 1).bool().reshape(shape)


def pack_bits(bits):
    w = (2 ** torch.arange(8, device=bits.device)).to(torch.int32)
    return (bits.reshape(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)


# ----------------------------------------------------------------------------------------------- statistics
def _rows(t, dtype):
    return t.to(dtype).reshape(-1, t.shape[-1])


def bn_stats(x, eps=EPS, dtype=F64):
    """mean, biased var, invstd, unbiased var (the biased one for a single row, the kernels' guard) and
    mean_abs = mean_r |x| per channel."""
    xs = _rows(x, dtype)
    M = xs.shape[0]
    mean = xs.sum(0) / M
    m2 = ((xs - mean) ** 2).sum(0)
    var = m2 / M
    return {"mean": mean, "var": var, "invstd": 1.0 / torch.sqrt(var + eps),
            "unbiased": m2 / (M - 1) if M > 1 else var, "mean_abs": xs.abs().sum(0) / M, "count": M}


def bn_stats_from_sums(sums, count, eps=EPS, dtype=F64):
    """The same from replica sums fp32 [nrep, 2, C] = (sum x, sum x^2): the sums are the kernel's INPUTS, so the
    statistics are what exact arithmetic makes of those fp32 numbers. Also ex2 = q / count, mean_sq = mean^2 and
    s_abs = sum_r |s_r| / count, the terms of var_bound_sums / mean_bound_sums."""
    s3 = sums.to(dtype)
    s, q = s3[:, 0].sum(0), s3[:, 1].sum(0)
    mean = s / count
    ex2 = q / count
    var = (ex2 - mean * mean).clamp(min=0.0)
    return {"mean": mean, "var": var, "invstd": 1.0 / torch.sqrt(var + eps),
            "unbiased": var * count / (count - 1) if count > 1 else var, "ex2": ex2, "mean_sq": mean * mean,
            "s_abs": s3[:, 0].abs().sum(0) / count, "nrep": sums.shape[0], "count": count}


def mean_bound_sums(st):
    """An fp32 mean from nrep replica sums: nrep - 1 additions, each off by at most u of a partial sum that is at most
    sum_r |s_r|, and the division's u: (nrep + 1) u s_abs. s_abs <= mean_r |x|, so for up to 7 replicas this is inside
    the own-reduce form 8 u mean_abs; for the convolutions' 32 replicas the additions alone allow 31 u."""
    return (st["nrep"] + 1) * U * st["s_abs"]


def var_bound_sums(st):
    """|d var| <= k u (ex2 + mean^2), k = 2 nrep + 4, for var = q / count - mean^2 formed in fp32:
      ex2 = q / count: nrep - 1 additions of non-negative terms and a division, nrep u ex2;
      mean: (nrep + 1) u s_abs (mean_bound_sums), so mean^2 is off by 2 |mean| (nrep + 1) u s_abs + u mean^2; by
        Cauchy-Schwarz s_abs <= sqrt(ex2), and 2 |mean| sqrt(ex2) <= mean^2 + ex2:
        (nrep + 1) u (ex2 + mean^2) + u mean^2;
      the subtraction: u |var| <= u (ex2 + mean^2).
    Summed: (2 nrep + 2) u ex2 + (nrep + 3) u mean^2 <= (2 nrep + 4) u (ex2 + mean^2). This is the loss in proportion
    to mean^2 / var that the sums form has by design."""
    return (2 * st["nrep"] + 4) * U * (st["ex2"] + st["mean_sq"])


def invstd_interval(var, dvar, eps=EPS, few=8):
    """[lo, hi] of (v + eps)^-1/2 over v in [max(var - dvar, 0), var + dvar], widened by `few` u relative (the
    addition of eps, the reciprocal square root to 2 ulp). To first order this is the relative bound
    0.5 dvar / (var + eps) + few u; the interval stays true where dvar is not small against var + eps (a constant
    channel: var = 0, and the clamp at 0 keeps hi at eps^-1/2)."""
    lo = 1.0 / torch.sqrt(var + dvar + eps)
    hi = 1.0 / torch.sqrt((var - dvar).clamp(min=0.0) + eps)
    return lo * (1 - few * U), hi * (1 + few * U)


def assert_between(got, lo, hi, what):
    g = got.to(F64)
    bad = ~((g >= lo) & (g <= hi))
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError("%s: element %d got %.9g outside [%.9g, %.9g] (%d of %d out)" % (
            what, i, float(g.reshape(-1)[i]), float(lo.reshape(-1)[i]), float(hi.reshape(-1)[i]), int(bad.sum()),
            bad.numel()))


def run_update(run_mean, run_var, st, momentum=MOMENTUM, dtype=F64):
    """The running statistics after one training step, and the absolute terms of each."""
    rm, rv = run_mean.to(dtype), run_var.to(dtype)
    mean, unb = st["mean"].to(dtype), st["unbiased"].to(dtype)
    return {"run_mean": (1 - momentum) * rm + momentum * mean, "run_var": (1 - momentum) * rv + momentum * unb,
            "abs_mean": (1 - momentum) * rm.abs() + momentum * mean.abs(),
            "abs_var": (1 - momentum) * rv.abs() + momentum * unb.abs()}


# ----------------------------------------------------------------------------------------------- forward apply
def bn_apply(x, mean, invstd, gamma, beta, res=None, relu=True, second=None, dtype=F64):
    """y = act(xhat gamma + beta [+ res | + BN_r(xr)]) from a GIVEN mean / invstd (the caller hands on the ones the
    kernel returned). second = (xr, mean_r, invstd_r, gamma_r, beta_r) for the two-BatchNorm form. Returns y (x's
    shape), bits = y > 0, and y_abs = |x scale| + |mean scale| + |beta| (+ |res| or the second side's terms): the terms
    of the kernels' affine form y = fma(x, scale, shift), scale = gamma invstd, shift = beta - mean scale."""
    def side(x_, mean_, invstd_, gamma_, beta_):
        xs = _rows(x_, dtype)
        mu, is_, gm, bt = (t.to(dtype) for t in (mean_, invstd_, gamma_, beta_))
        sc = gm * is_
        return (xs - mu) * is_ * gm + bt, (xs * sc).abs() + (mu * sc).abs() + bt.abs()

    y, y_abs = side(x, mean, invstd, gamma, beta)
    if second is not None:
        y2, a2 = side(*second)
        y, y_abs = y + y2, y_abs + a2
    if res is not None:
        r = _rows(res, dtype)
        y, y_abs = y + r, y_abs + r.abs()
    if relu:
        y = y.clamp(min=0.0)
    return {"y": y.reshape(x.shape), "y_abs": y_abs.reshape(x.shape), "bits": (y > 0).reshape(x.shape)}


def y_delta(o64, o32):
    """delta of y for assert_rounded: the measured fp32-against-fp64 distance of the oracle, plus the affine form's
    own roundings, which the textbook order does not have: scale = fl(gamma invstd) is off by u (felt through x scale
    and through mean scale), shift = fl(beta - mean scale) by u |shift|, the fma by u |y|, a residual add by u more:
    at most 4 u y_abs. (mean and invstd are the kernel's own, checked separately: nothing is carried from them.)
    ReLU is continuous, so the bound holds through it and no element is excluded."""
    return measured_delta(o32["y"], o64["y"]) + 4 * U * o64["y_abs"]


# ----------------------------------------------------------------------------------------------- backward
def bn_bwd(dy, x, bits, mean, invstd, gamma, beta, dtype=F64, dy_sums=None):
    """The backward from given mean / invstd and given ReLU bits (bool of x's shape, None: no ReLU):
    g = bits ? dy : 0, dbeta = sum g, dgamma = sum g xhat, dx = invstd gamma (g - mean(g) - xhat mean(g xhat)),
    dres = g, the table [sc | B | D | shift] of the kernels' form dx = sc g + B x + D, and the absolute terms.
    dy_sums: the gradient the two sums are taken over where it is not dy itself (the stem's sums form, below)."""
    C = x.shape[-1]
    g = _rows(dy, dtype)
    gs = g if dy_sums is None else _rows(dy_sums, dtype)
    if bits is not None:
        g = g * bits.reshape(-1, C).to(dtype)
        gs = g if dy_sums is None else gs * bits.reshape(-1, C).to(dtype)
    xs = _rows(x, dtype)
    M = xs.shape[0]
    mu, is_, gm, bt = (t.to(dtype) for t in (mean, invstd, gamma, beta))
    xhat = (xs - mu) * is_
    dbeta, dgamma = gs.sum(0), (gs * xhat).sum(0)
    k1, k2 = dbeta / M, dgamma / M
    sc = gm * is_
    B = -sc * is_ * k2
    D = -sc * k1 - B * mu
    return {"g": g.reshape(x.shape), "g_sums": gs.reshape(x.shape), "dbeta": dbeta, "dgamma": dgamma,
            "abs_dbeta": gs.abs().sum(0), "abs_dgamma": (gs * xhat).abs().sum(0),
            "dx": (sc * (g - k1 - xhat * k2)).reshape(x.shape),
            "table": torch.stack([sc, B, D, bt - mu * sc]),
            "t_abs": ((sc * g).abs() + (B * xs).abs() + (B * mu).abs() + (sc * k1).abs()).reshape(x.shape),
            "x_abs": xs.abs().reshape(x.shape), "sc": sc, "B": B, "mu": mu, "is": is_, "k1": k1, "beta": bt, "M": M}


def bn_bwd_bounds(o, k=32):
    """Bounds of the backward's outputs from bn_bwd's fp64 result `o`.
      dbeta, dgamma: k u sum|terms| (assert_fp32_sum); db = k u sum|g| / M and dg = k u sum|g xhat| / M are what they
        leave in k1 = dbeta / M, k2 = dgamma / M.
      sc = fl(gamma invstd): one rounding; 2 u |sc|.
      B = -sc invstd k2: sc (u), two products (2 u), k2 = fl(dgamma fl(1 / M)) (2 u): 6 u |B| (one spare), and
        |sc invstd| dg carried from dgamma.
      D = -sc k1 - B mean: the same count gives 6 u (|sc k1| + |B mean|) for the roundings of its own terms, then
        |sc| db from k1 and |mean| times B's whole bound. This is where the table loses accuracy in proportion to
        |mean| / std: B mean is large against D when the channel's mean is.
      shift = fma(-mean, sc, beta): 3 u (|beta| + |mean sc|).
      dx = fma(sc, g, fma(B, x, D)), per element, T = |sc g| + |B x| + |B mean| + |sc k1| (o['t_abs']):
        |g| d sc: u |sc g|;  |x| (B's own roundings): 6 u |B x|;  D's own: 6 u (|sc k1| + |B mean|) + 6 u |B mean|;
        the inner fma: u (|B x| + |sc k1| + |B mean|);  the outer: u T.  Per term at most 14 u; 16 u T taken.
        Carried from the sums: |x| |sc invstd| dg + (|sc| db + |mean| |sc invstd| dg)
          = |sc invstd| dg (|x| + |mean|) + |sc| db.
        (|x| + |mean|, not |x - mean|: the affine form is what the consumers apply on load, so the bound describes it.)
    """
    M = o["M"]
    sc, B, mu, is_ = o["sc"].abs(), o["B"].abs(), o["mu"].abs(), o["is"].abs()
    db_b, dg_b = k * U * o["abs_dbeta"], k * U * o["abs_dgamma"]
    db, dg = db_b / M, dg_b / M
    sck1 = sc * o["k1"].abs()
    B_b = 6 * U * B + sc * is_ * dg
    D_b = 6 * U * (sck1 + B * mu) + sc * db + mu * B_b
    table = torch.stack([2 * U * sc, B_b, D_b, 3 * U * (o["beta"].abs() + mu * sc)])
    shape = o["t_abs"].shape
    C = shape[-1]
    dx = 16 * U * o["t_abs"].reshape(-1, C) + sc * is_ * dg * (o["x_abs"].reshape(-1, C) + mu) + sc * db
    return {"dbeta": db_b, "dgamma": dg_b, "table": table, "dx": dx.reshape(shape)}


# ----------------------------------------------------------------------------------------------- stem: BN + pool
def pool_windows(z, pad):
    """[N, H, W, C] -> [N, Ho, Wo, 9, C]: the 3x3 / stride 2 / pad 1 windows, tap dh * 3 + dw = pixel
    (2 ho - 1 + dh, 2 wo - 1 + dw), `pad` outside the image."""
    N, H, W, C = z.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    zp = torch.full((N, 2 * Ho + 1, 2 * Wo + 1, C), pad, dtype=z.dtype, device=z.device)
    zp[:, 1:H + 1, 1:W + 1] = z
    taps = [zp[:, dh:dh + 2 * Ho:2, dw:dw + 2 * Wo:2] for dh in range(3) for dw in range(3)]
    return torch.stack(taps, 3)


def pool_route(dpool, idx, H, W, dtype=F64, rounded=True):
    """The max-pool gradient of each input pixel: dpool of every covering window whose winner (idx, the tap number) it
    is, summed, then rounded to bf16 as the kernel documents (the gradient as it would be stored); rounded=False:
    the unrounded sum in `dtype`."""
    N, Ho, Wo, C = dpool.shape
    dz = torch.zeros(N, H, W, C, dtype=dtype, device=dpool.device)
    d = dpool.to(dtype)
    ho, wo = torch.arange(Ho, device=dpool.device), torch.arange(Wo, device=dpool.device)
    for dh in range(3):
        for dw in range(3):
            h, w = 2 * ho - 1 + dh, 2 * wo - 1 + dw
            hv, wv = (h >= 0) & (h < H), (w >= 0) & (w < W)
            if not (bool(hv.any()) and bool(wv.any())):
                continue
            src = torch.where(idx == dh * 3 + dw, d, torch.zeros_like(d))
            dz[:, h[hv][:, None], w[wv][None, :]] += src[:, ho[hv][:, None], wo[wv][None, :]]
    return dz.float().bfloat16() if rounded else dz


def pool_bn_bwd(dpool, idx, x, bits, mean, invstd, gamma, beta, dtype=F64, from_sums=False):
    """Backward of BN + ReLU + max pool: route dpool to the winners (the kernel's idx), then bn_bwd with the ReLU bits
    of the BatchNorm output (relu_x). from_sums: dgamma / dbeta (and through them the table) come from sums that the
    data gradients took over the pooled gradient itself, so a pixel that wins several windows enters them unrounded;
    the apply pass still routes and rounds."""
    H, W = x.shape[1], x.shape[2]
    unrounded = pool_route(dpool, idx, H, W, rounded=False) if from_sums else None
    return bn_bwd(pool_route(dpool, idx, H, W), x, bits, mean, invstd, gamma, beta, dtype, dy_sums=unrounded)


# ----------------------------------------------------------------------------------------------- inputs
def bn_inputs(shape, device, seed=3, edge=None, res=False, dual=False):
    """x, dy (bf16, `shape` = (..., C)), gamma, beta (fp32), optionally res, or the second BatchNorm's x2 / gamma2 /
    beta2. edge: None randn * 3 + 1 | 'offset' mean 32, std 1 (mean^2 / var about 1000) | 'const' one channel constant
    at 0.75 | 'tiny' x * 1e-3 (invstd about 300) | 'mixed' per-channel scales 1e-2 .. 1e2 | 'zero_g' one channel's dy
    all zero."""
    torch.manual_seed(seed)
    C = shape[-1]
    x = torch.randn(*shape, device=device) * 3 + 1
    dy = torch.randn(*shape, device=device)
    c0 = edge_channel(C)
    if edge == "offset":
        x = torch.randn(*shape, device=device) + 32
    elif edge == "const":
        x[..., c0] = CONST_VALUE
    elif edge == "tiny":
        x = x * 1e-3
    elif edge == "mixed":
        x = x * torch.logspace(-2, 2, C, device=device)[torch.randperm(C, device=device)]
    elif edge == "zero_g":
        dy[..., c0] = 0.0
    else:
        assert edge is None, edge
    d = {"x": x.bfloat16(), "dy": dy.bfloat16(), "gamma": torch.rand(C, device=device) + 0.5,
         "beta": torch.randn(C, device=device) * 0.5, "res": None}
    if res:
        d["res"] = torch.randn(*shape, device=device).bfloat16()
    if dual:
        d["x2"] = (torch.randn(*shape, device=device) * 2 - 0.5 + (16 if edge == "offset" else 0)).bfloat16()
        d["gamma2"] = torch.rand(C, device=device) + 0.5
        d["beta2"] = torch.randn(C, device=device) * 0.5
    return d


def sums_from(x, nrep):
    """Conv-epilogue-style replica sums fp32 [nrep, 2, C] = (sum x, sum x^2): rows dealt to replicas as x[r::nrep],
    accumulated in fp64 per replica, rounded to fp32."""
    xs = _rows(x, F64)
    out = torch.zeros(nrep, 2, xs.shape[1], dtype=F64, device=x.device)
    for r in range(nrep):
        part = xs[r::nrep]
        out[r, 0], out[r, 1] = part.sum(0), (part * part).sum(0)
    return out.float().contiguous()


def bwd_sums_from(g, x, mean, nrep, second=False):
    """The data gradients' epilogue sums fp32 [nrep, 2, C] = (sum g, sum g (x - mean)) over the masked gradient g, dealt
    as sums_from does. second: the two-BatchNorm form's sums2, whose slot 0 no kernel reads (sum g is shared): it is
    filled with NaN so a read shows."""
    gs, xs = _rows(g, F64), _rows(x, F64)
    mu = mean.to(F64)
    out = torch.zeros(nrep, 2, xs.shape[1], dtype=F64, device=x.device)
    for r in range(nrep):
        out[r, 0] = gs[r::nrep].sum(0)
        out[r, 1] = (gs[r::nrep] * (xs[r::nrep] - mu)).sum(0)
    if second:
        out[:, 0] = float("nan")
    return out.float().contiguous()


# ----------------------------------------------------------------------------------------------- checks
def check_stats_own(mean, invstd, st, what=""):
    """A reduction over x itself (the shifted Chan merge): mean within 8 u mean_abs, invstd within 32 u relative --
    at every edge, 'offset' included: the shift takes the channel's mean out before anything is squared."""
    assert_within(mean, st["mean"], 8 * U * st["mean_abs"], what + "mean")
    assert_within(invstd, st["invstd"], 32 * U * st["invstd"], what + "invstd")


def check_stats_sums(mean, invstd, st, eps=EPS, what=""):
    """Statistics from replica sums: the derived conditioning bounds."""
    assert_within(mean, st["mean"], mean_bound_sums(st), what + "mean")
    lo, hi = invstd_interval(st["var"], var_bound_sums(st), eps)
    assert_between(invstd, lo, hi, what + "invstd")


def stats_carried(st, own, eps=EPS):
    """(mean bound, unbiased-variance bound) that check_running carries: own reduce -- 8 u mean_abs, and invstd to
    32 u relative is var + eps to 64 u; sums -- mean_bound_sums, var_bound_sums; both scaled to the unbiased form."""
    n = st["count"]
    f = n / (n - 1.0) if n > 1 else 1.0
    if own:
        return 8 * U * st["mean_abs"], 64 * U * (st["var"] + eps) * f
    return mean_bound_sums(st), var_bound_sums(st) * f


def check_running(run_mean, run_var, rm0, rv0, st, own, momentum=MOMENTUM, eps=EPS, what=""):
    """run = (1 - m) run0 + m stat: 4 u of the two terms (1 - m in fp32, two products, one sum) plus m times the
    statistic's own bound."""
    r = run_update(rm0, rv0, st, momentum)
    mb, vb = stats_carried(st, own, eps)
    assert_within(run_mean, r["run_mean"], 4 * U * r["abs_mean"] + momentum * mb, what + "run_mean")
    assert_within(run_var, r["run_var"], 4 * U * r["abs_var"] + momentum * vb, what + "run_var")


def check_fwd(y, mask, o64, o32, what=""):
    """y per element; the packed mask bit-equal to the checked y's own sign."""
    assert y.dtype == torch.bfloat16 and y.shape == o64["y"].shape
    assert_rounded(y, o64["y"], y_delta(o64, o32), what + "y")
    if mask is not None:
        assert torch.equal(unpack_bits(mask, y.shape), y > 0), what + "mask is not y > 0"


def check_table(params, o64, bounds, what=""):
    C = o64["table"].shape[1]
    assert params.dtype == torch.float32 and params.numel() == 4 * C
    got = params.reshape(4, C)
    for i, name in enumerate(["sc", "B", "D", "shift"]):
        assert_within(got[i], o64["table"][i], bounds["table"][i], what + "table " + name)


def check_bwd(dx, dres, dgamma, dbeta, o64, what="", bounds=None):
    b = bounds or bn_bwd_bounds(o64)
    assert_fp32_sum(dbeta, o64["dbeta"], o64["abs_dbeta"], what=what + "dbeta")
    assert_fp32_sum(dgamma, o64["dgamma"], o64["abs_dgamma"], what=what + "dgamma")
    if dx is not None:
        assert dx.dtype == torch.bfloat16
        assert_rounded(dx, o64["dx"], b["dx"], what + "dx")
    if dres is not None:
        assert torch.equal(dres, o64["g"].float().bfloat16()), what + "dres is not the masked dy"
