"""fp64 oracles of the row-wise kernels (norm.hip, xent.hip, elementwise.hip) and the per-element comparisons.

Every oracle is the textbook formula written out in torch, evaluated in `dtype` (fp64 unless asked otherwise) on the
device its inputs live on. It takes the kernel's exact inputs (bf16 / fp32 tensors, cast up) and returns what the
kernel returns plus the sums of absolute terms the error bounds are made of. Evaluated with dtype=torch.float32 the
same code is "a correct fp32 evaluation": the distance between the two evaluations is what the bounds' `delta` is
measured from (reference against reference, never the kernel's output).

Nothing here imports k8s_amd: the package's CPU reference shares the kernels' formulas.
"""
import math

import torch

U = 2.0 ** -24          # fp32 unit roundoff
BF16_ULP = 2.0 ** -7    # one bf16 ulp, relative
FP32_TINY = 2.0 ** -126  # smallest normal fp32: a correct fp32 evaluation may flush anything below it to zero
F64 = torch.float64


# ----------------------------------------------------------------------------------------------- comparisons
def _worst(excess, got, want, bound, what):
    i = int(torch.argmax(excess.reshape(-1)))
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), excess.shape)) if excess.dim() else ()
    return "%s: worst element %s got %.9g want %.9g |diff| %.3g bound %.3g" % (
        what, idx, float(got.reshape(-1)[i]), float(want.reshape(-1)[i]),
        abs(float(got.reshape(-1)[i]) - float(want.reshape(-1)[i])), float(bound.reshape(-1)[i]))


def assert_within(got, want64, bound, what="value"):
    """Every element: |got - want| <= bound (tensor or scalar). NaN on either side fails."""
    assert got.shape == want64.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(want64.shape))
    g = got.to(F64)
    bound = bound.expand_as(want64) if isinstance(bound, torch.Tensor) else torch.full_like(want64, float(bound))
    diff = (g - want64).abs()
    bad = ~(diff <= bound)  # a NaN on either side is bad
    if bool(bad.any()):
        excess = torch.where(bad, torch.where(torch.isfinite(diff - bound), diff - bound,
                                              torch.full_like(diff, float("inf"))), torch.full_like(diff, -1.0))
        raise AssertionError(_worst(excess, g, want64, bound, what) + " (%d of %d elements out)" % (
            int(bad.sum()), bad.numel()))


def _rel(got):
    if got.dtype == torch.bfloat16:
        return BF16_ULP
    assert got.dtype == torch.float32, got.dtype
    return 0.0


def assert_rounded(got, want64, delta, what="value"):
    """Every element: |got - want| <= r |want| + delta, r = 2^-7 (one bf16 ulp) for a bf16 output, 0 for fp32.
    delta (scalar or tensor) is the error of a correct fp32 evaluation."""
    assert_within(got, want64, _rel(got) * want64.abs() + delta, what)


def assert_fp32_sum(got, want64, abs_terms64, k=32, extra=0.0, what="sum"):
    """Every element: |got - want| <= k 2^-24 sum|terms| (+ extra, a derived allowance)."""
    assert got.dtype == torch.float32, got.dtype
    assert_within(got, want64, k * U * abs_terms64 + extra, what)


def bf16_spacing(t):
    """The spacing of bf16 numbers at each element's binade (0 for a zero)."""
    _, e = torch.frexp(t.to(F64))  # |t| = m 2^e, m in [0.5, 1)
    spacing = torch.ldexp(torch.ones_like(e, dtype=F64), e - 8)
    return torch.where(t == 0, torch.zeros_like(spacing), spacing)


def assert_nearest(got, want64, delta, what="value"):
    """Every element of a bf16 output is a round-to-nearest of some value within delta of want:
    |got - want| <= spacing(got) / 2 + delta. Tighter than assert_rounded by a factor of two to four; a systematic
    relative error well under a bf16 ulp shows here on the elements that sit next to a rounding boundary."""
    assert got.dtype == torch.bfloat16, got.dtype
    assert_within(got, want64, 0.5 * bf16_spacing(got) + delta + FP32_TINY, what)


def measured_delta(want32, want64, margin=16.0):
    """margin x max|fp32 evaluation - fp64 evaluation| of the same oracle on the same inputs."""
    d = (want32.to(F64) - want64).abs()
    d = d[torch.isfinite(d)]
    return margin * float(d.max()) if d.numel() else 0.0


# ----------------------------------------------------------------------------------------------- LayerNorm / RMSNorm
def norm_fwd(x, res, gamma, beta, eps, rms, dtype=F64):
    """y, mean, rstd of a row norm over x (+ res). xsum is the stored bf16 sum (None without res); mean_abs is
    mean_j |x_j| per row; xhat the normalised row."""
    xs = x.to(dtype)
    xsum = None
    if res is not None:
        xs = xs + res.to(dtype)
        xsum = (x.float() + res.float()).bfloat16()
    D = xs.shape[-1]
    if rms:
        mean = torch.zeros(xs.shape[:-1], dtype=dtype, device=xs.device)
        var = (xs * xs).sum(-1) / D
    else:
        mean = xs.sum(-1) / D
        var = ((xs - mean[..., None]) ** 2).sum(-1) / D
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (xs - mean[..., None]) * rstd[..., None]
    y = xhat * gamma.to(dtype)
    if not rms:
        y = y + beta.to(dtype)
    return {"y": y, "mean": mean, "rstd": rstd, "xsum": xsum, "mean_abs": xs.abs().sum(-1) / D, "xhat": xhat}


def norm_y_delta(f64, gamma, measured):
    """delta of y = (x - mean) rstd gamma + beta: the measured fp32-against-fp64 distance, plus the bounds asserted on
    mean (8 u mean_j |x_j|) and rstd (32 u relative) carried through the formula -- d y / d mean = -rstd gamma,
    d y / d rstd = (x - mean) gamma -- so 8 u mean|x| rstd |gamma| + 32 u |xhat gamma|. The measurement alone can
    miss the first: torch sums a row of equal values exactly, a tree of fp32 adds in another order need not, and
    rstd = eps^-1/2 magnifies the difference."""
    gm = gamma.to(F64).abs()
    return measured + 8 * U * (f64["mean_abs"] * f64["rstd"])[..., None] * gm + 32 * U * (f64["xhat"] * gm).abs()


def norm_bwd(dy, x, gamma, mean, rstd, dres, rms, dtype=F64):
    """The backward of norm_fwd from the saved mean / rstd (inputs: the caller hands the same ones to the kernel).
    dx (+ dres), dgamma = sum_r dy xhat, dbeta = sum_r dy, dsum = sum_r dx (without dres), and per column the sums of
    |dy xhat|, |dy|, |dx| (abs_dgamma, abs_dbeta, abs_dx) and the absolute terms dsum is bounded by (abs_dsum)."""
    g, xs, gm = dy.to(dtype), x.to(dtype), gamma.to(dtype)
    rs = rstd.to(dtype)[..., None]
    mu = 0.0 if rms else mean.to(dtype)[..., None]
    xhat = (xs - mu) * rs
    gg = g * gm
    D = xs.shape[-1]
    b = (gg * xhat).sum(-1, keepdim=True) / D
    a = 0.0 if rms else gg.sum(-1, keepdim=True) / D
    dx0 = rs * (gg - a - xhat * b)
    dx = dx0 if dres is None else dx0 + dres.to(dtype)
    flat = lambda t: t.reshape(-1, D)  # noqa: E731
    # The terms of dgamma and dbeta are products of inputs: an fp32 term is off by a few u of itself. A term of dsum
    # is the computed dx = rs (gg - a - xhat b), a difference: its fp32 error is a few u of rs (|gg| + |a'| + |xhat b'|)
    # whatever is left after the cancellation, and a, b are themselves fp32 row means, off by a few u of
    # a' = mean_j |gg|, b' = mean_j |gg xhat| rather than of |a|, |b|. Those magnitudes are dsum's absolute terms
    # (one row, R = 1, shows it: sum_r |dx| alone fails a plain fp32 evaluation of the formula).
    am = 0.0 if rms else gg.abs().sum(-1, keepdim=True) / D
    bm = (gg * xhat).abs().sum(-1, keepdim=True) / D
    parts = rs.abs() * (gg.abs() + am + xhat.abs() * bm)
    return {"dx": dx, "dgamma": flat(g * xhat).sum(0), "dbeta": flat(g).sum(0), "dsum": flat(dx0).sum(0),
            "abs_dgamma": flat(g * xhat).abs().sum(0), "abs_dbeta": flat(g).abs().sum(0),
            "abs_dx": flat(dx0).abs().sum(0), "abs_dsum": flat(parts).sum(0)}


# ----------------------------------------------------------------------------------------------- cross entropy
def xent_fwd(logits, labels, ignore_index, smoothing, dtype=F64):
    """lse and loss per row (ignored rows: loss 0). -inf logits are masked classes: logsumexp skips them; with
    smoothing > 0 they would make the loss infinite, as in torch. Also |x_label| and mean_j |x_j| for the bound."""
    x = logits.to(dtype)
    R, V = x.shape
    lse = torch.logsumexp(x, -1)
    valid = labels != ignore_index
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    xl = x.gather(1, lab[:, None])[:, 0]
    loss = lse - xl
    mean_abs = torch.zeros_like(lse)
    if smoothing > 0:
        loss = (1.0 - smoothing) * loss + smoothing * (lse - x.sum(-1) / V)
        mean_abs = x.abs().sum(-1) / V
    zero = torch.zeros_like(loss)
    return {"lse": lse, "loss": torch.where(valid, loss, zero), "xl_abs": torch.where(valid, xl.abs(), zero),
            "mean_abs": mean_abs, "valid": valid}


def lse_bound(lse64):
    """|lse - lse64| <= 32 u max(1, |lse64|)"""
    return 32 * U * lse64.abs().clamp(min=1.0)


def loss_bound(o, smoothing):
    """64 u (|lse64| + |x_label| + smoothing mean_j |x_j|) from xent_fwd's result"""
    return 64 * U * (o["lse"].abs() + o["xl_abs"] + smoothing * o["mean_abs"])


def xent_bwd(logits, labels, lse, scale, ignore_index, smoothing, dtype=F64):
    """d loss / d logits from the saved lse: (p - off - on onehot) sc with p = exp(x - lse), off = smoothing / V,
    on = 1 - smoothing, sc the scalar or per-row scale (0 for an ignored row). Also p, |x - lse|, onehot, |sc|."""
    x = logits.to(dtype)
    R, V = x.shape
    valid = labels != ignore_index
    sc = scale.to(dtype).reshape(-1)
    sc = sc.expand(R) if sc.numel() == 1 else sc
    sc = torch.where(valid, sc, torch.zeros_like(sc))[:, None]
    dist = x - lse.to(dtype)[:, None]
    p = torch.exp(dist)
    onehot = torch.zeros_like(x)
    onehot.scatter_(1, torch.where(valid, labels, torch.zeros_like(labels))[:, None], 1.0)
    off, on = smoothing / V, 1.0 - smoothing
    grad = (p - off - on * onehot) * sc
    grad = torch.where(sc == 0, torch.zeros_like(grad), grad)  # an ignored row is zero, not 0 * inf
    return {"grad": grad, "p": p, "dist": dist.abs(), "onehot": onehot, "sc_abs": sc.abs(), "off": off, "on": on}


def xent_grad_bound(o, bf16_out):
    """(8 + 2 |x - lse|) u p |sc| + 4 u (off + on onehot) |sc|, + 2^-7 |want| for bf16 logits.
    Two things the form needs to be usable on every element: where p == 0 (a -inf logit) the first term is 0, not
    inf * 0; and p |sc| below the smallest normal fp32 may come back as zero from a correct fp32 evaluation (exp
    underflows near x - lse = -87), so 2^-126 |sc| is added."""
    first = torch.where(o["p"] > 0, (8 + 2 * o["dist"]) * o["p"], torch.zeros_like(o["p"]))
    b = U * (first + 4 * (o["off"] + o["on"] * o["onehot"])) * o["sc_abs"] + FP32_TINY * o["sc_abs"]
    if bf16_out:
        # a bf16 result below bf16's smallest normal (the same 2^-126) is flushed or loses bits as well
        b = b + BF16_ULP * o["grad"].abs() + FP32_TINY
    return b


# ----------------------------------------------------------------------------------------------- elementwise
def _swiglu_split(gu, blk):
    F2 = gu.shape[-1]
    F = F2 // 2
    if not blk:
        return gu[..., :F], gu[..., F:]
    v = gu.reshape(*gu.shape[:-1], F // blk, 2, blk)  # blocks of blk gate columns then blk up columns
    return v[..., 0, :].reshape(*gu.shape[:-1], F), v[..., 1, :].reshape(*gu.shape[:-1], F)


def _swiglu_join(dg, du, blk):
    if not blk:
        return torch.cat([dg, du], -1)
    F = dg.shape[-1]
    s = dg.shape[:-1]
    return torch.stack([dg.reshape(*s, F // blk, blk), du.reshape(*s, F // blk, blk)], -2).reshape(*s, 2 * F)


def swiglu_fwd(gu, blk=0, dtype=F64):
    g, u = _swiglu_split(gu.to(dtype), blk)
    return g * torch.sigmoid(g) * u


def swiglu_bwd(gu, dy, blk=0, dtype=F64):
    g, u = _swiglu_split(gu.to(dtype), blk)
    d = dy.to(dtype)
    s = torch.sigmoid(g)
    return _swiglu_join(d * u * (s * (1 + g * (1 - s))), d * g * s, blk)


GELU_K0, GELU_K1 = math.sqrt(2.0 / math.pi), 0.044715


def gelu_tanh_bwd(dy, pre, dtype=F64):
    x = pre.to(dtype)
    t = torch.tanh(GELU_K0 * (x + GELU_K1 * x ** 3))
    return dy.to(dtype) * (0.5 * (1 + t) + 0.5 * x * (1 - t * t) * GELU_K0 * (1 + 3 * GELU_K1 * x * x))


def gelu_tanh_bwd_delta(dy, pre):
    """The error of an fp32 evaluation of g = dy (T1 + T2), T1 = (1 + t) / 2, T2 = x (1 - t^2) k0 (1 + 3 k1 x^2) / 2,
    t = tanh(a), a = k0 (x + k1 x^3), derived per element (u = 2^-24; exp, reciprocal and tanh taken as good to 2 ulp,
    4 u, which holds for the hardware's exp2 / rcp and for libm):
      a: five roundings, 5 u |a|. As t = 1 - 2 / (1 + e), e = exp(2 a): the exponent 2 a log2(e) adds the constant's
         rounding and one product, 7 u |2 a| in all, so e is off by (14 |a| + 4) u of itself; 1 + e and the
         reciprocal add 5 u, the last subtraction u |t| <= u. With 2 e / (1 + e)^2 = (1 - t^2) / 2:
         dt <= ((1 - t^2) (7 |a| + 2) + 11) u, which also covers a tanh good to 4 u;
      T1 + T2: d(T1 + T2) / dt = 1 / 2 - x t k0 (1 + 3 k1 x^2), and the products and sums of T1, T2 and dy add at
         most 12 u (|T1| + |T2|).
    A whole-tensor measurement with its x16 margin is 150 u of the largest element; this is 20 to 40 u of each."""
    x = pre.to(F64)
    a = GELU_K0 * (x + GELU_K1 * x ** 3)
    t = torch.tanh(a)
    poly = GELU_K0 * (1 + 3 * GELU_K1 * x * x)
    dt = (1 - t * t) * (7 * a.abs() + 2) + 11
    t1, t2 = 0.5 * (1 + t), (0.5 * x * (1 - t * t) * poly).abs()
    return U * dy.to(F64).abs() * (dt * (0.5 + (x * t).abs() * poly) + 12 * (t1 + t2))


def relu_bwd(dy, y, dtype=F64):
    return dy.to(dtype) * (y > 0).to(dtype)


def rope(x, pos, table, H, inverse=False, dtype=F64):
    """Rotate-half rotary embedding of x [T, H * D] with table [maxpos, D / 2, (cos, sin)]:
    out1 = x1 c - x2 s, out2 = x2 c + x1 s (s negated for the inverse). Returns (out, abs) with abs the
    |x1 c| + |x2 s| (first half) and |x2 c| + |x1 s| (second half) the rounding bound is made of."""
    T = x.shape[0]
    D = table.shape[1] * 2
    xs = x.to(dtype).reshape(T, H, D)
    cs = table.to(dtype)[pos.long()]
    c, s = cs[..., 0][:, None, :], cs[..., 1][:, None, :]
    if inverse:
        s = -s
    x1, x2 = xs[..., : D // 2], xs[..., D // 2:]
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(T, H * D)
    ab = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1).reshape(T, H * D)
    return out, ab


def colsum(x, dtype=F64):
    """Column sums of [R, C] and the sums of absolute values."""
    v = x.to(dtype).reshape(-1, x.shape[-1])
    return v.sum(0), v.abs().sum(0)


# ----------------------------------------------------------------------------------------------- input recipes
# Shared by the GPU tests (kernel against oracle) and the CPU tests (fp32 evaluation of the oracle against the same
# bounds): the distributions are the same, the device's generator supplies the numbers.
EPS = 1e-5
SWIGLU_EDGE = [0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 0.5]  # exp / rcp saturate at the large ones
GELU_EDGE = [0.0, 0.75, -0.75, 10.0, -10.0, 20.0, -20.0, 1.0]      # tanh saturates at the large ones


def norm_inputs(R, D, rms, res, device, seed=1, edge=None):
    """x, r, gamma, beta, dy, dres of one norm case. edge: 'small' (variance below eps), 'offset' (x + 64), 'equal'
    (row 5 all 0.75: rstd = eps^-1/2, y = beta), 'gamma' (zeros and negative entries)."""
    torch.manual_seed(seed)
    x = torch.randn(R, D, device=device)
    if edge == "small":
        x = x * 1e-3
    elif edge == "offset":
        x = x + 64
    elif edge == "equal":
        x[min(5, R - 1)] = 0.75
    x = x.bfloat16()
    r = torch.randn(R, D, device=device).bfloat16() if res else None
    g = torch.rand(D, device=device) + 0.5
    if edge == "gamma":
        g[::3] = 0.0
        g[1::3] = -g[1::3]
    b = None if rms else torch.randn(D, device=device)
    dy = torch.randn(R, D, device=device).bfloat16()
    dres = torch.randn(R, D, device=device).bfloat16() if res else None
    return x, r, g, b, dy, dres


def xent_logits(R, V, dt, device, seed=2, mul=4.0, shift=0.0):
    torch.manual_seed(seed)
    return (torch.randn(R, V, device=device) * mul + shift).to(dt)


def xent_labels(R, V, device, ignore_index=-100):
    """Row 0: column 0; row 1: column V - 1; row 2: inside the scalar tail past the last whole 8-column vector (the
    middle column when V % 8 == 0); row 3: ignored; the rest spread over the row."""
    tail = (V // 8) * 8 + (V % 8) // 2 if V % 8 else V // 2
    lab = [(i * 7919 + 13) % V for i in range(R)]
    for i, v in enumerate([0, V - 1, tail, ignore_index]):
        if i < R:
            lab[i] = v
    return torch.tensor(lab, device=device, dtype=torch.int64)


def swiglu_inputs(T, F, device, seed=8):
    torch.manual_seed(seed)
    gu = torch.randn(T, 2 * F, device=device)
    gu[0, :8] = torch.tensor(SWIGLU_EDGE, device=device)  # gate columns in the plain and the blocked layout alike
    return gu.bfloat16(), torch.randn(T, F, device=device).bfloat16()


def act_inputs(R, C, device, seed=9):
    torch.manual_seed(seed)
    pre = torch.randn(R, C, device=device) * 1.5
    pre[0, :8] = torch.tensor(GELU_EDGE, device=device)
    return torch.randn(R, C, device=device).bfloat16(), pre.bfloat16()


def rope_inputs(T, H, D, maxpos, device, seed=10, theta=10000.0):
    """x [T, H * D] bf16, shuffled int32 positions that include maxpos - 1, the [maxpos, D / 2, (cos, sin)] table."""
    torch.manual_seed(seed)
    x = torch.randn(T, H * D, device=device).bfloat16()
    pos = torch.randperm(maxpos, device=device)[:T].to(torch.int32)
    pos[T // 2] = maxpos - 1
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=F64) / D))
    ang = torch.arange(maxpos, dtype=F64)[:, None] * inv[None, :]
    return x, pos, torch.stack([ang.cos(), ang.sin()], -1).float().to(device)
