"""Plain-PyTorch fp32 reference implementations of every fused kernel.

These are (a) the numerics oracles the GPU tests compare the HIP kernels
against and (b) the CPU execution path used by the CPU-only test tier and by
CPU rehearsals of the distributed code (gloo). They are written from the
mathematical definitions, in fp32, with no fusion.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch


# --------------------------------------------------------------------------- batchnorm (NHWC)
def bn_fwd(x, res, gamma, beta, run_mean, run_var, training, momentum, eps, relu):
    C = x.shape[-1]
    xf = x.float().reshape(-1, C)
    if training:
        mean = xf.mean(0)
        var = xf.var(0, unbiased=False)
        if run_mean is not None:
            n = xf.shape[0]
            unb = var * n / max(n - 1, 1)
            run_mean.mul_(1 - momentum).add_(momentum * mean)
            run_var.mul_(1 - momentum).add_(momentum * unb)
    else:
        mean, var = run_mean.float(), run_var.float()
    invstd = torch.rsqrt(var + eps)
    y = (xf - mean) * invstd * gamma.float() + beta.float()
    if res is not None:
        y = y + res.float().reshape(-1, C)
    if relu:
        y = torch.relu(y)
    return y.reshape(x.shape).to(x.dtype), mean, invstd


def bn_bwd(dy, x, y, mean, invstd, gamma):
    C = x.shape[-1]
    g = dy.float().reshape(-1, C)
    if y is not None:
        g = g * (y.float().reshape(-1, C) > 0)
    xh = (x.float().reshape(-1, C) - mean) * invstd
    M = g.shape[0]
    sd = g.sum(0)
    sx = (g * xh).sum(0)
    dx = gamma.float() * invstd * (g - sd / M - xh * sx / M)
    return dx.reshape(x.shape).to(x.dtype), g.reshape(x.shape).to(x.dtype), sx, sd


# --------------------------------------------------------------------------- layernorm / rmsnorm
def norm_fwd(x, res, gamma, beta, eps, rms):
    xs = x.float() if res is None else x.float() + res.float()
    if rms:
        mean = torch.zeros(1)
        rstd = torch.rsqrt(xs.pow(2).mean(-1) + eps)
        y = xs * rstd.unsqueeze(-1) * gamma.float()
    else:
        mean = xs.mean(-1)
        var = (xs - mean.unsqueeze(-1)).pow(2).mean(-1)
        rstd = torch.rsqrt(var + eps)
        y = (xs - mean.unsqueeze(-1)) * rstd.unsqueeze(-1) * gamma.float() + beta.float()
    xsum = xs.to(x.dtype) if res is not None else None
    return y.to(x.dtype), mean.reshape(-1), rstd.reshape(-1), xsum


def norm_bwd(dy, x, gamma, mean, rstd, dres, rms):
    D = x.shape[-1]
    g = dy.float().reshape(-1, D)
    xf = x.float().reshape(-1, D)
    r = rstd.reshape(-1, 1)
    mu = 0.0 if rms else mean.reshape(-1, 1)
    xh = (xf - mu) * r
    gg = g * gamma.float()
    a = gg.mean(-1, keepdim=True)
    b = (gg * xh).mean(-1, keepdim=True)
    dx = r * (gg - (0.0 if rms else a) - xh * b)
    if dres is not None:
        dx = dx + dres.float().reshape(-1, D)
    dgamma = (g * xh).sum(0)
    dbeta = g.sum(0)
    return dx.reshape(x.shape).to(x.dtype), dgamma, dbeta


# --------------------------------------------------------------------------- dropout (counter generator)
# The definition the kernels implement (csrc/kernels/rng.h), in torch integer ops: int64 values masked to 32 bits, on
# whatever device the state / rows live on, with no host read of a device tensor -- so it is both the CPU oracle and the
# on-GPU fallback under graph capture.
#   rowkey = Philox4x32-10(counter = (row lo, row hi, site, step lo), key = (seed lo, seed hi))[0]
#   keep   = mix32(rowkey ^ (col * 0x9E3779B1)) >= thr
_M32 = 0xFFFFFFFF


def drop_params(p: float):
    """(thr, scale) of a drop probability in [0, 1): thr = min(floor(p 2^32 + 0.5), 2^32 - 1), scale = the fp32 value
    of 1 / (1 - thr / 2^32) -- the quantised probability, so E[keep * scale] = 1."""
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout probability must be in [0, 1), got %r" % (p,))
    thr = min(int(math.floor(p * 4294967296.0 + 0.5)), _M32)
    scale = torch.tensor(1.0 / (1.0 - thr / 4294967296.0), dtype=torch.float32).item()
    return thr, scale


def _mulhilo32(a: int, b):
    """(hi, lo) 32-bit halves of a * b for a constant a < 2^32 and an int64 tensor b of values < 2^32."""
    t1 = (b & 0xFFFF) * a   # < 2^48
    t2 = (b >> 16) * a      # < 2^48, weight 2^16
    low = ((t2 & 0xFFFF) << 16) + t1
    return (t2 >> 16) + (low >> 32), low & _M32


def _mul32(x, c: int):
    """x * c mod 2^32 for an int64 tensor x of values < 2^32 and a constant c < 2^32."""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & _M32


def philox4x32(counter, key):
    """Random123 Philox4x32-10 on int64 tensors holding 32-bit words: counter (c0, c1, c2, c3), key (k0, k1)."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        hi0, lo0 = _mulhilo32(0xD2511F53, c0)
        hi1, lo1 = _mulhilo32(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def _drop_state(state, device):
    """int64 [seed, step] on ``device`` from a DropoutState, a tensor or a (seed, step) pair of ints."""
    t = getattr(state, "tensor", state)
    if isinstance(t, torch.Tensor):
        return t if device is None else t.to(device)

    def wrap(v):  # any 64-bit seed as the int64 with the same bits
        v = int(v) & 0xFFFFFFFFFFFFFFFF
        return v - (1 << 64) if v >= (1 << 63) else v

    return torch.tensor([wrap(t[0]), wrap(t[1])], dtype=torch.int64, device=device)


def dropout_rowkey(state, site: int, rows):
    """Philox rowkeys (int64 tensor of 32-bit values, ``rows``' shape) of the int64 row indices ``rows``."""
    rows = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(rows, dtype=torch.int64)
    st = _drop_state(state, rows.device)
    rows = rows.to(torch.int64)
    seed, step = st[0], st[1]
    z = torch.zeros_like(rows)
    counter = (rows & _M32, (rows >> 32) & _M32, z + int(site), z + (step & _M32))
    key = (z + (seed & _M32), z + ((seed >> 32) & _M32))
    return philox4x32(counter, key)[0]


def counter_bits(state, site: int, rows, cols):
    """The counter generator's 32-bit value (int64 tensor of values < 2^32, ``rows``' shape + [len(cols)]) at
    ``(seed, step, site, row, col)``: ``rows`` int64 row indices (a tensor, or a count meaning 0 .. n - 1), ``cols``
    likewise the columns; ``state`` a DropoutState, its int64 [seed, step] tensor, or a (seed, step) pair. What
    ``dropout_keep`` compares with its threshold, and what ``ops.sampling`` draws its uniform number from."""
    t = getattr(state, "tensor", state)
    dev = t.device if isinstance(t, torch.Tensor) else None
    if not isinstance(rows, torch.Tensor):
        rows = torch.arange(int(rows), dtype=torch.int64, device=dev)
    if not isinstance(cols, torch.Tensor):
        cols = torch.arange(int(cols), dtype=torch.int64, device=rows.device)
    rk = dropout_rowkey(state, site, rows).unsqueeze(-1)
    x = rk ^ _mul32(cols.to(device=rows.device, dtype=torch.int64) & _M32, 0x9E3779B1)
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def dropout_keep(state, site: int, rows, cols, p: float):
    """Keep mask (bool, ``rows``' shape + [len(cols)]) of the dropout site ``site``: ``counter_bits`` of the same
    arguments at or above the threshold of ``p``."""
    thr, _ = drop_params(p)
    return counter_bits(state, site, rows, cols) >= thr


def attention_keep(state, site: int, B: int, H: int, Sq: int, Sk: int, p: float, device=None):
    """Keep mask [B, H, Sq, Sk] of attention probabilities: row = (b H + h) Sq + q, col = key."""
    t = getattr(state, "tensor", state)
    dev = t.device if isinstance(t, torch.Tensor) else device
    rows = torch.arange(B * H * Sq, dtype=torch.int64, device=dev)
    return dropout_keep(state, site, rows, torch.arange(Sk, dtype=torch.int64, device=dev), p).view(B, H, Sq, Sk)


def dropout(x, keep, scale: float):
    """y = keep ? x * scale : 0, rounded once to x's dtype (forward and backward are the same map)."""
    return torch.where(keep.reshape(x.shape), x.float() * scale, torch.zeros((), device=x.device)).to(x.dtype)


def dropout_add_norm_fwd(x, res, gamma, beta, eps, keep, scale: float):
    """LayerNorm(keep * scale * x + res): (y, mean, rstd, xsum) like ``norm_fwd`` with a residual."""
    xs = torch.where(keep.reshape(x.shape), x.float() * scale, torch.zeros((), device=x.device)) + res.float()
    mean = xs.mean(-1)
    var = (xs - mean.unsqueeze(-1)).pow(2).mean(-1)
    rstd = torch.rsqrt(var + eps)
    y = (xs - mean.unsqueeze(-1)) * rstd.unsqueeze(-1) * gamma.float() + beta.float()
    return y.to(x.dtype), mean.reshape(-1), rstd.reshape(-1), xs.to(x.dtype)


def dropout_add_norm_bwd(dy, xsum, gamma, mean, rstd, dres, keep, scale: float):
    """(dx, da, dgamma, dbeta, dsum): dx the gradient of the sum (the residual's), da = keep * scale * dx the dropped
    summand's, dsum the fp32 column sums of da."""
    D = xsum.shape[-1]
    g = dy.float().reshape(-1, D)
    r = rstd.reshape(-1, 1)
    xh = (xsum.float().reshape(-1, D) - mean.reshape(-1, 1)) * r
    gg = g * gamma.float()
    dx = r * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres.float().reshape(-1, D)
    da = torch.where(keep.reshape(-1, D), dx * scale, torch.zeros((), device=dx.device))
    return (dx.reshape(xsum.shape).to(xsum.dtype), da.reshape(xsum.shape).to(xsum.dtype), (g * xh).sum(0), g.sum(0),
            da.sum(0))


# --------------------------------------------------------------------------- cross entropy
def xent_fwd(logits, labels, ignore_index=-100, smoothing=0.0):
    lf = logits.float()
    lse = torch.logsumexp(lf, -1)
    valid = labels != ignore_index
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    picked = lf.gather(-1, safe.unsqueeze(-1)).squeeze(-1)
    loss = lse - picked
    if smoothing > 0:
        loss = (1 - smoothing) * loss + smoothing * (lse - lf.mean(-1))
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    return loss, lse


def xent_bwd(logits, labels, lse, dscale, ignore_index=-100, smoothing=0.0):
    lf = logits.float()
    V = lf.shape[-1]
    p = torch.exp(lf - lse.unsqueeze(-1)) - smoothing / V
    valid = labels != ignore_index
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    p.scatter_add_(-1, safe.unsqueeze(-1), torch.full_like(p[:, :1], -(1 - smoothing)))
    sc = dscale.float().reshape(-1)
    sc = sc.expand(lf.shape[0]) if sc.numel() == 1 else sc
    sc = torch.where(valid, sc, torch.zeros_like(sc))
    return (p * sc.unsqueeze(-1)).to(logits.dtype)


def xent_eval(logits, labels, ignore_index=-100):
    """(loss[R] fp32, rank[R] int32): per-row cross-entropy and the label's rank among the columns,
    rank = #{j : l[j] > l[y]} + #{j < y : l[j] == l[y]} (ties to the lower index). Ignored rows: loss 0, rank V."""
    lf = logits.float()
    V = lf.shape[-1]
    valid = labels != ignore_index
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    picked = lf.gather(-1, safe.unsqueeze(-1))
    loss = torch.logsumexp(lf, -1) - picked.squeeze(-1)
    before = torch.arange(V, device=lf.device).unsqueeze(0) < safe.unsqueeze(-1)
    rank = ((lf > picked) | ((lf == picked) & before)).sum(-1)
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    rank = torch.where(valid, rank, torch.full_like(rank, V))
    return loss, rank.to(torch.int32)


# --------------------------------------------------------------------------- inference convolution
def conv_bn_act_infer(x, w, scale, shift, stride, padding, residual=None, relu=True):
    """act(conv(x, w) * scale + shift + residual) on NHWC ``x`` / KRSC ``w`` with a folded BatchNorm (fp32 [K] scale
    / shift), in fp32, rounded once to ``x``'s dtype."""
    y = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), None, stride,
                                   padding).permute(0, 2, 3, 1)
    y = y * scale.float() + shift.float()
    if residual is not None:
        y = y + residual.float()
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype).contiguous()


# --------------------------------------------------------------------------- optimizers
def _decay_vec(mask, n, wd, device):
    if mask is None:
        return torch.full((n,), wd, device=device)
    return mask.to(device).repeat_interleave(64)[:n].float() * wd


def _skipped(scale_t) -> bool:
    """A zero clip factor marks non-finite gradients: the step is skipped, all buffers untouched."""
    return scale_t is not None and float(scale_t.reshape(-1)[0]) == 0.0


def sgd(p, mom, g, pbf, mask, lr, mu, wd, scale, scale_t, nesterov, first_step):
    if _skipped(scale_t):
        return
    s = scale * (float(scale_t.reshape(-1)[0]) if scale_t is not None else 1.0)
    d = g.float() * s + _decay_vec(mask, p.numel(), wd, p.device) * p
    m = d.clone() if first_step else mom * mu + d
    mom.copy_(m)
    p.sub_(lr * (d + mu * m if nesterov else m))
    if pbf is not None:
        pbf.copy_(p)


def adam(p, m1, m2, g, pbf, mask, lr, b1, b2, eps, wd, scale, scale_t, step, decoupled):
    if _skipped(scale_t):
        return
    s = scale * (float(scale_t.reshape(-1)[0]) if scale_t is not None else 1.0)
    w = _decay_vec(mask, p.numel(), wd, p.device)
    gr = g.float() * s
    if not decoupled:
        gr = gr + w * p
    m1.mul_(b1).add_((1 - b1) * gr)
    m2.mul_(b2).add_((1 - b2) * gr * gr)
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    upd = (lr / bc1) * m1 / (m2.sqrt() / math.sqrt(bc2) + eps)
    if decoupled:
        p.sub_(lr * w * p)
    p.sub_(upd)
    if pbf is not None:
        pbf.copy_(p)


def grad_sumsq(g):
    gf = g.float()
    return torch.stack([(gf * gf).sum(), (~torch.isfinite(gf)).sum().float()])


# --------------------------------------------------------------------------- gradient accumulation
def _accum_range(a, b, lo, hi):
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError("gradient accumulation works on fp32 buffers")
    if a.numel() != b.numel() or lo % 64 or hi % 64 or not 0 <= lo <= hi <= a.numel():
        raise ValueError("range [%d, %d) must be 64-aligned and inside two buffers of one size" % (lo, hi))


def grad_accumulate(acc, g, lo, hi, first):
    """acc[lo:hi] = g[lo:hi] if first else acc[lo:hi] + g[lo:hi] (whatever acc held is overwritten when first)."""
    _accum_range(acc, g, lo, hi)
    if first:
        acc[lo:hi].copy_(g[lo:hi])
    else:
        torch.add(acc[lo:hi], g[lo:hi], out=acc[lo:hi])


def grad_fold(g, acc, lo, hi, out_bf=None):
    """g[lo:hi] = g[lo:hi] + acc[lo:hi]; with out_bf also out_bf[:hi - lo] = bf16(g[lo:hi]), round to nearest even."""
    _accum_range(g, acc, lo, hi)
    if out_bf is not None and (out_bf.dtype != torch.bfloat16 or out_bf.numel() < hi - lo):
        raise ValueError("out_bf must be bf16 with at least hi - lo elements")
    torch.add(g[lo:hi], acc[lo:hi], out=g[lo:hi])
    if out_bf is not None:
        out_bf[:hi - lo].copy_(g[lo:hi])


# --------------------------------------------------------------------------- layer-wise optimizers (LARS / LAMB)
# These work on one PIECE of one parameter slot at a time (a slot, or the part of it inside one owned range of a
# sharded update); ``ops/optim.py`` walks the pieces. ``s`` is grad_scale times the clip factor, ``w`` the slot's
# weight decay (0 where it does not decay).
def lamb_moments(m1, m2, g, s, b1, b2):
    gr = g.float() * s
    m1.mul_(b1).add_((1 - b1) * gr)
    m2.mul_(b2).add_((1 - b2) * gr * gr)


def lamb_u(p, m1, m2, b1, b2, eps, w, step):
    """LAMB's direction from the advanced moments: the Adam step plus decay."""
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    return (m1 / bc1) / ((m2 / bc2).sqrt() + eps) + w * p


def layer_sums(p, x):
    """(sum p^2, sum x^2) of one piece, fp32 [2]; the per-slot sums are these added over the slot's pieces."""
    return torch.stack([(p * p).sum(), (x * x).sum()])


def trust_ratio(sums, decay, lamb, eta=0.001, wd=0.0):
    """Per-slot trust ratio from sums [n][2] and the decay flags [n]: LAMB ||p|| / ||u||, LARS eta ||p|| / (||g|| +
    wd ||p||); 1 where the slot does not decay or either norm is zero."""
    pn, xn = sums[:, 0].sqrt(), sums[:, 1].sqrt()
    ok = decay.bool() & (pn > 0) & (xn > 0)
    den = xn if lamb else xn + wd * pn
    r = pn / torch.where(ok, den, torch.ones_like(den))
    if not lamb:
        r = r * eta
    return torch.where(ok, r, torch.ones_like(r))


def lars(p, mom, g, pbf, r, lr, mu, w, s, first_step):
    d = r * (g.float() * s + w * p)
    m = d.clone() if first_step else mom * mu + d
    mom.copy_(m)
    p.sub_(lr * m)
    if pbf is not None:
        pbf.copy_(p)


def lamb(p, m1, m2, pbf, r, lr, b1, b2, eps, w, step):
    """Second half of a LAMB step (``lamb_moments`` has run): p -= lr r u."""
    p.sub_(lr * r * lamb_u(p, m1, m2, b1, b2, eps, w, step))
    if pbf is not None:
        pbf.copy_(p)


# --------------------------------------------------------------------------- dataset augmentation (ops/data.py)
def s2d_input(x8, pad: int = 3):
    """[N, H, W, >= 4] -> [N, (H+2 pad)/2, (W+2 pad)/2, 16]: ``stem_s2d_input`` (channels 0..3 of every 2x2 block)."""
    N, H, W = x8.shape[:3]
    p = torch.nn.functional.pad(x8[..., :4], (0, 0, pad, pad, pad, pad))
    Hs, Ws = (H + 2 * pad) // 2, (W + 2 * pad) // 2
    return p.reshape(N, Hs, 2, Ws, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(N, Hs, Ws, 16).contiguous()


def augment(src, table, a, b, S: int, layout: str = "nhwc8"):
    """The definition of ``ops.data.augment`` in float64, rounded once to fp32 and once to bf16 (the CPU path and the
    GPU kernel's oracle). ``src`` uint8 [M, Hs, Ws, 3]; ``table`` int32 [N, 6] rows (index, y0, x0, h, w, flip);
    ``a``, ``b``: the fp32 values 1 / std_c and -mean_c / std_c. Output element (n, i, j, c), jj = S-1-j when flipped:
    a row with h == w == S copies source pixel (y0+i, x0+jj), ``u8 * a_c + b_c`` (exact in float64, so the fp32
    rounding is fmaf's), 0 outside the source; any other row resizes its box bilinearly to S x S (half-pixel centres,
    indices clamped to the box) first. ``layout``: "nhwc8" [N, S, S, 8] or "s2d" [N, S/2+3, S/2+3, 16]; bf16."""
    src = torch.as_tensor(src)
    table = torch.as_tensor(table).cpu()
    M, Hs, Ws = src.shape[:3]
    N = table.shape[0]
    a64 = torch.tensor([float(v) for v in a], dtype=torch.float32).double()
    b64 = torch.tensor([float(v) for v in b], dtype=torch.float32).double()
    out = torch.zeros(N, S, S, 8, dtype=torch.float64)
    for n, (idx, y0, x0, h, w, flip) in enumerate(table.tolist()):
        if not (0 <= idx < M and h >= 1 and w >= 1 and flip in (0, 1)):
            raise ValueError("table row %d: bad index, box or flip" % n)
        if h == S and w == S:
            ys, ye, xs, xe = max(y0, 0), min(y0 + S, Hs), max(x0, 0), min(x0 + S, Ws)
            img = torch.zeros(S, S, 3, dtype=torch.float64)
            if ye > ys and xe > xs:
                img[ys - y0:ye - y0, xs - x0:xe - x0] = src[idx, ys:ye, xs:xe].double() * a64 + b64
        else:
            if y0 < 0 or x0 < 0 or y0 + h > Hs or x0 + w > Ws:
                raise ValueError("table row %d: resized box leaves the source" % n)
            box = src[idx, y0:y0 + h, x0:x0 + w].double()
            fy = ((torch.arange(S, dtype=torch.float64) + 0.5) * (h / S) - 0.5).clamp_(min=0)
            fx = ((torch.arange(S, dtype=torch.float64) + 0.5) * (w / S) - 0.5).clamp_(min=0)
            iy0 = fy.floor().long().clamp_(max=h - 1)
            ix0 = fx.floor().long().clamp_(max=w - 1)
            iy1, ix1 = (iy0 + 1).clamp_(max=h - 1), (ix0 + 1).clamp_(max=w - 1)
            ly, lx = (fy - iy0).view(S, 1, 1), (fx - ix0).view(1, S, 1)
            top = (1 - lx) * box[iy0][:, ix0] + lx * box[iy0][:, ix1]
            bot = (1 - lx) * box[iy1][:, ix0] + lx * box[iy1][:, ix1]
            img = ((1 - ly) * top + ly * bot) * a64 + b64
        out[n, :, :, :3] = img.flip(1) if flip else img
    out = out.float().to(torch.bfloat16)
    if layout == "nhwc8":
        return out
    if layout != "s2d" or S % 2:
        raise ValueError("layout must be 'nhwc8' or 's2d' (even S), got %r with S = %d" % (layout, S))
    return s2d_input(out, 3)


# --------------------------------------------------------------------------- token batches (ops/data.py)
#   tok / type: [CLS] A [SEP] B [SEP] pad; keys = philox rowkey(seed, step 0, site 3 * stream + {0, 1, 2}, row ord)
#   score[j] = mix32(ksel ^ (j * G)); the n candidates with the smallest (score, j) are selected
#   id[j] = u < 0.8 2^32 ? mask : u < 0.9 2^32 ? (mix32(krep ^ j G) * vocab) >> 32 : tok[j], u = mix32(kdec ^ j G)
TOKEN_G = 0x9E3779B1
MLM_MASK_THR = 3435973837   # floor(0.8 * 2^32 + 0.5)
MLM_RANDOM_THR = 3865470566  # floor(0.9 * 2^32 + 0.5)
MLM_MAX_SEQ = 512


def _mix32(x):
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def _token_values(src, idx):
    """int64 tokens ``src[idx]``: ``src`` int32 / int64, or uint16 data (numpy uint16 or an int16 view, read
    unsigned)."""
    v = src[idx].to(torch.int64)
    return v & 0xFFFF if src.dtype == torch.int16 else v


def mlm_keys(seed: int, stream: int, ords):
    """(ksel, kdec, krep): int64 tensors of 32-bit values, ``ords``' shape."""
    return tuple(dropout_rowkey((seed, 0), 3 * int(stream) + i, ords) for i in range(3))


def mlm_scores(seed: int, stream: int, ords, S: int):
    """Selection scores [len(ords), S] (32-bit values in int64) of the positions 0 .. S - 1."""
    ords = torch.as_tensor(ords, dtype=torch.int64)
    jg = _mul32(torch.arange(S, dtype=torch.int64, device=ords.device), TOKEN_G)
    return _mix32(mlm_keys(seed, stream, ords)[0].unsqueeze(1) ^ jg)


def check_mlm_table(table, T: int, S: int, P: int, vocab: int, special, u16: bool = False) -> None:
    """The checks of the GPU binding, on the host; raises ValueError on the first bad row."""
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 6 or table.shape[0] < 1:
        raise ValueError("table must be int64 [N, 6]")
    if not 1 <= S <= MLM_MAX_SEQ or not 1 <= P <= S:
        raise ValueError("S must be in [1, %d] and P in [1, S], got S = %d, P = %d" % (MLM_MAX_SEQ, S, P))
    if not 2 <= vocab <= 2 ** 31 - 1 or (u16 and vocab > 65536):
        raise ValueError("vocab must be in [2, 2^31 - 1] (uint16 tokens: <= 65536), got %d" % vocab)
    if len(special) != 4 or any(not 0 <= int(v) < vocab for v in special):
        raise ValueError("special must be four ids (pad, cls, sep, mask) below vocab")
    a0, la, b0, lb, n, ord_ = table.unbind(1)
    bad = ((la < 1) | (lb < 1) | (la > S) | (lb > S) | (la + lb + 3 > S) | (a0 < 0) | (a0 > T - la) | (b0 < 0)
           | (b0 > T - lb) | (n < 1) | (n > P) | (n > la + lb) | (ord_ < 0))
    if bool(bad.any()):
        r = int(bad.nonzero()[0])
        raise ValueError("table row %d: %s is not a valid (a0, la, b0, lb, n, ord) for T = %d, S = %d, P = %d"
                         % (r, tuple(table[r].tolist()), T, S, P))


def mlm_batch(src, table, S: int, P: int, vocab: int, special, seed: int, stream: int = 0):
    """The definition of ``ops.data.mlm_batch`` in torch integer ops (the CPU path and the GPU kernel's oracle; it
    runs on ``src``'s device). ``src``: the 1-D token array; ``table`` int64 [N, 6] rows (a0, la, b0, lb, n, ord);
    ``special`` = (pad, cls, sep, mask). Returns (ids [N, S], token_types [N, S], labels [N, P], positions [N, P]),
    int64."""
    src = torch.as_tensor(src)
    table = torch.as_tensor(table)
    S, P, vocab = int(S), int(P), int(vocab)
    T = int(src.shape[0])
    check_mlm_table(table.cpu(), T, S, P, vocab, special, u16=src.dtype == torch.int16)
    dev = src.device
    pad, cls, sep, mask = (int(v) for v in special)
    a0, la, b0, lb, n, ord_ = (c.unsqueeze(1) for c in table.to(dev).unbind(1))
    N = table.shape[0]
    j = torch.arange(S, dtype=torch.int64, device=dev).unsqueeze(0)
    L = la + lb + 3
    in_a, in_b = (j >= 1) & (j <= la), (j >= la + 2) & (j <= la + lb + 1)
    cand = in_a | in_b
    idx = torch.where(in_a, a0 + j - 1, torch.where(in_b, b0 + j - la - 2, torch.zeros_like(j))).clamp_(0, T - 1)
    tok = torch.where(cand, _token_values(src, idx), torch.full_like(idx, pad))
    tok = torch.where(j == 0, torch.full_like(tok, cls), tok)
    tok = torch.where((j == la + 1) | (j == L - 1), torch.full_like(tok, sep), tok)
    types = ((j >= la + 2) & (j <= L - 1)).to(torch.int64)
    ksel, kdec, krep = mlm_keys(seed, stream, ord_)
    jg = _mul32(j, TOKEN_G)
    # rank among the candidates by (score, j): the key is unique per position, so one sort gives it
    key = torch.where(cand, _mix32(ksel ^ jg) * 1024 + j, torch.full_like(idx, 1 << 62))
    rank = torch.empty_like(key)
    rank.scatter_(1, key.argsort(dim=1), j.expand(N, S).contiguous())
    sel = cand & (rank < n)
    slot = sel.to(torch.int64).cumsum(1) - 1
    labels = torch.full((N, P), -100, dtype=torch.int64, device=dev)
    positions = torch.zeros((N, P), dtype=torch.int64, device=dev)
    rows = torch.arange(N, device=dev).unsqueeze(1).expand(N, S)[sel]
    labels[rows, slot[sel]] = tok[sel]
    positions[rows, slot[sel]] = j.expand(N, S)[sel]
    u = _mix32(kdec ^ jg)
    rep = (_mix32(krep ^ jg) * vocab) >> 32
    masked = torch.where(u < MLM_MASK_THR, torch.full_like(tok, mask), torch.where(u < MLM_RANDOM_THR, rep, tok))
    return torch.where(sel, masked, tok), types, labels, positions


def check_unpad_stream(table, cu, T: int) -> None:
    """``cu`` and ``T`` of ``mlm_batch_unpadded`` against a checked table, as the GPU binding does; raises ValueError
    on the first failed check."""
    N = table.shape[0]
    if not isinstance(cu, torch.Tensor) or cu.dtype != torch.int64 or cu.dim() != 1 or cu.shape[0] != N + 1:
        raise ValueError("cu must be int64 [N + 1] with N = %d table rows" % N)
    if int(cu[0]) != 0:
        raise ValueError("cu[0] must be 0, got %d" % int(cu[0]))
    bad = (cu[1:] - cu[:-1]) != table[:, 1] + table[:, 3] + 3
    if bool(bad.any()):
        raise ValueError("cu row %d: the difference is not la + lb + 3" % int(bad.nonzero()[0]))
    T, end = int(T), int(cu[-1])
    if T < end:
        raise ValueError("T = %d is below cu[N] = %d" % (T, end))
    if T % 128:
        raise ValueError("T = %d must be a multiple of 128" % T)
    if T - end >= 128:
        raise ValueError("T = %d must be cu[N] = %d rounded up to a multiple of 128" % (T, end))


def unpad_stream_rows(total: int) -> int:
    """``T`` of ``mlm_batch_unpadded``: ``total = cu[N]`` rounded up to a multiple of 128."""
    return (int(total) + 127) // 128 * 128


def mlm_batch_unpadded(src, table, cu, T: int, S: int, P: int, vocab: int, special, seed: int, stream: int = 0):
    """The definition of ``ops.data.mlm_batch_unpadded``: ``mlm_batch`` gathered at the real positions, plus the tail.
    ``cu`` int64 [N + 1] (host): cu[0] = 0, cu[n + 1] - cu[n] = L_n = la + lb + 3; ``T``: cu[N] rounded up to a
    multiple of 128. Stream row cu[n] + j (j < L_n) holds what ``mlm_batch`` writes at [n, j], with pos = j and the
    span bounds lo = cu[n], hi = cu[n + 1]; the tail [cu[N], T) is one pad span (pad, type 0, pos 0, lo = cu[N],
    hi = T). Returns (ids, token_types, pos) int64 [T], (labels, rows) int64 [N, P] with rows = cu[n] + position
    (unused slots: cu[n]), cls_rows = cu[:N] int64 [N] and (lo, hi) int32 [1, T]."""
    src = torch.as_tensor(src)
    table, cu = torch.as_tensor(table), torch.as_tensor(cu)
    ids2, types2, labels, positions = mlm_batch(src, table, S, P, vocab, special, seed, stream)
    check_unpad_stream(table.cpu(), cu.cpu() if isinstance(cu, torch.Tensor) else cu, T)
    dev, T, N = src.device, int(T), table.shape[0]
    cu = cu.to(dev)
    total = int(cu[-1])
    n = torch.repeat_interleave(torch.arange(N, device=dev), cu[1:] - cu[:-1])
    j = torch.arange(total, dtype=torch.int64, device=dev) - cu[n]
    ids = torch.full((T,), int(special[0]), dtype=torch.int64, device=dev)
    types = torch.zeros(T, dtype=torch.int64, device=dev)
    pos = torch.zeros(T, dtype=torch.int64, device=dev)
    lo = torch.full((T,), total, dtype=torch.int64, device=dev)
    hi = torch.full((T,), T, dtype=torch.int64, device=dev)
    ids[:total], types[:total], pos[:total] = ids2[n, j], types2[n, j], j
    lo[:total], hi[:total] = cu[n], cu[n + 1]
    return (ids, types, pos, labels, cu[:N, None] + positions, cu[:N].clone(), lo.to(torch.int32).unsqueeze(0),
            hi.to(torch.int32).unsqueeze(0))


def causal_batch(src, starts, S: int):
    """The definition of ``ops.data.causal_batch``: ids = src[start + j], labels = src[start + j + 1], int64 [N, S]."""
    src = torch.as_tensor(src)
    starts = torch.as_tensor(starts)
    S, T = int(S), int(src.shape[0])
    if starts.dtype != torch.int64 or starts.dim() != 1 or starts.shape[0] < 1 or S < 1:
        raise ValueError("starts must be int64 [N] and S positive")
    if bool(((starts < 0) | (starts > T - S - 1)).any()):
        raise ValueError("a window [start, start + %d + 1) leaves the %d tokens of src" % (S, T))
    at = starts.to(src.device).unsqueeze(1) + torch.arange(S, dtype=torch.int64, device=src.device)
    return _token_values(src, at), _token_values(src, at + 1)


def check_doc_tok(doc_tok) -> None:
    """The documents' token offsets: int64 [D + 1], strictly ascending from 0."""
    doc_tok = torch.as_tensor(doc_tok)
    if doc_tok.dtype != torch.int64 or doc_tok.dim() != 1 or doc_tok.shape[0] < 2 or int(doc_tok[0]) != 0 or \
            not bool((doc_tok[1:] > doc_tok[:-1]).all()):
        raise ValueError("doc_tok must be int64 [D + 1] and ascend strictly from 0")


def causal_doc_batch(src, starts, abs_starts, doc_tok, S: int):
    """The definition of ``ops.data.causal_doc_batch``: ``causal_batch`` with document boundaries. ``starts`` index
    ``src``, ``abs_starts`` are the same windows' positions in the split and ``doc_tok`` int64 [D + 1] the documents'
    token offsets. For element (n, j) at p = abs_starts[n] + j with d the last document starting at or before p:
    lo = max(doc_tok[d] - abs_starts[n], 0), hi = min(doc_tok[d + 1] - abs_starts[n], S), pos = j - lo (int32 [N, S]),
    ids = src[start + j] and labels = src[start + j + 1], or -100 where p is its document's last token."""
    src = torch.as_tensor(src)
    starts, abs_starts, doc_tok = torch.as_tensor(starts), torch.as_tensor(abs_starts), torch.as_tensor(doc_tok)
    ids, labels = causal_batch(src, starts, S)
    S = int(S)
    check_doc_tok(doc_tok.cpu())
    if abs_starts.dtype != torch.int64 or abs_starts.shape != starts.shape:
        raise ValueError("abs_starts must be int64 [N] like starts")
    if bool(((abs_starts < 0) | (abs_starts > int(doc_tok[-1]) - S - 1)).any()):
        raise ValueError("a window [start, start + %d + 1) leaves the %d tokens of the split" % (S, int(doc_tok[-1])))
    dev = src.device
    doc_tok, ab = doc_tok.to(dev), abs_starts.to(dev).unsqueeze(1)
    j = torch.arange(S, dtype=torch.int64, device=dev)
    p = ab + j
    d = (torch.searchsorted(doc_tok, p.contiguous(), right=True) - 1).clamp(0, doc_tok.shape[0] - 2)
    end = doc_tok[d + 1]
    lo = (doc_tok[d] - ab).clamp(min=0)
    hi = (end - ab).clamp(max=S)
    labels = torch.where(p + 1 < end, labels, torch.full_like(labels, -100))
    return ids, labels, lo.to(torch.int32), hi.to(torch.int32), (j - lo).to(torch.int32)


# --------------------------------------------------------------------------- generation (ops/decode.py)
def linear_skinny(x, w):
    """y = x . w^T accumulated in fp32, one rounding to x's dtype."""
    return torch.matmul(x.float(), w.float().t()).to(x.dtype)


def check_cache_table(table, B: int, lo: int, hi: int, what: str) -> None:
    """A host mirror (int [B]) with every entry in [lo, hi], as the bindings check it before a launch."""
    t = torch.as_tensor(table).reshape(-1)
    if t.numel() != B:
        raise RuntimeError("%s must have B = %d entries, has %d" % (what, B, t.numel()))
    bad = ((t < lo) | (t > hi)).nonzero()
    if bad.numel():
        b = int(bad[0])
        raise RuntimeError("%s row %d: %d outside [%d, %d]" % (what, b, int(t[b]), lo, hi))


def kv_append(qkv, cache_k, cache_v, start, S: int, Hq: int) -> None:
    """Token s of row b of the packed, rotated projection output ``qkv`` [B * S, (Hq + 2 Hkv) * D] goes to position
    ``start[b] + s`` of the caches [B, Hkv, Smax, D]: an index copy."""
    B, Hkv, Smax, D = cache_k.shape
    start = torch.as_tensor(start).to(qkv.device).long()
    check_cache_table(start.cpu(), B, 0, Smax - S, "start")
    g = qkv.reshape(B, S, Hq + 2 * Hkv, D)
    pos = start[:, None] + torch.arange(S, device=qkv.device)[None]  # [B, S]
    b = torch.arange(B, device=qkv.device)[:, None].expand(B, S)
    for h in range(Hkv):
        cache_k[b, h, pos] = g[:, :, Hq + h].to(cache_k.dtype)
        cache_v[b, h, pos] = g[:, :, Hq + Hkv + h].to(cache_v.dtype)


def decode_attention(q, cache_k, cache_v, lens, scale: float):
    """One query token per row: q [B, Hq, D] against the keys 0 .. lens[b] - 1 of the caches [B, Hkv, Smax, D]; returns
    [B, Hq * D]. Cache positions at or past lens[b] are never read (they may hold anything, NaN included): they are
    replaced by zeros before the products, not merely masked in the scores."""
    B, Hq, D = q.shape
    Hkv, Smax = cache_k.shape[1], cache_k.shape[2]
    lens = torch.as_tensor(lens).to(q.device).long().clamp(1, Smax)
    live = torch.arange(Smax, device=q.device)[None, :] < lens[:, None]  # [B, Smax]
    zero = torch.zeros((), device=q.device)
    k = torch.where(live[:, None, :, None], cache_k.float(), zero)
    v = torch.where(live[:, None, :, None], cache_v.float(), zero)
    s = torch.einsum("bhgd,bhsd->bhgs", q.float().reshape(B, Hkv, Hq // Hkv, D), k) * scale
    p = torch.softmax(s.masked_fill(~live[:, None, None, :], float("-inf")), -1)
    return torch.einsum("bhgs,bhsd->bhgd", p, v).reshape(B, Hq * D).to(q.dtype)
