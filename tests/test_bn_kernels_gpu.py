"""batchnorm.hip, every form, per element against the fp64 oracles of tests/bn_oracles.py.

Every bound is derived in bn_oracles (next to the function that forms it), is a reference-against-reference
measurement (measured_delta inside B.y_delta; the sizes seen are noted at its use below), or is exact equality. None was fitted to
a kernel; test_bn_oracles_cpu.py shows that plain fp32 evaluations stay inside each of them and that they catch a
dropped row, a dropped channel group, a count off by one, a biased run_var, a D without its B mean term, a shifted mask
bit and a swapped second input. Outputs that the caller allocates start as NaN; before a call whose outputs the
binding allocates the caching allocator's free blocks are filled with NaN, so an element no kernel writes fails.
The mask and the pool's winner index are taken from the kernel and checked for exactness on their own, so no element is
excluded from any comparison.

The geometry notes are what bn_geom gives on a 256-CU part; no assertion depends on the CU count.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_oracles as B  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
EPS, MOM = B.EPS, B.MOMENTUM


def _C():
    from k8s_amd.ops._ext import load

    return load()


def _nan(C, dev):
    return torch.full((C,), NAN, device=dev)


def _dirty(x):
    """Fill what the allocator will hand the binding next with NaN: three tensors of x's size (y / dx / dres / dx2),
    the per-channel vectors and tables, the mask bytes (0xAA: neither all set nor all clear)."""
    C, dev = x.shape[-1], x.device
    keep = [torch.full(x.shape, NAN, device=dev, dtype=BF16) for _ in range(3)]
    keep += [torch.full((n * C,), NAN, device=dev) for n in (1, 1, 1, 1, 2, 2, 4, 4)]
    keep += [torch.full((max(x.numel() // 8, 1),), 0xAA, device=dev, dtype=torch.uint8) for _ in range(2)]
    del keep


def _run_stats(C, dev, seed=11):
    torch.manual_seed(seed)
    return torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5


# =============================================================================================== forward
def _forward(d, relu, res, want_mask, nrep=None, sub2=False, edge=None):
    """bn_fwd (nrep None: its own reduction) or bn_fwd_from_sums, every output checked: y, mask, mean, invstd."""
    C_ = _C()
    x, g, b = d["x"], d["gamma"], d["beta"]
    C = x.shape[-1]
    M = x.numel() // C
    r = d["res"] if res else None
    rm0, rv0 = _run_stats(C, x.device)
    rm, rv = rm0.clone(), rv0.clone()
    _dirty(x)
    if nrep is None:
        out = C_.bn_fwd(x, r, g, b, rm, rv, True, MOM, EPS, relu, want_mask)
        st = B.bn_stats(x, EPS)
        B.check_stats_own(out[1], out[2], st)
    else:
        sums = B.sums_from(x, nrep)
        out = C_.bn_fwd_from_sums(x, r, g, b, sums, rm, rv, MOM, EPS, relu, want_mask, sub2)
        st = B.bn_stats_from_sums(sums, M, EPS)
        B.check_stats_sums(out[1], out[2], st, EPS)
    y, mean, invstd = out[:3]
    mask = out[3] if want_mask else None
    if edge == "const":  # var = 0: the clamp leaves eps^-1/2, not NaN; the checks above held it to that
        assert abs(float(st["invstd"][B.edge_channel(C)]) - EPS ** -0.5) < 1e-9
    B.check_running(rm, rv, rm0, rv0, st, nrep is None, MOM, EPS)
    # measured (fp32 oracle against fp64, |y| up to 9): 2.6e-7 .. 7.1e-7 at every edge (x16: up to 1.1e-5); the affine
    # form's 4 u y_abs adds up to 2e-6, 2.9e-5 at 'offset' and 1.4e-4 in the constant channel (invstd = 316); a bf16
    # half ulp at |y| = 1 is 3.9e-3
    o64 = B.bn_apply(x, mean, invstd, g, b, r, relu)
    B.check_fwd(y, mask, o64, B.bn_apply(x, mean, invstd, g, b, r, relu, dtype=F32))
    if sub2:
        assert torch.equal(out[-1], y[:, ::2, ::2, :]), "ysub is not y[:, ::2, ::2, :]"
    return y, mask, mean, invstd


# =============================================================================================== backward
def _backward(d, y, mask, mean, invstd, relu, res, nreps=(1,)):
    """Every bn_bwd form the forward allows against one oracle; bn_bwd_params + bn_bwd_apply give bn_bwd's bits."""
    C_ = _C()
    x, dy, g, b = d["x"], d["dy"], d["gamma"], d["beta"]
    C, dev = x.shape[-1], x.device
    bits = (y > 0) if relu else None
    o64 = B.bn_bwd(dy, x, bits, mean, invstd, g, b)
    bounds = B.bn_bwd_bounds(o64)

    def run(y_arg, relu_x, mask_arg, want_dres, sums=None):
        dg, db = _nan(C, dev), _nan(C, dev)
        _dirty(x)
        dx, dres = C_.bn_bwd(dy, x, y_arg, mean, invstd, g, b, relu_x, dg, db, want_dres, mask_arg, sums)
        what = "bn_bwd(y=%s relu_x=%s mask=%s dres=%s sums=%s) " % (
            y_arg is not None, relu_x, mask_arg is not None, want_dres, None if sums is None else sums.shape[0])
        B.check_bwd(dx, dres if want_dres else None, dg, db, o64, what, bounds)
        return dx

    def halves(mask_arg, dx_whole, sums=None):
        dg, db = _nan(C, dev), _nan(C, dev)
        _dirty(x)
        params = C_.bn_bwd_params(dy, x, mask_arg, sums, mean, invstd, g, b, dg, db)
        B.check_table(params, o64, bounds, "bn_bwd_params ")
        B.check_bwd(None, None, dg, db, o64, "bn_bwd_params ", bounds)
        _dirty(x)
        assert torch.equal(C_.bn_bwd_apply(dy, x, mask_arg, params), dx_whole), "params + apply is not bn_bwd"

    if not relu:
        run(None, False, None, False)
        run(None, False, None, True)
        return
    run(y, False, None, False)
    run(y, False, None, True)
    if mask is not None:
        dxm = run(None, False, mask, res)
        run(None, False, mask, not res)
        halves(mask, dxm)
        for n in nreps:
            s = B.bwd_sums_from(o64["g"], x, mean, n)
            dxs = run(None, False, mask, res, s)
            halves(mask, dxs, s)
    if not res:  # the ReLU decision can be recomputed from x
        dxr = run(None, True, None, False)
        halves(None, dxr)
        for n in nreps:
            s = B.bwd_sums_from(o64["g"], x, mean, n)
            dxs = run(None, True, None, False, s)
            halves(None, dxs, s)


# (M, C), each the smallest that reaches its edge (bn_geom on 256 CUs: tpr = threads per row, rpi = rows per
# iteration = 256 / tpr; flat = blocks of the per-element passes, ceil(M C / 8 / 256)):
#   (1, 8)      one row, one vector: the count > 1 guard, seven empty bands, flat 1
#   (7, 8)      fewer rows than the 8 bands (bandlen 1, band 7 empty)
#   (9, 24)     tpr 3, rpi 85, thread 255 idle; bandlen 2, band 4 holds one row, bands 5..7 clamp M_ < 0 to 0
#   (63, 64)    M / 64 == 0
#   (64, 72)    tpr 9 (odd, no halving), rpi 28, four idle threads
#   (98, 80)    tpr 10 halves to 5, two channel slices
#   (333, 24)   idle threads with four trips and a remainder
#   (333, 72)
#   (1000, 256) tpr 32 halves to 8, four channel slices
#   (4099, 8)   prime M: ragged last statistics block, tpr 1 / rpi 256, flat 17
#   (4099, 64)  tpr 8
#   (98, 2048)  tpr 256 halves to 8: 32 channel slices
#   (7, 2048)   flat 7: the band order with q = 0, r = 7
#   (9, 2048)   flat 9: q = 1, r = 1
#   (64, 256)   flat 8: r = 0
#   (64, 2056)  257 channel groups: a second channel slice that holds one group
SHAPES = B.SHAPES
FORMS = [(True, False, False), (True, False, True), (True, True, True), (False, False, False), (False, True, False)]


@pytest.mark.parametrize("relu,res,want_mask", FORMS)
@pytest.mark.parametrize("M,C", SHAPES)
def test_bn_own_reduce(cuda, M, C, relu, res, want_mask):
    d = B.bn_inputs((M, C), cuda, res=res)
    y, mask, mean, invstd = _forward(d, relu, res, want_mask)
    _backward(d, y, mask, mean, invstd, relu, res)


@pytest.mark.parametrize("nrep", [1, 32])
@pytest.mark.parametrize("relu,res,want_mask", [(True, False, True), (True, True, True), (False, False, False)])
@pytest.mark.parametrize("M,C", [(1, 8), (7, 8), (9, 24), (63, 64), (333, 72), (4099, 8), (98, 2048), (64, 2056)])
def test_bn_from_sums(cuda, M, C, relu, res, want_mask, nrep):
    """Statistics and the backward's sums from replicas: one, and conv_stat_replicas of them."""
    nrep = _C().conv_stat_replicas if nrep == 32 else nrep
    d = B.bn_inputs((M, C), cuda, res=res, seed=4)
    y, mask, mean, invstd = _forward(d, relu, res, want_mask, nrep=nrep)
    _backward(d, y, mask, mean, invstd, relu, res, nreps=(nrep,))


@pytest.mark.parametrize("own", [True, False])
@pytest.mark.parametrize("edge", [e for e in B.EDGES if e])
@pytest.mark.parametrize("M,C", [(333, 72), (1000, 8)])
def test_bn_value_edges(cuda, M, C, edge, own):
    """'offset' is where the sums form's variance and the table's D lose accuracy by design (the bounds say by how
    much) and the shifted reduction must not; 'const' is var = 0; 'tiny' invstd about 300; 'mixed' a small channel
    next to a large one; 'zero_g' a channel whose gradient sums are exactly zero."""
    d = B.bn_inputs((M, C), cuda, res=False, edge=edge, seed=5)
    nrep = None if own else _C().conv_stat_replicas
    y, mask, mean, invstd = _forward(d, True, False, True, nrep=nrep, edge=edge)
    _backward(d, y, mask, mean, invstd, True, False, nreps=(32,))
    if edge == "zero_g":
        c0 = B.edge_channel(C)
        dg, db = _nan(C, cuda), _nan(C, cuda)
        _C().bn_bwd(d["dy"], d["x"], None, mean, invstd, d["gamma"], d["beta"], True, dg, db, False)
        assert float(dg[c0]) == 0.0 and float(db[c0]) == 0.0


@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("N,H,W", [(2, 5, 7), (1, 4, 4), (3, 1, 1)])
def test_bn_from_sums_subsample(cuda, N, H, W, C):
    d = B.bn_inputs((N, H, W, C), cuda, res=True, seed=6)
    for res in (False, True):
        _forward(d, True, res, True, nrep=_C().conv_stat_replicas, sub2=True)


@pytest.mark.parametrize("M,C", [(1, 8), (9, 24), (333, 72), (64, 2056)])
def test_bn_eval(cuda, M, C):
    """Eval mode: mean is run_mean, invstd its (run_var + eps)^-1/2 (the addition and a 2-ulp rsqrt: 8 u), the running
    statistics are left alone."""
    d = B.bn_inputs((M, C), cuda, res=True, seed=7)
    rm0, rv0 = _run_stats(C, cuda)
    for relu, res in [(True, False), (True, True), (False, False)]:
        rm, rv = rm0.clone(), rv0.clone()
        r = d["res"] if res else None
        _dirty(d["x"])
        y, mean, invstd, mask = _C().bn_fwd(d["x"], r, d["gamma"], d["beta"], rm, rv, False, MOM, EPS, relu, True)
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and torch.equal(mean, rm0)
        want = 1.0 / torch.sqrt(rv0.double() + EPS)
        B.assert_within(invstd, want, 8 * B.U * want, "invstd")
        o64 = B.bn_apply(d["x"], mean, invstd, d["gamma"], d["beta"], r, relu)
        B.check_fwd(y, mask, o64, B.bn_apply(d["x"], mean, invstd, d["gamma"], d["beta"], r, relu, dtype=F32))


@pytest.mark.parametrize("nrep", [1, 32])
@pytest.mark.parametrize("edge", [None, "offset", "const"])
@pytest.mark.parametrize("M,C", [(1, 8), (333, 72), (64, 2056)])
def test_bn_finalize(cuda, M, C, edge, nrep):
    d = B.bn_inputs((M, C), cuda, edge=edge, seed=8)
    sums = B.sums_from(d["x"], nrep)
    rm0, rv0 = _run_stats(C, cuda)
    rm, rv = rm0.clone(), rv0.clone()
    _dirty(d["x"])
    mean, invstd, params = _C().bn_finalize(sums, d["gamma"], d["beta"], rm, rv, M, MOM, EPS)
    st = B.bn_stats_from_sums(sums, M, EPS)
    B.check_stats_sums(mean, invstd, st, EPS)
    B.check_running(rm, rv, rm0, rv0, st, False, MOM, EPS)
    # [scale | shift] from the returned mean / invstd: one rounding; an fma, 3 u of its terms (B.bn_bwd_bounds)
    sc = d["gamma"].double() * invstd.double()
    B.assert_within(params[:C], sc, 2 * B.U * sc.abs(), "scale")
    B.assert_within(params[C:], d["beta"].double() - mean.double() * sc,
                    3 * B.U * (d["beta"].double().abs() + (mean.double() * sc).abs()), "shift")


# =============================================================================================== two BatchNorms
@pytest.mark.parametrize("edge", [None, "offset"])
@pytest.mark.parametrize("M,C", [(1, 8), (7, 8), (9, 24), (63, 64), (333, 72), (98, 80), (4099, 8), (98, 2048),
                                 (64, 2056)])
def test_bn_dual(cuda, M, C, edge):
    """y = relu(BN(x) + BN_r(xr)) and both backwards from one masked dy: own reduce and sums, whole and in halves."""
    C_ = _C()
    R = C_.conv_stat_replicas
    d = B.bn_inputs((M, C), cuda, edge=edge, dual=True, seed=9)
    x, x2, dy = d["x"], d["x2"], d["dy"]
    g1, b1, g2, b2 = d["gamma"], d["beta"], d["gamma2"], d["beta2"]
    s1, s2 = B.sums_from(x, R), B.sums_from(x2, 1)
    rm0, rv0 = _run_stats(C, cuda)
    rma, rva, rmb, rvb = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    _dirty(x)
    y, mean, invstd, mask, mean2, invstd2 = C_.bn_fwd_from_sums_dual(x, s1, g1, b1, rma, rva, x2, s2, g2, b2, rmb, rvb,
                                                                     MOM, EPS)
    for (mu, is_, rm, rv, s, what) in [(mean, invstd, rma, rva, s1, "first "),
                                       (mean2, invstd2, rmb, rvb, s2, "second ")]:
        st = B.bn_stats_from_sums(s, M, EPS)
        B.check_stats_sums(mu, is_, st, EPS, what)
        B.check_running(rm, rv, rm0, rv0, st, False, MOM, EPS, what)
    second = (x2, mean2, invstd2, g2, b2)
    o64 = B.bn_apply(x, mean, invstd, g1, b1, None, True, second)
    B.check_fwd(y, mask, o64, B.bn_apply(x, mean, invstd, g1, b1, None, True, second, dtype=F32))

    bits = B.unpack_bits(mask, x.shape)
    oa = B.bn_bwd(dy, x, bits, mean, invstd, g1, b1)
    ob = B.bn_bwd(dy, x2, bits, mean2, invstd2, g2, b2)
    ba, bb = B.bn_bwd_bounds(oa), B.bn_bwd_bounds(ob)
    for nrep in (None, 1, R):
        pre = (None, None) if nrep is None else (B.bwd_sums_from(oa["g"], x, mean, nrep),
                                                 B.bwd_sums_from(ob["g"], x2, mean2, nrep, second=True))
        v = [_nan(C, cuda) for _ in range(4)]
        _dirty(x)
        dx, dx2 = C_.bn_bwd_dual(dy, mask, x, mean, invstd, g1, b1, v[0], v[1], x2, mean2, invstd2, g2, b2, v[2],
                                 v[3], *pre)
        B.check_bwd(dx, None, v[0], v[1], oa, "dual %s first " % nrep, ba)
        B.check_bwd(dx2, None, v[2], v[3], ob, "dual %s second " % nrep, bb)
        assert M == 1 or not torch.equal(dx, dx2)  # one row: xhat = 0 and g = mean(g), both are zero
        w = [_nan(C, cuda) for _ in range(4)]
        _dirty(x)
        p, p2 = C_.bn_bwd_dual_params(dy, mask, x, mean, invstd, g1, b1, w[0], w[1], x2, mean2, invstd2, g2, b2, w[2],
                                      w[3], *pre)
        B.check_table(p, oa, ba, "dual %s first " % nrep)
        B.check_table(p2, ob, bb, "dual %s second " % nrep)
        for a, c in zip(v, w):
            assert torch.equal(a, c), "bn_bwd_dual and bn_bwd_dual_params disagree on dgamma / dbeta"
        _dirty(x)
        assert torch.equal(C_.bn_bwd_apply(dy, x, mask, p), dx) and torch.equal(C_.bn_bwd_apply(dy, x2, mask, p2), dx2)


# =============================================================================================== stem: BN + ReLU + pool
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("N,H,W", [(2, 5, 7), (1, 8, 8), (1, 1, 1)])
def test_bn_relu_maxpool(cuda, N, H, W, C):
    C_ = _C()
    R = C_.conv_stat_replicas
    d = B.bn_inputs((N, H, W, C), cuda, seed=10)
    x, g, b = d["x"], d["gamma"], d["beta"]
    M = N * H * W
    sums = B.sums_from(x, R)
    rm0, rv0 = _run_stats(C, cuda)
    rm, rv, rmz, rvz = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    _dirty(x)
    y, idx, mean, invstd = C_.bn_relu_maxpool(x, sums, g, b, rm, rv, MOM, EPS)
    st = B.bn_stats_from_sums(sums, M, EPS)
    B.check_stats_sums(mean, invstd, st, EPS)
    B.check_running(rm, rv, rm0, rv0, st, False, MOM, EPS)
    # the BatchNorm output the pool never stores, from the apply kernel on the same x and sums
    z, meanz, invstdz = C_.bn_fwd_from_sums(x, None, g, b, sums, rmz, rvz, MOM, EPS, True)
    assert torch.equal(meanz, mean) and torch.equal(invstdz, invstd)
    win = B.pool_windows(z.float(), float("-inf"))
    top = win.max(3).values
    assert torch.equal(y.float(), top), "pooled y is not the window maximum of the bf16 z"
    pos = torch.arange(9, device=cuda).reshape(1, 1, 1, 9, 1)
    first = torch.where(win == top.unsqueeze(3), pos, torch.full_like(pos, 9)).min(3).values
    assert torch.equal(idx.long(), first), "idx is not the first arg-max"
    # the pooled y bounded: rounding is monotonic, so max of the rounded is the rounded max, and
    # |max a - max b| <= max |a - b| over the window
    o64 = B.bn_apply(x, mean, invstd, g, b, None, True)
    delta = B.y_delta(o64, B.bn_apply(x, mean, invstd, g, b, None, True, dtype=F32))
    B.assert_rounded(y, B.pool_windows(o64["y"], float("-inf")).max(3).values,
                     B.pool_windows(delta, 0.0).max(3).values, "pooled y")

    torch.manual_seed(12)
    dpool = torch.randn(y.shape, device=cuda).bfloat16()
    bits = z > 0
    o64 = B.pool_bn_bwd(dpool, idx, x, bits, mean, invstd, g, b)
    dg, db = _nan(C, cuda), _nan(C, cuda)
    _dirty(x)
    dx = C_.pool_bn_bwd(dpool, idx, x, mean, invstd, g, b, dg, db)
    B.check_bwd(dx, None, dg, db, o64, "pool own reduce ")
    # sums over the pooled gradient (what the consumers' data-gradient epilogues accumulate)
    o64s = B.pool_bn_bwd(dpool, idx, x, bits, mean, invstd, g, b, from_sums=True)
    dg, db = _nan(C, cuda), _nan(C, cuda)
    _dirty(x)
    dx = C_.pool_bn_bwd(dpool, idx, x, mean, invstd, g, b, dg, db, B.bwd_sums_from(o64s["g_sums"], x, mean, R))
    B.check_bwd(dx, None, dg, db, o64s, "pool sums ")


# =============================================================================================== argument checks
def _args(C, cuda, M=2):
    x = torch.zeros(M, C, device=cuda, dtype=BF16)
    v = lambda n=1: torch.ones(n * C, device=cuda)  # noqa: E731
    mask = torch.zeros(max(M * C // 8, 1), device=cuda, dtype=torch.uint8)
    sums = lambda r=1: torch.zeros(r, 2, C, device=cuda)  # noqa: E731
    return x, v, mask, sums


@pytest.mark.parametrize("C", [4, 12, 20])
def test_bn_rejects_channels_not_in_groups_of_8(cuda, C):
    """Every kernel moves 16-byte groups of 8 channels: before the check bn_bwd, and the two-BatchNorm backwards given
    sums, took such a C and left the last C % 8 channels of dx, dgamma and dbeta unwritten (C < 8: a division by 0).
    Every entry point refuses before it allocates or launches."""
    C_ = _C()
    x, v, mask, sums = _args(C, cuda)
    x4 = x.reshape(1, 1, 2, C)
    idx = torch.zeros(1, 1, 1, C, device=cuda, dtype=torch.uint8)
    dp = torch.zeros(1, 1, 1, C, device=cuda, dtype=BF16)
    m8 = "multiple of 8"
    with pytest.raises(RuntimeError, match=m8):
        C_.bn_fwd(x, None, v(), v(), v(), v(), True, MOM, EPS, True)
    with pytest.raises(RuntimeError, match=m8):
        C_.bn_fwd_from_sums(x, None, v(), v(), sums(), v(), v(), MOM, EPS, True)
    with pytest.raises(RuntimeError, match=m8):
        C_.bn_fwd_from_sums_dual(x, sums(), v(), v(), v(), v(), x, sums(), v(), v(), v(), v(), MOM, EPS)
    with pytest.raises(RuntimeError, match=m8):
        C_.bn_finalize(sums(), v(), v(), v(), v(), 2, MOM, EPS)
    for s in (None, sums()):
        with pytest.raises(RuntimeError, match=m8):
            C_.bn_bwd(x, x, None, v(), v(), v(), v(), True, v(), v(), False, None, s)
        with pytest.raises(RuntimeError, match=m8):
            C_.bn_bwd_params(x, x, None, s, v(), v(), v(), v(), v(), v())
        for fn in (C_.bn_bwd_dual, C_.bn_bwd_dual_params):
            with pytest.raises(RuntimeError, match=m8):
                fn(x, mask, x, v(), v(), v(), v(), v(), v(), x, v(), v(), v(), v(), v(), v(), s, s)
    with pytest.raises(RuntimeError, match=m8):
        C_.bn_bwd_apply(x, x, None, v(4))
    with pytest.raises(RuntimeError, match="divide 256"):
        C_.bn_relu_maxpool(x4, sums(), v(), v(), v(), v(), MOM, EPS)
    with pytest.raises(RuntimeError, match="divide 256"):
        C_.pool_bn_bwd(dp, idx, x4, v(), v(), v(), v(), v(), v())


def test_bn_bwd_rejects_what_it_documents(cuda):
    C_ = _C()
    C, M = 16, 4
    x, v, mask, sums = _args(C, cuda, M)
    R = C_.conv_stat_replicas

    def bwd(dy=x, y=None, relu_x=False, want_dres=False, mask=None, sums=None, gamma=None):
        return C_.bn_bwd(dy, x, y, v(), v(), gamma if gamma is not None else v(), v(), relu_x, v(), v(), want_dres,
                         mask, sums)

    def dual(x2=x, s=None, s2=None, mask=mask):
        return C_.bn_bwd_dual(x, mask, x, v(), v(), v(), v(), v(), v(), x2, v(), v(), v(), v(), v(), v(), s, s2)

    for kw in ({"relu_x": True, "y": x}, {"relu_x": True, "mask": mask}, {"y": x, "mask": mask}):
        with pytest.raises(RuntimeError, match="exclusive"):
            bwd(**kw)
    with pytest.raises(RuntimeError, match="sums: with the packed mask or relu_x"):
        bwd(sums=sums())
    with pytest.raises(RuntimeError, match="sums: with the packed mask or relu_x"):
        bwd(y=x, sums=sums())
    with pytest.raises(RuntimeError, match="no dres"):
        bwd(relu_x=True, want_dres=True, sums=sums())
    with pytest.raises(RuntimeError, match="come together"):
        dual(s=sums())
    with pytest.raises(RuntimeError, match="come together"):
        C_.bn_bwd_dual_params(x, mask, x, v(), v(), v(), v(), v(), v(), x, v(), v(), v(), v(), v(), v(), None, sums())
    with pytest.raises(RuntimeError, match="same replica count"):
        dual(s=sums(1), s2=sums(2))
    # shapes
    other = torch.zeros(M + 1, C, device=cuda, dtype=BF16)
    with pytest.raises(RuntimeError, match="shape of x"):
        bwd(dy=other)
    with pytest.raises(RuntimeError, match="shape of x"):
        bwd(y=other)
    with pytest.raises(RuntimeError, match="shape of x"):
        dual(x2=other)
    with pytest.raises(RuntimeError, match="shape of x"):
        C_.bn_fwd(x, other, v(), v(), v(), v(), True, MOM, EPS, True)
    with pytest.raises(RuntimeError, match="packed uint8"):
        bwd(mask=mask[:-1])
    with pytest.raises(RuntimeError, match="packed uint8"):
        dual(mask=torch.cat([mask, mask]))
    with pytest.raises(RuntimeError, match="fp32 elements"):
        bwd(gamma=v(2))
    with pytest.raises(RuntimeError, match=r"must be fp32 \["):
        bwd(relu_x=True, sums=torch.zeros(2 * C + 1, device=cuda))
    with pytest.raises(RuntimeError, match="conv_stat_replicas"):  # the pool's sums: exactly that many replicas
        C_.pool_bn_bwd(torch.zeros(1, 1, 1, C, device=cuda, dtype=BF16),
                       torch.zeros(1, 1, 1, C, device=cuda, dtype=torch.uint8), x.reshape(1, 2, 2, C), v(), v(), v(),
                       v(), v(), v(), sums(R + 1))
    with pytest.raises(RuntimeError, match="want_sub2"):
        C_.bn_fwd_from_sums(x, None, v(), v(), sums(), v(), v(), MOM, EPS, True, False, True)
    # the params table of bn_bwd_apply
    with pytest.raises(RuntimeError, match="fp32 elements"):
        C_.bn_bwd_apply(x, x, None, v(2))
    with pytest.raises(RuntimeError, match="fp32 elements"):
        C_.bn_bwd_apply(x, x, mask, v(5))
    with pytest.raises(RuntimeError, match="GPU tensor|device"):
        C_.bn_bwd_apply(x, x, None, torch.ones(4 * C))
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="device"):
            C_.bn_bwd_apply(x, x, None, torch.ones(4 * C, device="cuda:1"))
