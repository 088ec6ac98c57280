"""norm.hip, xent.hip and elementwise.hip per element against the fp64 oracles of tests/row_oracles.py.

Every bound here is one of three kinds: a form derived from the arithmetic (the mean / rstd / lse / loss / gradient /
rope forms and assert_fp32_sum's k 2^-24 sum|terms|), a reference-against-reference measurement (16 x the largest
distance between the oracle evaluated in fp32 and in fp64 on the case's own inputs, O.measured_delta; the sizes seen
are written next to each use), or a measurement plus a derivation written where it is added. None was fitted to a
kernel's output. The CPU tier (test_row_oracles_cpu.py) shows that a plain fp32 evaluation stays inside each of them.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_oracles as O  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
IGN = -100
NAN = float("nan")
NINF = float("-inf")


def _C():
    from k8s_amd.ops._ext import load

    return load()


# =============================================================================================== LayerNorm / RMSNorm
def _norm_case(dev, R, D, rms, res, edge=None):
    """Forward, then the backward with dres (res) or with and without the dx column sums (no res)."""
    C = _C()
    x, r, g, b, dy, dres = O.norm_inputs(R, D, rms, res, dev, edge=edge)
    y, mean, rstd, xs = C.norm_fwd(x, r, g, b, O.EPS, rms)
    f64 = O.norm_fwd(x, r, g, b, O.EPS, rms)
    f32 = O.norm_fwd(x, r, g, b, O.EPS, rms, dtype=F32)
    if res:
        assert torch.equal(xs, f64["xsum"]), "xsum is not bf16(x + r)"
    if not rms:
        O.assert_within(mean, f64["mean"], 8 * O.U * f64["mean_abs"], "mean")
    O.assert_within(rstd, f64["rstd"], 32 * O.U * f64["rstd"], "rstd")
    # measured: 2e-7 .. 1.1e-6 on randn rows (x16: up to 1.7e-5), 6e-6 (x16: 1e-4) on the x + 64 rows; bf16's own
    # half ulp at |y| = 1 is 3.9e-3. norm_y_delta adds the mean / rstd bounds carried through the formula.
    O.assert_rounded(y, f64["y"], O.norm_y_delta(f64, g, O.measured_delta(f32["y"], f64["y"])), "y")
    if edge == "equal" and not rms:  # the all-equal row: rstd = eps^-1/2 and y = beta, to the derived part of delta
        row = min(5, R - 1)
        assert abs(float(f64["rstd"][row]) - O.EPS ** -0.5) < 1e-9
        O.assert_rounded(y[row], b.double(), O.norm_y_delta(f64, g, 0.0)[row], "y = beta on the all-equal row")

    xin = xs if res else x
    o64 = O.norm_bwd(dy, xin, g, mean, rstd, dres, rms)
    o32 = O.norm_bwd(dy, xin, g, mean, rstd, dres, rms, dtype=F32)
    # measured: up to 1.2e-6 on randn rows (x16: 2e-5); 7.6e-5 (x16: 1.2e-3) with the all-equal row, whose rstd is 316
    # and dx up to 1e3; 2.2e-4 (x16: 3.5e-3) on the x * 1e-3 rows, rstd 300 on every row
    ddx = O.measured_delta(o32["dx"], o64["dx"])

    def run(want_dsum):
        dg = torch.full((D,), NAN, device=dev)
        db = None if rms else torch.full((D,), NAN, device=dev)
        ds = torch.full((D,), NAN, device=dev) if want_dsum else None
        dx = C.norm_bwd(dy, xin, g, mean, rstd, dres, dg, db, rms, dsum=ds)
        O.assert_rounded(dx, o64["dx"], ddx, "dx")
        O.assert_fp32_sum(dg, o64["dgamma"], o64["abs_dgamma"], what="dgamma")
        if not rms:
            O.assert_fp32_sum(db, o64["dbeta"], o64["abs_dbeta"], what="dbeta")
        if want_dsum:
            O.assert_fp32_sum(ds, o64["dsum"], o64["abs_dsum"], what="dsum")
        return dx, dg

    if res:
        run(False)
    else:
        dx0, dg0 = run(False)
        dx1, dg1 = run(True)
        assert torch.equal(dx0, dx1) and torch.equal(dg0, dg1), "asking for dsum changed dx or dgamma"


# D: 8 one lane | 136 partial row | 512 CPL 1 full | 520 CPL 2, one lane in the second chunk | 1032 CPL 4, chunk 2 held
# by lane 0 alone and chunk 3 empty | 2048 CPL 4 full | 4104 CPL 16 partial | 8192 CPL 16 full
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("R", [1, 3, 64, 257])
@pytest.mark.parametrize("D", [8, 136, 512, 520, 1032, 2048, 4104, 8192])
def test_norm_row_lengths(cuda, D, R, res, rms):
    _norm_case(cuda, R, D, rms, res)


# The one-pass backward (D <= 1024, R >= 16384). Without dres the three-slot prefetch form runs, with dres the
# two-slot form, which walks a wave's rows in pairs and leaves on the first odd one.
# R: 16384 = 128 blocks, ungrouped fold | 16385 = 129 blocks, grouped fold, last wave one row (the three-slot form's
# first exit) | 16418 = the last block's waves hold 32 and 2 rows (its second exit on a tail) | 16411 the odd tail
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("R", [16384, 16385, 16418, 16411])
@pytest.mark.parametrize("D", [8, 136, 520, 1024])
def test_norm_fused_backward_tails(cuda, D, R, res, rms):
    _norm_case(cuda, R, D, rms, res)


@pytest.mark.parametrize("rms", [False, True])
def test_norm_two_launch_wide_partial_blocks(cuda, rms):
    """33000 rows of 1032: norm_param_rows is 96 (more than a block's 64), the last block has 72 rows."""
    _norm_case(cuda, 33000, 1032, rms, False)


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("edge", ["small", "offset", "equal", "gamma"])
def test_norm_value_edges(cuda, edge, rms):
    _norm_case(cuda, 257, 520, rms, False, edge=edge)


@pytest.mark.parametrize("D", [12, 8200])
def test_norm_bwd_rejects_row_lengths_the_kernels_cannot_take(cuda, D):
    """Before any launch: D = 8200 used to run the CPL 16 kernel and leave the columns past 8192 unwritten."""
    R = 2
    x = torch.zeros(R, D, device=cuda, dtype=BF16)
    g = torch.ones(D, device=cuda)
    mean, rstd = torch.zeros(R, device=cuda), torch.ones(R, device=cuda)
    dg, db = torch.empty(D, device=cuda), torch.empty(D, device=cuda)
    with pytest.raises(RuntimeError, match="multiple of 8 and <= 8192"):
        _C().norm_bwd(x, x, g, mean, rstd, None, dg, db, False)
    with pytest.raises(RuntimeError, match="multiple of 8 and <= 8192"):
        _C().norm_fwd(x, None, g, g, O.EPS, False)
    torch.cuda.synchronize()


@pytest.mark.parametrize("rms", [False, True])
def test_norm_no_rows(cuda, rms):
    C, D = _C(), 64
    x = torch.empty(0, D, device=cuda, dtype=BF16)
    g = torch.ones(D, device=cuda)
    b = None if rms else torch.ones(D, device=cuda)
    y, mean, rstd, xs = C.norm_fwd(x, x, g, b, O.EPS, rms)
    assert y.shape == (0, D) and xs.shape == (0, D) and rstd.shape == (0,)
    dg = torch.full((D,), NAN, device=cuda)
    db = None if rms else torch.full((D,), NAN, device=cuda)
    ds = torch.full((D,), NAN, device=cuda)
    dx = C.norm_bwd(x, x, g, mean, rstd, None, dg, db, rms, dsum=ds)
    torch.cuda.synchronize()
    assert dx.shape == (0, D)
    zero = torch.zeros(D, device=cuda)
    assert torch.equal(dg, zero) and torch.equal(ds, zero) and (rms or torch.equal(db, zero))


# =============================================================================================== cross entropy
def _xent_fwd_check(x, lab, smoothing):
    """xent_fwd on x (a view is fine) against the oracle; returns the kernel's lse."""
    loss, lse = _C().xent_fwd(x, lab, IGN, smoothing)
    f64 = O.xent_fwd(x, lab, IGN, smoothing)
    O.assert_within(lse, f64["lse"], O.lse_bound(f64["lse"]), "lse")
    O.assert_within(loss, f64["loss"], O.loss_bound(f64, smoothing), "loss")
    assert torch.equal(loss[~f64["valid"]], torch.zeros_like(loss[~f64["valid"]]))
    return lse


def _xent_eval_check(x, lab):
    loss, rank = _C().xent_eval(x, lab, IGN)
    f64 = O.xent_fwd(x, lab, IGN, 0.0)
    O.assert_within(loss, f64["loss"], O.loss_bound(f64, 0.0), "eval loss")
    R, V = x.shape
    valid = f64["valid"]
    xl = x.gather(1, torch.where(valid, lab, torch.zeros_like(lab))[:, None])
    before = torch.arange(V, device=x.device)[None, :] < lab[:, None]
    want = ((x > xl) | ((x == xl) & before)).sum(1)
    assert torch.equal(rank.long(), torch.where(valid, want, torch.full_like(want, V))), "rank"


def _xent_bwd_check(full, V, lab, lse, dscale, smoothing):
    """xent_bwd on the dense [R, Vpad] logits (classes in the first V columns) from the kernel's own lse."""
    d = _C().xent_bwd(full, lab, lse, dscale, IGN, smoothing, V)
    assert d.shape == full.shape and d.dtype == full.dtype
    o = O.xent_bwd(full[:, :V], lab, lse, dscale, IGN, smoothing)
    O.assert_within(d[:, :V], o["grad"], O.xent_grad_bound(o, full.dtype == BF16), "grad")
    assert torch.equal(d[:, V:], torch.zeros_like(d[:, V:])), "pad columns of the gradient"
    ign = lab == IGN
    assert torch.equal(d[ign], torch.zeros_like(d[ign])), "gradient of an ignored row"
    return d


def _row_scales(R, dev):
    return torch.linspace(0.2, 1.7, R, device=dev)  # distinct per row


_WIDTHS = [(V, s) for V in (5, 8, 1000, 1001, 2048, 2059) for s in (0.0, 0.1)] + [(30522, 0.1)]


# 1001 is odd: in bf16 every other row is only 2-byte aligned and the row stride is no multiple of 8, so the scalar
# path runs. 5 < 8: no vector trip at all. 2059: a second trip of the vector loop for three threads and a tail.
@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("V,smoothing", _WIDTHS)
def test_xent_widths_labels_and_scales(cuda, V, smoothing, dt):
    R = 6
    x = O.xent_logits(R, V, dt, cuda)
    lab = O.xent_labels(R, V, cuda)  # column 0, column V - 1, the scalar tail, one ignored row
    lse = _xent_fwd_check(x, lab, smoothing)
    _xent_bwd_check(x, V, lab, lse, _row_scales(R, cuda), smoothing)
    _xent_bwd_check(x, V, lab, lse, torch.tensor([0.37], device=cuda), smoothing)
    if smoothing == 0.0:
        _xent_eval_check(x, lab)
    none = torch.full((R,), IGN, device=cuda, dtype=torch.int64)  # every row ignored
    lse2 = _xent_fwd_check(x, none, smoothing)
    assert torch.equal(lse2, lse)
    d = _xent_bwd_check(x, V, none, lse, _row_scales(R, cuda), smoothing)
    assert torch.equal(d, torch.zeros_like(d))


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("V", [1000, 1003])
def test_xent_forward_never_reads_the_pad_of_a_view(cuda, V, dt):
    R = 6
    full = torch.full((R, 1024), NAN, device=cuda, dtype=dt)
    full[:, :V] = O.xent_logits(R, V, dt, cuda)
    lab = O.xent_labels(R, V, cuda)
    _xent_fwd_check(full[:, :V], lab, 0.1)
    _xent_eval_check(full[:, :V], lab)


@pytest.mark.parametrize("V", [1000, 1003])
def test_xent_forward_on_a_misaligned_base(cuda, V):
    """bf16 full[:, 4:4 + V]: the base is 8-byte aligned and ld % 8 == 0, so the 16-byte loads are off and the whole
    row takes the scalar loop."""
    R = 6
    full = torch.full((R, 1024), NAN, device=cuda, dtype=BF16)
    view = full[:, 4:4 + V]
    view.copy_(O.xent_logits(R, V, BF16, cuda))
    assert view.data_ptr() % 16 == 8
    lab = O.xent_labels(R, V, cuda)
    _xent_fwd_check(view, lab, 0.1)
    _xent_eval_check(view, lab)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("V,Vpad", [(1000, 1024), (1003, 1024)])
def test_xent_backward_padded(cuda, V, Vpad, dt):
    R = 6
    full = torch.full((R, Vpad), NAN, device=cuda, dtype=dt)
    full[:, :V] = O.xent_logits(R, V, dt, cuda)
    lab = O.xent_labels(R, V, cuda)
    lse = _xent_fwd_check(full[:, :V], lab, 0.1)
    torch.full((R * Vpad * 4,), NAN, device=cuda)  # dirty the caching allocator's free blocks
    _xent_bwd_check(full, V, lab, lse, _row_scales(R, cuda), 0.1)


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("dt,mul,shift", [(F32, 4.0, 1000.0), (F32, 4.0, -1000.0), (BF16, 120.0, 0.0)])
def test_xent_range(cuda, dt, mul, shift, smoothing):
    """fp32 rows moved by +-1000 (the loss does not move, the lse does) and bf16 logits 30 times as wide."""
    R, V = 6, 2059
    x = O.xent_logits(R, V, dt, cuda, mul=mul, shift=shift)
    lab = O.xent_labels(R, V, cuda)
    lse = _xent_fwd_check(x, lab, smoothing)
    _xent_bwd_check(x, V, lab, lse, _row_scales(R, cuda), smoothing)


@pytest.mark.parametrize("dt", [BF16, F32])
def test_xent_many_rows(cuda, dt):
    R, V = 70000, 16  # one launch of 70000 blocks
    x = O.xent_logits(R, V, dt, cuda)
    torch.manual_seed(3)
    lab = torch.randint(0, V, (R,), device=cuda)
    lab[::97] = IGN
    lse = _xent_fwd_check(x, lab, 0.1)
    torch.manual_seed(4)
    _xent_bwd_check(x, V, lab, lse, torch.rand(R, device=cuda) + 0.5, 0.1)
    _xent_eval_check(x, lab)


@pytest.mark.parametrize("pattern,dt", [("first16", BF16), ("first16", F32), ("every3rd", BF16), ("every3rd", F32),
                                        ("first16_scalar_loop", BF16)])  # an 8-byte-aligned base is a bf16 case
def test_xent_masked_classes(cuda, pattern, dt):
    """-inf logits. first16: thread 0 and 1 of the vector loop (every thread 0..15 of the scalar loop) start on -inf
    only and meet finite values one trip later -- the running maximum is -inf when the rescale is formed, which gave
    NaN. The label sits on a finite class; the masked columns' gradient is exactly zero."""
    R, V = 6, 4200
    if pattern == "first16_scalar_loop":
        full = torch.full((R, 4224), NAN, device=cuda, dtype=dt)
        x = full[:, 4:4 + V]
    else:
        x = torch.empty(R, V, device=cuda, dtype=dt)
    x.copy_(O.xent_logits(R, V, dt, cuda))
    cols = torch.arange(V, device=cuda)
    masked = cols % 3 == 0 if pattern == "every3rd" else cols < 16
    x[:, masked] = NINF
    finite = cols[~masked]
    lab = finite[(torch.arange(R, device=cuda) * 577 + 1) % finite.numel()]
    lab[0], lab[1], lab[3] = finite[0], finite[-1], IGN
    lse = _xent_fwd_check(x, lab, 0.0)
    assert torch.isfinite(lse).all()
    _xent_eval_check(x, lab)
    dense = x.contiguous()
    d = _xent_bwd_check(dense, V, lab, lse, _row_scales(R, cuda), 0.0)
    assert torch.equal(d[:, masked], torch.zeros_like(d[:, masked])), "gradient of a masked class"


def test_xent_no_rows(cuda):
    C = _C()
    for dt in (BF16, F32):
        x = torch.empty(0, 16, device=cuda, dtype=dt)
        lab = torch.empty(0, device=cuda, dtype=torch.int64)
        loss, lse = C.xent_fwd(x, lab, IGN, 0.1)
        d = C.xent_bwd(x, lab, lse, torch.ones(1, device=cuda), IGN, 0.1, 16)
        torch.cuda.synchronize()
        assert loss.shape == (0,) and lse.shape == (0,) and d.shape == (0, 16) and d.dtype == dt


# =============================================================================================== elementwise
# the gate row carries 0, +-20, +-88, +-100: exp(-g) overflows to inf past 88 and the reciprocal returns 0
@pytest.mark.parametrize("T,F,blk", [(1, 8, 0), (96, 2056, 0), (5, 128, 64)])
def test_swiglu(cuda, T, F, blk):
    C = _C()
    gu, dy = O.swiglu_inputs(T, F, cuda)
    # measured: up to 9e-7 forward and backward (x16: 1.4e-5), set by the +-88 / +-100 gates times an up value of 2
    y64, y32 = O.swiglu_fwd(gu, blk), O.swiglu_fwd(gu, blk, dtype=F32)
    O.assert_rounded(C.swiglu_fwd(gu, blk), y64, O.measured_delta(y32, y64), "swiglu_fwd")
    d64, d32 = O.swiglu_bwd(gu, dy, blk), O.swiglu_bwd(gu, dy, blk, dtype=F32)
    O.assert_rounded(C.swiglu_bwd(gu, dy, blk), d64, O.measured_delta(d32, d64), "swiglu_bwd")


# 8200 rows: 256 row blocks of 33, so the row loop takes a second trip and the trailing blocks are empty
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("R,Cn", [(37, 64), (8200, 776)])
def test_act_bwd_and_colsum(cuda, R, Cn, act):
    C = _C()
    dy, pre = O.act_inputs(R, Cn, cuda)
    if act == 1:
        saved = torch.relu(pre)
        w64 = O.relu_bwd(dy, saved)
        delta = 0.0  # dy or 0: exact
        alone = C.relu_bwd(dy, saved)
    else:
        saved = pre
        w64 = O.gelu_tanh_bwd(dy, pre)
        # derived per element (O.gelu_tanh_bwd_delta): 20 to 40 u of the element's parts, about 2e-6 |dy|, against a
        # bf16 half spacing of 2e-3 |g|. The measured form (x16 the largest error in the tensor: 2.5e-5 at 8200 x 776)
        # is as large as what a fourth-digit error of the cubic's constant moves an element by.
        delta = O.gelu_tanh_bwd_delta(dy, pre)
        alone = C.gelu_bwd(dy, pre)
    g, db = C.act_bwd_colsum(dy, saved, act)
    for got, what in ((alone, "act_bwd"), (g, "act_bwd_colsum g")):
        O.assert_rounded(got, w64, delta, what)
        # half a bf16 spacing, not a whole ulp: an error of the derivative in its fifth digit moves the elements next
        # to a rounding boundary by more than delta
        O.assert_nearest(got, w64, delta, what)
    # The kernel sums what it stores. Against the sums of the oracle's bf16-rounded g the difference is the fp32
    # summation error plus the elements that sit within delta of a rounding boundary and went the other way: each of
    # those was just checked to be a nearest rounding of a value within delta of the oracle's, so their total is added.
    gr = w64.bfloat16()
    flips = (g.double() - gr.double()).abs().sum(0)
    s, a = O.colsum(gr)
    O.assert_fp32_sum(db, s, a, extra=flips, what="column sums")
    out = torch.full((Cn,), NAN, device=cuda)
    g2, db2 = C.act_bwd_colsum(dy, saved, act, out)
    assert db2.data_ptr() == out.data_ptr() and torch.equal(out, db) and torch.equal(g2, g)


@pytest.mark.parametrize("R", [1, 37, 8200])
@pytest.mark.parametrize("Cn", [8, 776])
def test_colsum(cuda, R, Cn):
    torch.manual_seed(11)
    x = torch.randn(R, Cn, device=cuda).bfloat16()
    s, a = O.colsum(x)
    got = _C().colsum(x)
    O.assert_fp32_sum(got, s, a, what="colsum")
    out = torch.full((Cn,), NAN, device=cuda)
    got2 = _C().colsum(x, out)
    assert got2.data_ptr() == out.data_ptr() and torch.equal(out, got)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("T,H,D", [(7, 3, 16), (96, 4, 128)])
def test_rope(cuda, T, H, D, inverse):
    C = _C()
    maxpos = 512
    x, pos, table = O.rope_inputs(T, H, D, maxpos, cuda)
    assert int(pos.max()) == maxpos - 1
    want, ab = O.rope(x, pos, table, H, inverse)
    # each output is one product rounded and one fma: 2 u (|x1 cos| + |x2 sin|)
    xr = x.clone()
    C.rope_(xr, pos, table, inverse)
    O.assert_rounded(xr, want, 2 * O.U * ab, "rope, contiguous")
    # the k heads of a packed [T, 3 H D] projection, rotated in place through a column slice
    HD = H * D
    torch.manual_seed(12)
    packed = torch.randn(T, 3 * HD, device=cuda).bfloat16()
    packed[:, HD:2 * HD] = x
    before = packed.clone()
    C.rope_(packed[:, HD:2 * HD], pos, table, inverse)
    assert torch.equal(packed[:, HD:2 * HD], xr), "the strided form differs from the contiguous one"
    assert torch.equal(packed[:, :HD], before[:, :HD]) and torch.equal(packed[:, 2 * HD:], before[:, 2 * HD:])
