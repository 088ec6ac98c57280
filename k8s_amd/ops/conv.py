"""NHWC convolution (K2) on the gfx950 implicit-GEMM MFMA kernel.

Activations NHWC bf16, weights KRSC bf16. Per product:

    fwd    y  = conv(x, w)                  ConvA implicit im2col (C % 64 == 0; per-16-B-unit decode for
                                            other C % 8 == 0, e.g. the 8-channel stem)
    wgrad  dw = dy^T . im2col(x)            fp32, split-K atomics, written straight into the
                                            parameter's flat gradient slot
    dgrad  1x1, stride 1: dx = dy . w       plain GEMM, w read N-major (no transpose)
           RxS, stride 1: dx = conv(dy, w') w' = spatially flipped, in/out-swapped w
                                            (tiny per-step transform), pad' = R-1-pad
           stride s     : split by output parity (a, b): each of the s*s sub-grids of dx is a stride-1
                          conv of dy with the taps r = a + pad - s*d (d = row offset into dy), written
                          through the GEMM epilogue's sub-grid row map; parities with no taps are zero

Every ResNet-50 shape runs on these kernels (plus the streaming tall-K weight gradient of
``csrc/kernels/wgrad_stream.hip`` for the 1x1 / strided layers with few output tiles): there is no vendor
candidate in the dispatch. Round 1 timed MIOpen against our kernels per shape; with the streaming weight
gradient the whole-step difference of forcing our kernels everywhere measured at noise level (ResNet-50 b1024:
8884/8869 vs 8967/8878 img/s, scripts/gpurun/bench_ab.sh) and a cold node no longer builds MIOpen kernels
(~16 s of the job-create -> step 0 latency in round 1, profiles/r01_coldstart.md). Shapes outside the kernels'
contract (C or K not a multiple of 8, dilation, CPU tensors) go through ATen's convolution on a channels-last
view; on the GPU they are counted in ``STATS`` and warned about once.
"""
from __future__ import annotations

import collections
import functools
import os
import warnings

import torch
import torch.nn.functional as F

from k8s_amd.ops._ext import load as _load


# The data gradients also take BatchNorm-backward sums in their epilogues: nn.BnStatLink lists the link kinds and the
# routes serving each; _plan_dgrad / _plan_dgrad_strided / _plan_bwd choose the route, ROUTES counts the ones that ran.

STATS = {"hip_fwd": 0, "aten_fwd": 0, "hip_wgrad": 0, "aten_wgrad": 0, "hip_dgrad": 0, "aten_dgrad": 0,
         "bn_bstats": 0, "hip_infer": 0, "aten_infer": 0,
         # a residual BatchNorm that holds a mask-kind nn.ApplyLink: fused 1x1 backwards that applied its backward on
         # load, and apply passes (bn_bwd_apply) run for it instead, by its own backward or by the linked
         # convolution's when it could not take the deferred form
         "bn3_onload": 0, "bn3_apply": 0,
         # a downsample block's two BatchNorms (nn.bn_act_dual) holding two dual-kind links: backwards that deferred
         # both apply halves, apply passes run for a deferred half after all, and launches of the fused 1x1 backward's
         # final form (the downsample convolution's; with or without the downsample BatchNorm's backward on load)
         "dual_onload": 0, "dual_apply": 0, "fused_final": 0,
         # 3x3 forwards on the 4-wave GEMM with gathered A rows (_w4_3x3; counted in hip_fwd as well)
         "w4_3x3_fwd": 0,
         # an identity block's bn1 that holds a relu-kind link with conv1: bn1 backwards that deferred their apply
         # pass, apply passes run for bn1 after all (by its own backward, or by conv1's when it could not take the
         # deferred form), and launches of conv1_fused.hip (conv1's whole backward, bn1's applied on load)
         "conv1_onload": 0, "conv1_apply": 0, "conv1_fused": 0}
# data-gradient route name -> times executed. The names name the data gradient's contract (what it accumulates onto,
# which sums it takes), not the kernel: the fused 1x1 backward's final form is counted under the name _plan_dgrad gives
# its data gradient ("tile_final_sums"), the kernel that ran in STATS["fused_final"]; conv1_fused.hip's launches
# likewise under "short_mask_sums" and in STATS["conv1_fused"].
ROUTES = collections.Counter()


# The fused backwards' switches (NAME=0 switches off; read per call: A/B, tests), each with the switch it needs on as
# well -- the hierarchy, stated here only:
#   K8S_AMD_BWD1X1_FUSED  off: a normalize-on-load 1x1 convolution's two gradients stay on their two kernels
#   K8S_AMD_BN3_ONLOAD    off: a residual BatchNorm always runs its own apply pass
#   K8S_AMD_DUAL_ONLOAD   off: a downsample block's two BatchNorms run their dual apply pass, its downsample
#                         convolution's backward stays on its two kernels
#   K8S_AMD_CONV1_FUSED   off: an identity block's bn1 runs its own apply pass, conv1's backward stays on its two
#                         kernels (gemm_short's masked-addend data gradient, the streaming weight gradient)
_SWITCH_NEEDS = {"K8S_AMD_BWD1X1_FUSED": None, "K8S_AMD_BN3_ONLOAD": "K8S_AMD_BWD1X1_FUSED",
                 "K8S_AMD_DUAL_ONLOAD": "K8S_AMD_BN3_ONLOAD", "K8S_AMD_CONV1_FUSED": None}


def _switch_on(name) -> bool:
    return name is None or (os.environ.get(name, "1") != "0" and _switch_on(_SWITCH_NEEDS[name]))


bwd1x1_fused_on = functools.partial(_switch_on, "K8S_AMD_BWD1X1_FUSED")
bn3_onload_on = functools.partial(_switch_on, "K8S_AMD_BN3_ONLOAD")
dual_onload_on = functools.partial(_switch_on, "K8S_AMD_DUAL_ONLOAD")
conv1_fused_on = functools.partial(_switch_on, "K8S_AMD_CONV1_FUSED")


# (Round 5 built weight gradients on a second HIP stream -- each conv's dW kernel forked off the compute stream to
# overlap the data gradient and BatchNorm passes after it. The streams co-ran, but the HBM-bound kernels stretched:
# +0.7 % at b1024, noise at the b3072 default (profiles/r05_wgrad_side_ab.md); its serial-vs-side gradient test then
# failed intermittently on the GPU (1 in ~3 runs, one fixed 2e-3 difference: an unordered operand somewhere in the
# fork / join), so it was removed rather than shipped off by default.)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(y):
    return y.permute(0, 2, 3, 1).contiguous()


def _hip(*ts):
    return all(t.is_cuda and t.dtype == torch.bfloat16 for t in ts)


def fwd_ok(x, w):
    return _hip(x, w) and x.shape[-1] % 8 == 0 and w.shape[0] % 8 == 0


def _key(op, x, w, stride, padding):
    return "%s|%s|%s|%d|%d" % (op, "x".join(map(str, x.shape)), "x".join(map(str, w.shape)), stride, padding)


def fwd_uses_hip(x, w, stride, padding) -> bool:
    """Whether the forward of this shape runs on our kernel (every shape inside its contract does)."""
    return fwd_ok(x, w)


_WARNED = set()


def _vendor(op, x, w, stride, padding):
    """Count and warn once about a GPU product that has to use ATen/MIOpen (CPU tensors always use ATen: the
    plain-PyTorch oracle path, not counted)."""
    if x.is_cuda:
        STATS["aten_" + op] += 1
        key = _key("conv_" + op, x, w, stride, padding)
        if key not in _WARNED:
            _WARNED.add(key)
            warnings.warn("k8s_amd conv: %s is outside the MFMA kernels' shape contract; using ATen" % key)


def _w4_3x3(C_, x, w, stride, padding, dgrad=False):
    """Whether the 3x3 / pad-1 convolution of ``x`` [N, H, W, C] with ``w`` [K, 3, 3, C] goes to the 4-wave GEMM with
    gathered A rows (gemm256.hip ConvGather; ``dgrad``: the stride-1 data gradient, ``x`` is dy [N, H, W, K], which
    is correlated with conv_dgrad_wtrans(w) [C, 3, 3, K]). The extension's ``conv3x3_w4_use`` is the policy: K8S_AMD_CONV3X3_W4=0 (read per call)
    switches the route off, and it takes only chip-filling grids of the shapes where it measured faster."""
    use = getattr(C_, "conv3x3_w4_use", None)  # (the planners' test stubs carry no such predicate)
    K, R, S, C = (w.shape[3], 3, 3, w.shape[0]) if dgrad else w.shape
    N, H, W = x.shape[:3]
    return (use is not None and w.shape[1] == 3 and w.shape[2] == 3 and padding == 1 and x.is_contiguous()
            and w.is_contiguous() and use(N, H, W, C, K, stride, dgrad))


def conv_fwd(x, w, stride, padding, stats=None):
    """y = conv(x, w); with ``stats`` (zeroed fp32 [R, 2, K]) the epilogue also accumulates the per-channel
    sum / sum-of-squares of y for the following BatchNorm (HIP path only)."""
    if fwd_uses_hip(x, w, stride, padding):
        STATS["hip_fwd"] += 1
        C_ = _load()
        if _w4_3x3(C_, x, w, stride, padding):
            STATS["w4_3x3_fwd"] += 1
            return C_.conv3x3_w4_fwd(x, w, stride, stats)
        return C_.conv_fwd(x, w, stride, padding, 1, False, None, 0, stats)
    _vendor("fwd", x, w, stride, padding)
    return _nhwc(F.conv2d(_nchw(x), _nchw(w), None, stride, padding))


def infer_ok(x, w, scale, shift, residual=None) -> bool:
    """The inference epilogue's contract (gemm.hip TileEpi::LeanInfer): bf16 GPU operands, C % 8 == 0, K % 8 == 0, contiguous
    16-B aligned tensors, fp32 scale / shift."""
    ts = [x, w] + ([residual] if residual is not None else [])
    return (_hip(*ts) and x.shape[-1] % 8 == 0 and w.shape[0] % 8 == 0
            and all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in ts)
            and scale.is_cuda and shift.is_cuda and scale.dtype == torch.float32 and shift.dtype == torch.float32
            and scale.is_contiguous() and shift.is_contiguous())


def conv_infer(x, w, stride, padding, scale, shift, residual=None, relu=True):
    """y = act(bf16(conv(x, w) * scale + shift) + residual): an inference convolution with its BatchNorm folded to a
    per-channel fp32 affine, on the tile kernel's inference epilogue inside its contract; outside it (GPU) an ATen
    composite with the same two roundings, counted in ``STATS["aten_infer"]`` and warned about once."""
    if infer_ok(x, w, scale, shift, residual):
        STATS["hip_infer"] += 1
        return _load().conv_infer(x, w, stride, padding, scale, shift, residual, relu)
    _vendor("infer", x, w, stride, padding)
    y = F.conv2d(_nchw(x), _nchw(w), None, stride, padding).permute(0, 2, 3, 1)
    y = (y.float() * scale.float() + shift.float()).to(x.dtype)
    if residual is not None:
        y = y.float() + residual.float()
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype).contiguous()


def _aten_bwd(gy, x, w, stride, padding, need_dx, need_dw):
    dx, dw, _ = torch.ops.aten.convolution_backward(
        _nchw(gy), _nchw(x), _nchw(w), None, [stride, stride], [padding, padding], [1, 1], False, [0, 0], 1,
        [bool(need_dx), bool(need_dw), False])
    return (_nhwc(dx) if dx is not None else None), (dw.permute(0, 2, 3, 1) if dw is not None else None)


def _wgrad_hip(C_, gy, x, out, stride, padding, acc, xform=None):
    """dW (fp32, written or accumulated into ``out``): the streaming tall-K kernel where it applies (1x1 and
    strided layers with few output tiles; decided in the binding), a plain split-K GEMM for other 1x1 / stride 1
    layers (no im2col decode), else the implicit-GEMM split-K kernel. ``xform`` (fp32 [2, C] BatchNorm scale |
    shift): the activation operand is relu(x * scale + shift), normalised as the GEMM loads it (the streaming
    kernel has no such path: those shapes take the GEMMs)."""
    K, R, S, C = out.shape
    N, Ho, Wo = gy.shape[0], gy.shape[1], gy.shape[2]
    if (R == 1 and S == 1 and stride == 1 and padding == 0
            and (xform is not None or not C_.wgrad_stream_eligible(N, Ho, Wo, C, K, R, S))):
        C_.gemm(gy.reshape(-1, K), False, x.reshape(-1, C), False, out.view(K, C), True, None, 0, None, acc, 1.0, 0,
                xform_b=xform, xform_c=C if xform is not None else 0)
    else:
        C_.conv_wgrad(x, gy, out, stride, padding, 1, 0, acc, xform=xform)


# which data-gradient kernels take a non-residual BatchNorm + ReLU's backward sums (nn.BnStatLink, relu): the 3x3
# staged-window kernel and the 1x1 tile kernel (K8S_AMD_BN_BSTATS_3X3 / _GEMM = 0 for the A/B)
BSTATS_3X3 = os.environ.get("K8S_AMD_BN_BSTATS_3X3", "1") != "0"
BSTATS_GEMM = os.environ.get("K8S_AMD_BN_BSTATS_GEMM", "1") != "0"
# a stage-entry block's residual BN: sums over conv1's dgrad completed by the downsample's strided dgrad
BSTATS_ENTRY = os.environ.get("K8S_AMD_BN_BSTATS_ENTRY", "1") != "0"
# a residual BN's sums in a masked-addend 1x1 dgrad too deep for gemm_short (the tile kernel: stage 4, K = 512)
BSTATS_TILE_MASK = os.environ.get("K8S_AMD_BN_BSTATS_TILE_MASK", "1") != "0"
# a BatchNorm + ReLU's sums in the parities of a stride-2 data gradient (ResNet's stage-entry bn1). Off by default:
# the parities' epilogue x reads cost what the reduction saves (b3072: +1.7 ms in the parity kernels for the 1.55 ms of
# the three reductions; same-box A/B within noise, profiles/r06_notes.md)
BSTATS_STRIDED = os.environ.get("K8S_AMD_BN_BSTATS_STRIDED", "0") != "0"
# ... including the two-BatchNorm form at a gemm_short depth (K = 256: that epilogue spills). Off by default: the
# plain product runs on gemm_short at 659 us, the tile kernel with the sums at 1,537 us, for a ~510 us reduction
# (scripts/microbench/bst_shapes.py, profiles/r06_bst_shapes.jsonl)
BSTATS_TILE_SHORT = os.environ.get("K8S_AMD_BN_BSTATS_TILE_SHORT", "0") != "0"


def _bn_sums(C_, bn_link, C, device):
    """Zeroed fp32 [conv_stat_replicas, 2, C] for a BnStatLink's sums: the BatchNorm store's per-step scratch (one fill
    per step) where it has one, else a fresh zeros tensor."""
    R = C_.conv_stat_replicas
    if bn_link.store is not None:
        from k8s_amd.ops.nn import _zero_scratch
        return _zero_scratch(bn_link.store, device, R * 2 * C).view(R, 2, C)
    return torch.zeros(R, 2, C, device=device, dtype=torch.float32)


def _link_kind(bn_link, shape):
    """The kind of a BnStatLink that is filled, and filled for a data gradient of ``shape`` -- what every sum-taking
    route needs first -- else None. (The fill methods of the link give each kind its fields.)"""
    filled = bn_link is not None and bn_link.kind is not None and bn_link.x.shape == shape
    return bn_link.kind if filled else None


def _plan_dgrad(C_, gy, w, padding, addend, bn_link):
    """The route of a stride-1 data gradient, by name (``_dgrad_hip`` executes it). Launches and allocates nothing:
    reads shapes, contiguity, the addend's kind, the link's kind, the BSTATS_* switches and ``C_``'s predicates."""
    K, R, S, C = w.shape
    N, Ho, Wo = gy.shape[:3]
    masked = addend is not None and not torch.is_tensor(addend)  # nn.MaskedGrad: (dy, packed ReLU mask)
    kind = _link_kind(bn_link, (N, Ho + R - 1 - 2 * padding, Wo + S - 1 - 2 * padding, C))
    # the 256 / 512-channel 3x3 layers on a chip-filling grid: the 4-wave GEMM with gathered A rows, with the sums of a
    # BatchNorm + ReLU where the staged-window route would take them (and at 7x7, where no other route does)
    if _w4_3x3(C_, gy, w, 1, padding, True):
        return "w4_3x3_relu_sums" if BSTATS_3X3 and kind == "relu" and addend is None else "w4_3x3_flipped"
    if (BSTATS_3X3 and kind == "relu" and addend is None and R == 3 and S == 3 and padding == 1 and Ho == Wo
            and C_.conv3x3_staged_ok(Ho, Wo, C, K, 3, 3, 1, 1)):
        return "conv3x3_relu_sums"
    if not (R == 1 and S == 1 and padding == 0):
        return "implicit_flipped"
    M = N * Ho * Wo
    if masked:
        residual = kind in ("mask", "dual", "pool")  # a packed ReLU mask: g = bit ? dx : 0
        if residual and C_.gemm_short_bnstats_ok(M, C, K, kind == "dual"):
            return "short_mask_sums"
        # the same on the tile kernel: K = 512 (the stage-4 identity blocks) and the two-BatchNorm form past
        # gemm_short's K = 128 (a downsample block's output read by the next block's conv1 at stages 3-4)
        if (residual and BSTATS_TILE_MASK and M < 2 ** 31
                and (BSTATS_TILE_SHORT or kind != "dual" or not C_.gemm_short_bnstats_ok(M, C, K, False))):
            return "tile_mask_sums"
        return "gemm_masked_add"
    if addend is None:
        if BSTATS_GEMM and kind == "relu" and C_.gemm_dgrad_bnstats_ok(M, C, K):
            return "tile_relu_sums"
        # the first of two data gradients into a residual BN's output (a stage-entry block's conv1): the sums over
        # its values, completed by the downsample's strided dgrad (parity_complete_sums)
        if BSTATS_ENTRY and kind == "mask" and C_.gemm_short_bnstats_ok(M, C, K, False):
            return "short_entry_pending"
        return "gemm_plain"
    # the second of two data gradients into the stem pool's output (64 channels, the tile kernel): accumulated onto the
    # first's, the sums taken over the final tensor
    if kind == "pool" and addend.is_contiguous() and C % 8 == 0 and M < 2 ** 31:
        return "tile_final_sums"
    return "gemm_add"


def _dgrad_hip(C_, gy, w, padding, addend=None, bn_link=None):
    """dx on our kernels; with ``addend`` (bf16, shape of dx, or an nn.MaskedGrad) a 1x1 dgrad accumulates onto it in
    the GEMM epilogue (the fused residual-gradient add; a tensor addend is overwritten and returned). ``bn_link``
    (nn.BnStatLink): on the ``*_sums`` / ``*_pending`` routes the epilogue also accumulates the BatchNorm-backward sums
    of dx for the BatchNorm(s) that produced x, and deposits them in the link."""
    route = _plan_dgrad(C_, gy, w, padding, addend, bn_link)
    ROUTES[route] += 1
    K, R, S, C = w.shape
    ln = bn_link
    if route == "implicit_flipped":
        if addend is not None and not torch.is_tensor(addend):
            addend = addend.materialize()
        dx = C_.conv_fwd(gy, C_.conv_dgrad_wtrans(w), 1, R - 1 - padding, 1, False, None, 0, None)
        return dx if addend is None else dx.add_(addend)
    if route == "w4_3x3_flipped":
        if addend is not None and not torch.is_tensor(addend):
            addend = addend.materialize()
        dx = C_.conv3x3_w4_dgrad(gy, C_.conv_dgrad_wtrans(w))
        return dx if addend is None else dx.add_(addend)
    if route == "w4_3x3_relu_sums":
        sums = _bn_sums(C_, ln, C, gy.device)
        dx = C_.conv3x3_w4_dgrad(gy, C_.conv_dgrad_wtrans(w), ln.x, ln.gamma, ln.beta, ln.mean, ln.invstd, sums)
        ln.deposit(sums, None, dx)
        return dx
    if route == "conv3x3_relu_sums":
        sums = _bn_sums(C_, ln, C, gy.device)
        dx = C_.conv3x3_dgrad_bnstats(gy, C_.conv_dgrad_wtrans(w), ln.x, ln.gamma, ln.beta, ln.mean, ln.invstd, sums)
        ln.deposit(sums, None, dx)
        return dx
    shape = gy.shape[:3] + (C,)
    gy, w = gy.reshape(-1, K), w.reshape(K, C)
    if route == "gemm_plain":
        return C_.gemm(gy, True, w, False, None, False, None, 0, None, False, 1.0, 1).reshape(shape)
    if route == "gemm_add":
        C_.gemm(gy, True, w, False, addend.view(-1, C), False, None, 0, None, True, 1.0, 1)
        return addend
    if route == "gemm_masked_add":  # the epilogue reads dy and the mask bits itself: no materialised residual gradient
        out = torch.empty(shape, device=gy.device, dtype=gy.dtype)
        C_.gemm(gy, True, w, False, out.view(-1, C), False, None, 0, None, True, 1.0, 1,
                add_src=addend.dy.view(-1, C), add_mask=addend.mask)
        return out
    sums, sums2, x = _bn_sums(C_, ln, C, gy.device), None, ln.x.view(-1, C)
    if route == "tile_relu_sums":
        out = C_.gemm_dgrad_bnstats(gy, w, x, ln.gamma, ln.beta, ln.mean, ln.invstd, sums).view(shape)
    elif route == "short_entry_pending":
        out = C_.dgrad_short_bnstats(gy, w, None, None, x, ln.mask, ln.mean, sums).view(shape)
        ln.deposit_pending(sums)
        return out
    elif route == "tile_final_sums":
        out = addend
        C_.gemm_dgrad_bnstats_mask(gy, w, out.view(-1, C), x, ln.mask, ln.mean, sums)
    else:  # short_mask_sums / tile_mask_sums: a masked addend, one or two BatchNorms' sums
        x2 = None
        if ln.kind == "dual":
            sums2, x2 = _bn_sums(C_, ln, C, gy.device), ln.x2.view(-1, C)
        add = addend.dy.view(-1, C)
        if route == "short_mask_sums":
            out = C_.dgrad_short_bnstats(gy, w, add, addend.mask, x, ln.mask, ln.mean, sums, x2, ln.mean2,
                                         sums2).view(shape)
        else:
            out = torch.empty(shape, device=gy.device, dtype=gy.dtype)
            C_.gemm_dgrad_bnstats_mask(gy, w, out.view(-1, C), x, ln.mask, ln.mean, sums, add, addend.mask, x2,
                                       ln.mean2, sums2)
    ln.deposit(sums, sums2, out)
    return out


def _parity_taps(R, a, pad, stride):
    """[(d, r)] sorted by d: taps r of an R-tap filter that reach output rows h = i*stride + a, read from dy
    row i + d. None if the offsets are not contiguous (cannot be one stride-1 correlation)."""
    taps = sorted(((a + pad - r) // stride, r) for r in range(R) if (a + pad - r) % stride == 0)
    if taps and [d for d, _ in taps] != list(range(taps[0][0], taps[0][0] + len(taps))):
        return None
    return taps


def strided_dgrad_ok(gy, w, stride, padding):
    K, R, S, C = w.shape
    if stride < 2 or K % 8 or C % 8:
        return False
    for a in range(stride):
        for b in range(stride):
            tr, ts = _parity_taps(R, a, padding, stride), _parity_taps(S, b, padding, stride)
            if tr is None or ts is None:
                return False
            if tr and ts and tr[0][0] != ts[0][0]:
                return False  # one pad for both dims
    return True


def _plan_dgrad_strided(gy, w, stride, padding, H, W, addend, bn_link):
    """The route of a strided data gradient, by name (``_dgrad_strided_hip`` executes it); launches and allocates
    nothing. A pending link this data gradient cannot complete is cleared: its BatchNorm takes its own reduction."""
    K, R, S, C = w.shape
    kind = _link_kind(bn_link, (gy.shape[0], H, W, C))
    if bn_link is not None and bn_link.pending:
        # completing a residual BN's backward sums started by the first data gradient into `addend`
        # (short_entry_pending): the live parity's epilogue adds the changes it makes (gemm.hip TileEpi::LeanBnBwd, sub-grid rows)
        if (kind is not None and R == 1 and S == 1 and padding == 0 and torch.is_tensor(addend)
                and addend.is_contiguous() and addend.shape == bn_link.x.shape):
            return "parity_complete_sums"
        bn_link.drop_pending()
    # a BatchNorm + ReLU's sums (ResNet's bn1 before a stride-2 3x3 conv2): every parity stores its own pixels and adds
    # the sums over them (gemm.hip BST sub-grid path, relu kind)
    if BSTATS_STRIDED and kind == "relu" and addend is None and C > 64 and K % 64 == 0:
        return "parity_relu_sums"
    return "parity"


def _dgrad_strided_hip(C_, gy, w, stride, padding, H, W, addend=None, bn_link=None):
    """dx [N, H, W, C] of a stride-s conv on our implicit-GEMM kernel, one launch per output parity.

    With ``addend`` (bf16 [N, H, W, C], e.g. the gradient the block input already got from the other branch)
    every parity accumulates onto it in the GEMM epilogue and it is returned: no memset for the parities no
    tap reaches (they keep the addend) and no separate add pass."""
    route = _plan_dgrad_strided(gy, w, stride, padding, H, W, addend, bn_link)
    ROUTES[route] += 1
    K, R, S, C = w.shape
    ln = bn_link
    tail = (addend is not None,)  # conv_fwd_subgrid's last arguments: accumulate onto dx[, what the sums need]
    if route == "parity_complete_sums":
        tail = (True, ln.x, ln.mask, ln.mean, ln.sums)
    elif route == "parity_relu_sums":
        rsums = _bn_sums(C_, ln, C, gy.device)
        tail = (False, ln.x, None, ln.mean, rsums, ln.gamma, ln.beta, ln.invstd)
    live = [(a, b, _parity_taps(R, a, padding, stride), _parity_taps(S, b, padding, stride))
            for a in range(stride) for b in range(stride)]
    live = [(a, b, tr, ts) for a, b, tr, ts in live if tr and ts]
    if addend is not None:
        dx = addend
    else:
        # parities no tap reaches are zero: one contiguous memset beats strided fills of the sub-grids
        # (1x1 stride-2: 3 of 4 parities; strided fills made that path 1.8x slower than MIOpen)
        alloc = torch.zeros if len(live) < stride * stride else torch.empty
        dx = alloc(gy.shape[0], H, W, C, device=gy.device, dtype=gy.dtype)
    # every parity's [C, Tr, Ts, K] sub-weight gathered by one kernel (taps r*S + s, row-major over Tr x Ts)
    packed, offs = C_.conv_dgrad_wsub(w, [[r * S + s_ for _, r in tr for _, s_ in ts] for _, _, tr, ts in live])
    offs = offs.tolist()
    for i, (a, b, tr, ts) in enumerate(live):
        n = C * len(tr) * len(ts) * K
        wsub = packed[offs[i]:offs[i] + n].view(C, len(tr), len(ts), K)
        Hs, Ws = (H - a + stride - 1) // stride, (W - b + stride - 1) // stride
        C_.conv_fwd_subgrid(gy, wsub, -tr[0][0], Hs, Ws, dx, stride, a, b, *tail)
    if route == "parity_complete_sums":
        ln.complete(dx)
    elif route == "parity_relu_sums":
        ln.deposit(rsums, None, dx)
    return dx


def conv1_fused_shape_ok(C_, M, K, C) -> bool:
    """Whether conv1_fused.hip takes a (C -> K)-channel 1x1 convolution over M rows (the planners' test stubs carry no
    such predicate: no)."""
    ok = getattr(C_, "conv1_fused_ok", None)
    return ok is not None and bool(ok(M, K, C))


def fused_candidate(C_, x, w, stride, padding, x_kind, slot_ok, onload):
    """The forward-known half of the fused backward families' contracts, written once for the forward's offer
    (``offer_family``) and for ``_plan_bwd``: the one family this convolution's backward can be, else None. A
    contiguous x into a 1x1 / stride-1 / pad-0 filter, ``x_kind`` the ``_link_kind`` of the BnStatLink on x, and
      "fused_1x1"    x normalised on load (``onload``), a relu-kind link, ``bwd1x1_fused_ok``
      "fused_final"  a stored x, a pool-kind link, ``bwd1x1_final_ok``    } bf16 GPU operands, dw into the parameter's
      "conv1_fused"  a stored x, a mask-kind link, ``conv1_fused_ok``     } fp32 slot, x not subsampled (``slot_ok``)"""
    K, R, S, C = w.shape
    if not (R == 1 and S == 1 and stride == 1 and padding == 0 and x.is_contiguous()):
        return None
    M = x.numel() // C
    if onload:
        return "fused_1x1" if x_kind == "relu" and C_.bwd1x1_fused_ok(M, C, K) else None
    if not (slot_ok and _hip(x, w)):
        return None
    if x_kind == "pool" and C_.bwd1x1_final_ok(M, C, K):
        return "fused_final"
    if x_kind == "mask" and conv1_fused_shape_ok(C_, M, K, C):
        return "conv1_fused"
    return None


def offer_family(C_, x, w, stride, padding, x_kind, slot_ok, onload=False, grad_link=None):
    """The forward's question: the fused family this convolution's backward will be as far as it can know, so that
    it may offer to take the apply pass of the BatchNorm reading its output (``nn.ApplyLink``), else None:
    ``fused_candidate`` plus what only the forward sees -- which reader of x this is (``grad_link``: "fused_final" is
    one of two on a shared link, "conv1_fused" gets a residual gradient on a link of its own), that x wants a
    gradient, and for the final form ``dual_onload_on()`` as of now."""
    family = fused_candidate(C_, x, w, stride, padding, x_kind, slot_ok, onload)
    if family == "fused_final":
        return family if grad_link is not None and grad_link.shared and x.requires_grad and dual_onload_on() else None
    if family == "conv1_fused":
        return family if grad_link is not None and not grad_link.shared and x.requires_grad else None
    return family


def _plan_bwd(C_, gy, x, w, stride, padding, addend, xform, bn_link, dw_ok=True, apply_link=None):
    """Which family forms a convolution backward's data gradient: a fused one, "stride1" (``_plan_dgrad``), "strided"
    (``_plan_dgrad_strided``) or "aten". Launches and allocates nothing. A fused family is ``fused_candidate``'s
    (``dw_ok``: the weight gradient is still to be formed, into an fp32 slot) where the backward's own facts hold too:
      "fused_1x1"    both gradients and the input BatchNorm + ReLU's backward sums in one pass over gy and x
                     (bwd1x1_fused.hip): no addend, the relu-kind link filled for this very x; ``bwd1x1_fused_on()``
      "fused_final"  that kernel's final form, the second data gradient into x (ResNet's stage-1 downsample
                     convolution): it accumulates onto the contiguous tensor ``addend`` and takes the pool-kind link's
                     sums, the contract of ``_plan_dgrad``'s "tile_final_sums"; ``dual_onload_on()``
      "conv1_fused"  both gradients, a mask-kind link's sums and the apply pass of the BatchNorm + ReLU reading the
                     output (conv1_fused.hip; an identity bottleneck's conv1 in stages 1-2 behind another identity
                     block): ``apply_link`` is that BatchNorm's relu-kind ``nn.ApplyLink`` covering ``gy``, the addend
                     masked, and the data gradient's own route takes the sums ("short_mask_sums": the switches that
                     turn those sums off turn this family off with them); ``conv1_fused_on()``
    The first two also apply a mask- or dual-kind link on load, which is ``conv_bwd``'s to decide."""
    K, R, S, C = w.shape
    family = fused_candidate(C_, x, w, stride, padding, _link_kind(bn_link, x.shape), dw_ok, xform is not None)
    masked = addend is not None and not torch.is_tensor(addend)
    if (family == "conv1_fused" and apply_link is not None and apply_link.kind == "relu" and apply_link.covers(gy)
            and masked and conv1_fused_on() and _hip(gy, addend.dy) and gy.is_contiguous()
            and addend.dy.is_contiguous() and addend.dy.shape == x.shape and apply_link.x.shape == gy.shape
            and C_.gemm_short_bnstats_ok(x.numel() // C, C, K, False)):
        return family
    if (family == "fused_final" and torch.is_tensor(addend) and addend.is_contiguous() and addend.shape == x.shape
            and dual_onload_on() and _hip(gy, addend) and gy.is_contiguous()):
        return family
    if (family == "fused_1x1" and addend is None and bwd1x1_fused_on() and bn_link.x.data_ptr() == x.data_ptr()
            and gy.is_contiguous()):
        return family
    if _hip(gy, x, w) and stride == 1 and K % 8 == 0 and C % 8 == 0:
        return "stride1"
    if _hip(gy, x, w) and strided_dgrad_ok(gy, w, stride, padding):
        return "strided"
    return "aten"


def _slot_written(p):
    """A kernel wrote (``p.written`` was False when it was launched) or accumulated into ``p``'s flat gradient slot."""
    p.store._notify(p) if p.written else p.store.mark_written(p)


def _finish_dw(p, gy, x, w, stride, padding):
    """The weight gradient our kernels did not take (``p`` still set): ATen's, deposited."""
    if p is not None:
        _vendor("wgrad", x, w, stride, padding)
        _, dw = _aten_bwd(gy, x, w, stride, padding, False, True)
        p.store.deposit(p, dw)


def _fused_bwd(C_, family, gy, x, w, padding, addend, xform, ln, p, apply_link):
    """A fused family's one launch: dw into ``p``'s slot, the data gradient with the sums of the BnStatLink ``ln``
    deposited, and ``apply_link``'s BatchNorm backward applied as gy is loaded. Returns the data gradient."""
    K, _, _, C = w.shape
    STATS["hip_wgrad"] += 1
    STATS["hip_dgrad"] += 1
    sums = _bn_sums(C_, ln, C, gy.device)
    gy2, x2, w2, dw = gy.view(-1, K), x.view(-1, C), w.view(K, C), p.grad.view(K, C)
    onload = {} if apply_link is None else {"x3": apply_link.x.view(-1, K), "mask": apply_link.mask,
                                            "params": apply_link.params}
    if family == "conv1_fused":
        ROUTES[_plan_dgrad(C_, gy, w, padding, addend, ln)] += 1  # the data gradient's contract: short_mask_sums
        STATS["conv1_fused"] += 1
        dx = C_.conv1_fused(gy2, onload["x3"], onload["params"], w2, x2, addend.dy.view(-1, C), addend.mask,
                            ln.x.view(-1, C), ln.mask, ln.mean, sums, dw, p.written).view(x.shape)
    elif family == "fused_final":
        ROUTES[_plan_dgrad(C_, gy, w, padding, addend, ln)] += 1  # the data gradient's contract: tile_final_sums
        STATS["fused_final"] += 1
        C_.bwd1x1_fused(gy2, x2, w2, None, None, None, None, None, dw, sums, p.written, addend=addend.view(-1, C),
                        winner_x=ln.x.view(-1, C), winner_bits=ln.mask.view(-1), winner_mean=ln.mean, **onload)
        dx = addend
    else:
        ROUTES[family] += 1
        STATS["bn3_onload"] += apply_link is not None
        dx = C_.bwd1x1_fused(gy2, x2, w2, xform, ln.gamma, ln.beta, ln.mean, ln.invstd, dw, sums, p.written,
                             **onload).view(x.shape)
    _slot_written(p)
    ln.deposit(sums, None, dx)
    return dx


def conv_bwd(gy, x, w, stride, padding, need_dx, p=None, addend=None, xform=None, x_sub=None, bn_link=None,
             apply_link=None):
    """Returns dx (+ ``addend``, e.g. the residual branch's gradient of the same tensor, fused into the
    dgrad epilogue where our kernel runs) or None; deposits dw into ``p``'s flat gradient slot. ``xform``: the
    convolution's input is relu(bn(x)) normalised on load (see ``_wgrad_hip``); dx is then the gradient w.r.t.
    that normalised input. ``x_sub``: a 1x1 / pad-0 convolution's input already subsampled by its stride
    (``nn._Conv2dNHWC`` with ``subsample_ok``): the weight gradient runs as the stride-1 product on it; ``x`` then only gives dx's shape.
    ``apply_link``: a filled ``nn.ApplyLink`` -- the BatchNorm that read this convolution's output deferred its apply
    pass, so ``gy`` is that BatchNorm's incoming dy and not yet the gradient of the output. The link is kept, and
    applied as the kernel loads gy, when the planned family is one its kind can go to (``nn.APPLY_KINDS``) and it
    covers ``gy``; in every other case the apply pass runs here first, on the ``gy`` received, counted under the
    kind's ``apply_stat``."""
    from k8s_amd.ops.nn import APPLY_KINDS

    K, R, S, C = w.shape
    C_ = _load() if gy.is_cuda else None
    dw_ok = p is not None and x_sub is None and p.grad.dtype == torch.float32
    hip = _hip(gy, x, w)
    if addend is not None and not torch.is_tensor(addend) and not (
            hip and stride == 1 and K % 8 == 0 and C % 8 == 0):
        addend = addend.materialize()  # only the stride-1 dgrad on our kernels takes the (dy, mask) pair

    def plan():
        return _plan_bwd(C_, gy, x, w, stride, padding, addend, xform, bn_link, dw_ok, apply_link) if need_dx else None

    family = plan()
    if apply_link is not None:
        kind = APPLY_KINDS[apply_link.kind]
        if not (family in kind.families and apply_link.covers(gy)):
            STATS[kind.apply_stat] += 1
            gy = C_.bn_bwd_apply(gy.contiguous(), apply_link.x, apply_link.mask, apply_link.params)
            apply_link = None
            family = plan()
    if x_sub is not None:
        _wgrad_hip(C_, gy, x_sub, p.grad.view(p.shape), 1, 0, p.written)
        STATS["hip_wgrad"] += 1
        _slot_written(p)
        p = None  # done
    if xform is not None and not (hip and C % 64 == 0 and K % 8 == 0 and p is not None
                                  and p.grad.dtype == torch.float32):
        raise RuntimeError("normalize-on-load weight gradient outside the kernels' contract")
    if family in ("fused_1x1", "fused_final", "conv1_fused"):
        return _fused_bwd(C_, family, gy, x, w, padding, addend, xform, bn_link, p, apply_link)
    # ---- weight gradient
    if hip and C % 8 == 0 and K % 8 == 0 and p is not None and p.grad.dtype == torch.float32:
        STATS["hip_wgrad"] += 1
        _wgrad_hip(C_, gy, x, p.grad.view(p.shape), stride, padding, p.written, xform)
        _slot_written(p)
        p = None  # done
    # ---- data gradient
    dx = None
    if family in ("stride1", "strided"):
        STATS["hip_dgrad"] += 1
        if family == "stride1":
            dx = _dgrad_hip(C_, gy, w, padding, addend, bn_link)
        else:
            dx = _dgrad_strided_hip(C_, gy, w, stride, padding, x.shape[1], x.shape[2], addend, bn_link)
    elif family == "aten":
        ROUTES[family] += 1
        _vendor("dgrad", x, w, stride, padding)
        dx, _ = _aten_bwd(gy, x, w, stride, padding, True, False)
        if addend is not None:
            dx = dx + addend
    _finish_dw(p, gy, x, w, stride, padding)
    return dx


# 1x1 / stride-2 / pad-0 convolutions (ResNet's downsample branch) as stride-1 GEMMs on the subsampled input: one
# subsample pass (pool.hip), then the forward (with the BN statistics, the 4-wave / short-K kernels) and the weight
# gradient take the plain-GEMM paths instead of the strided implicit-GEMM gather; the data gradient keeps the
# strided parity path (it accumulates onto the block input's other gradient). K8S_AMD_SUB1X1=0 for the A/B.
SUB1X1 = os.environ.get("K8S_AMD_SUB1X1", "1") != "0"


def subsample_ok(x, w, stride, padding) -> bool:
    K, R, S, C = w.shape
    return (SUB1X1 and stride > 1 and R == 1 and S == 1 and padding == 0 and _hip(x, w) and C % 64 == 0
            and K % 8 == 0 and x.is_contiguous())
