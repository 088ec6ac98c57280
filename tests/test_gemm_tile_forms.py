"""gemm_tile_form pinned: which form of the tile kernel (gemm.hip TileEpi, "+A" / "+B" with an operand normalized on
load) a launch takes, and which launches the chooser refuses.

One row per distinct route -- each legal (operand pair, tile, kind, on-load), the kernel's 38 instantiations (x single
/ double buffer) -- and the three refusals. No GPU is needed: the chooser is a pure host function. The last column of
a row names a GPU test that launches the route (recorded by logging the route of every launch of the GPU suite):
  G   tests/test_gemm_conv_gpu.py            I   tests/test_infer_gpu.py
  W   tests/test_gemm256_gpu.py              T   tests/test_gemm_tile_routes_gpu.py
"-" marks an instantiation that no entry point of launchers.h reaches (kept: the instantiation set is the kernel's).
"""
import glob
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def C():
    if not glob.glob(os.path.join(ROOT, "k8s_amd", "_C*.so")):
        pytest.skip("extension not built here (python -m k8s_amd._build)")
    import k8s_amd._C as C_

    return C_


def _form(C, pair, wm, kw):
    return C.gemm_tile_form(pair, wm=wm, N=kw.pop("N", 64 if wm == 4 else 128), **kw)


F32 = dict(out_f32=True)
SUB_MASK = dict(bb_sums=True, bb_mask=True, rst=True, mode=1)   # a 1x1 parity's correction of a residual BN's sums
SUB_RELU = dict(bb_sums=True, rst=True)                         # a stride-2 parity storing with a BN + ReLU's sums
NORM, AFFINE = dict(xuse=1), dict(xuse=2)

# pair, wm (2: 128 x 128 tiles, 4: 256 x 64), what describes the Epi, the form, the GPU test that launches it
ROUTES = [
    ("KK", 2, F32, "General", "G::test_gemm_layouts[True-True-256-256-64]"),
    ("KK", 2, {}, "Lean", "G::test_gemm_layouts[True-True-256-256-64]"),
    ("KK", 2, dict(bias=True, act=2, pre=True), "LeanLinear", "G::test_gemm_epilogue[True-512-768-768-0]"),
    ("KK", 2, SUB_MASK, "LeanBnBwd", "G::test_stage_entry_bn_sums_two_dgrads[4-16-128-256-512]"),
    ("KK", 2, AFFINE, "LeanInfer", "I::test_epilogue_against_fp32[case2-False-False]"),
    ("KK", 2, dict(NORM, stats=True), "Lean+A", "G::test_conv_fwd_normalize_on_load[case3]"),
    ("KK", 4, dict(N=4, ldc=4), "General", "W::test_linear_ragged_rows_and_columns_on_our_kernels[4-4]"),
    ("KK", 4, dict(mode=1, rst=True), "Lean", "G::test_conv_dgrad_strided_accumulate[2-15-64-128-3-2-1]"),
    ("KK", 4, dict(bias=True), "LeanLinear", "G::test_gemm_epilogue[True-40-64-64-0]"),
    ("KK", 4, AFFINE, "LeanInfer", "I::test_epilogue_against_fp32[case8-False-False]"),
    ("KK", 4, NORM, "Lean+A", "G::test_conv_fwd_normalize_on_load[case5]"),
    ("KM", 2, F32, "General", "G::test_gemm_layouts[True-False-256-256-64]"),
    ("KM", 2, {}, "Lean", "G::test_gemm_layouts[True-False-1000-520-192]"),
    ("KM", 2, dict(bb_sums=True), "LeanBnBwd", "G::test_gemm_dgrad_bnstats_epilogue[9000-256-64]"),
    ("MK", 2, F32, "General", "G::test_gemm_layouts[False-True-256-256-64]"),
    ("MK", 2, {}, "Lean", "G::test_gemm_layouts[False-True-256-256-64]"),
    ("MM", 2, dict(F32, bias=True), "General", "T::test_gemm_mn_major_pair_general_epilogue"),
    ("MM", 2, {}, "Lean", "G::test_gemm_layouts[False-False-256-256-64]"),
    ("MM", 2, F32, "F32Rows", "G::test_gemm_layouts[False-False-256-256-64]"),
    ("MM", 2, dict(F32, **NORM, mode=3, splits=2), "F32Rows+B", "G::test_conv_wgrad_normalize_on_load[case2]"),
    ("ConvK", 2, dict(F32, bias=True, act=1), "General", "T::test_conv_fwd_general_epilogue[128-1-2-0-19-136]"),
    ("ConvK", 2, {}, "Lean", "G::test_conv_fwd[case1]"),
    ("ConvK", 2, SUB_RELU, "LeanBnBwd", "G::test_strided_dgrad_bn_relu_sums[4-28-128-128]"),
    ("ConvK", 2, AFFINE, "LeanInfer", "I::test_epilogue_against_fp32[case1-False-False]"),
    ("ConvK", 2, NORM, "Lean+A", "G::test_conv_fwd_normalize_on_load[case1]"),
    ("ConvK", 4, dict(F32, bias=True, act=1), "General", "T::test_conv_fwd_general_epilogue[64-3-1-1-10-64]"),
    ("ConvK", 4, {}, "Lean", "G::test_conv_fwd[case0]"),
    ("ConvK", 4, AFFINE, "LeanInfer", "I::test_epilogue_against_fp32[case0-False-False]"),
    ("ConvK", 4, NORM, "Lean+A", "G::test_conv_fwd_normalize_on_load[case0]"),
    ("ConvGK", 2, dict(F32, bias=True, act=1), "General", "T::test_conv_fwd_general_epilogue[144-2-1-0-11-136]"),
    ("ConvGK", 2, {}, "Lean", "I::test_forward_infer_resnet_tiny"),
    ("ConvGK", 2, AFFINE, "LeanInfer", "I::test_epilogue_against_fp32[case12-False-False]"),
    ("ConvGK", 4, dict(F32, bias=True, act=1), "General", "T::test_conv_fwd_general_epilogue[32-2-1-0-11-64]"),
    ("ConvGK", 4, {}, "Lean", "G::test_conv_fwd[case5]"),
    ("ConvGK", 4, AFFINE, "LeanInfer", "I::test_epilogue_against_fp32[case5-False-False]"),
    ("MWg", 2, dict(F32, stats=True), "General", "-"),  # launch_conv_wgrad only ever describes F32Rows' Epi
    ("MWg", 2, dict(F32, mode=3, splits=2), "F32Rows", "G::test_conv_wgrad[case0]"),
    ("MWg", 2, dict(F32, **NORM), "F32Rows+B", "G::test_conv_wgrad_normalize_on_load[case0]"),
]


@pytest.mark.parametrize("pair,wm,kw,want,gpu_test", ROUTES)
def test_route(C, pair, wm, kw, want, gpu_test):
    assert _form(C, pair, wm, dict(kw)) == want


def test_every_instantiation_has_a_row():
    assert len({(p, wm, want) for p, wm, _, want, _ in ROUTES}) == len(ROUTES) == 38


REFUSED = [
    ("KM", NORM, "normalize-on-load: no instantiation"),                       # no operand to transform in a dgrad
    ("MK", dict(SUB_RELU), "BatchNorm-backward sums epilogue"),
    ("KK", dict(F32, mode=1, addsrc=True), "a separate (masked) addend needs the lean epilogue"),
]


@pytest.mark.parametrize("pair,kw,msg", REFUSED)
def test_refused(C, pair, kw, msg):
    with pytest.raises(RuntimeError, match=msg.replace("(", r"\(").replace(")", r"\)")):
        _form(C, pair, 2, dict(kw))


def test_gates_read_in_one_place(C):
    """The edges of each kind's predicate (gemm.hip tile_epi_takes)."""
    f = lambda pair, **kw: _form(C, pair, kw.pop("wm", 2), kw)  # noqa: E731
    # Lean needs bf16 C in whole 16-B row chunks: ldc % 8, N % 8, an aligned base; else the General epilogue
    assert f("KK", N=132, ldc=132) == f("KK", ldc=132) == f("KK", c_aligned=False) == f("KK", mode=2) == "General"
    assert f("KK", mode=1) == f("KK", stats=True) == f("KK", rst=True) == f("KK", mode=1, addsrc=True) == "Lean"
    # LeanLinear: store mode, identity rows, no statistics, an aligned pre; only the K-major pair has it
    assert f("KK", bias=True) == f("KK", act=2, pre=True) == "LeanLinear"
    assert f("KK", bias=True, mode=1) == f("KK", bias=True, stats=True) == f("KK", pre=True, pre_aligned=False) \
        == f("KM", bias=True) == f("ConvK", bias=True) == "General"
    # F32Rows: the weight-gradient pairs with a plain fp32 output or slab; never atomics
    assert f("MM", **F32, mode=1) == f("MWg", **F32, mode=3, splits=2) == "F32Rows"
    assert f("MM", **F32, mode=2) == f("MM", **F32, bias=True) == f("MWg", **F32, stats=True) == f("KM", **F32) \
        == "General"
    # normalize on load: A with Lean on identity rows, B with F32Rows
    assert f("ConvK", **NORM, stats=True) == f("KK", **NORM, wm=4) == "Lean+A"
    assert f("MM", **F32, **NORM, mode=3, splits=2) == "F32Rows+B"
    for kw in (dict(rst=True), dict(mode=1, addsrc=True), dict(F32), dict(bias=True)):
        with pytest.raises(RuntimeError, match="normalize-on-load"):
            f("KK", **NORM, **kw)
    # LeanBnBwd: identity rows on the data-gradient pair (ldc == N; accumulate only for a mask-kind BatchNorm), sub-grid
    # rows on the convolution pairs (the mask kind's correction only on the K-major source); 2 x 2 tile, no split-K
    assert f("KM", bb_sums=True) == f("KM", bb_sums=True, bb_mask=True, mode=1, addsrc=True, addmask=True) == "LeanBnBwd"
    assert f("KK", **SUB_MASK) == f("KK", **SUB_RELU) == f("ConvK", **SUB_RELU) == "LeanBnBwd"
    for pair, kw in (("KM", dict(bb_sums=True, mode=1)), ("KM", dict(bb_sums=True, ldc=136)),
                     ("KM", dict(bb_sums=True, mode=1, bb_mask=True, addmask=True)), ("KM", dict(SUB_RELU)),
                     ("KK", dict(bb_sums=True)), ("ConvK", dict(SUB_MASK)), ("KK", dict(SUB_RELU, splits=2)),
                     ("KK", dict(SUB_RELU, wm=4)), ("ConvGK", dict(SUB_RELU)), ("KK", dict(SUB_RELU, addsrc=True))):
        with pytest.raises(RuntimeError, match="BatchNorm-backward sums epilogue"):
            f(pair, **kw)
    # the inference scale: the convolution pairs only
    assert f("ConvGK", **AFFINE, wm=4) == "LeanInfer"
    with pytest.raises(RuntimeError, match="inference epilogue"):
        f("KM", **AFFINE)
    with pytest.raises(RuntimeError, match="gemm_tile_form"):
        f("KX")
