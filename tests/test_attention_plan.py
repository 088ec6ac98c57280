"""flash_plan pinned: which attention kernels run for a shape, and which calls the flash kernels do not take.

One row per distinct route, with 256 compute units planned for (an MI355X). No GPU is needed: the plan is a pure
host function. The last column of each table names the GPU test that launches the route:
  A   tests/test_attention_gpu.py::test_flash_fwd_bwd            AR  ...::test_flash_fwd_bwd_routes
  Dr  tests/test_dropout_gpu.py::test_attention_dropout_fwd_bwd  DL  tests/test_dropout_long_gpu.py (LONG_CASES)
  Dc  tests/test_doc_mask_gpu.py::test_flash_doc_fwd_bwd         U   tests/test_unpad_gpu.py::test_flash_span_fwd_bwd
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

    C_.set_planner_cus(256)
    yield C_
    C_.set_planner_cus(0)


def _plan(C, mask, D, Sq, Sk=None, B=2, Hq=4, Hkv=None, causal=None, **kw):
    causal = mask == "doc" if causal is None else causal
    return C.flash_plan(D, B, Sq, Sq if Sk is None else Sk, Hq, Hq if Hkv is None else Hkv, causal=causal, mask=mask,
                        **kw)


# mask, D, Sq, Sk, extra, (tile, nb) or None for a call the kernels do not take
FWD = [
    ("plain", 128, 192, 192, {}, (64, 2)),                        # A  (2, 192, 4, 4, 128)
    ("plain", 64, 128, 128, {}, (128, 1)),                        # A  (2, 128, 12, 12, 64)
    ("plain", 64, 192, 192, {}, (64, 2)),                         # A  (2, 200, 4, 4, 64)
    ("plain", 64, 1024, 1024, {}, (128, 2)),                      # A  (2, 1024, 2, 2, 64)
    ("plain", 64, 1024, 128, {}, (128, 1)),                       # AR cross: the forward picks its tile by Sk
    ("drop", 64, 128, 128, {}, (128, 1)),                         # Dr (2, 128, 2)
    ("drop", 64, 192, 192, {}, (64, 2)),                          # DL (1, 192, 192, 2, 2)
    ("drop", 64, 1024, 1024, {}, (128, 2)),                       # DL (1, 1024, 1024, 1, 1)
    ("drop", 128, 256, 256, {}, None),
    ("drop", 64, 200, 200, {}, None),
    ("drop", 64, 100, 100, {}, (128, 1)),                         # Dr (2, 100, 4): one-block backward
    ("drop", 64, 100, 100, {"Hkv": 2}, None),
    ("doc", 64, 128, 128, {}, (64, 2)),                           # Dc (2, 96, 2, 2, 64): never the one-tile forward
    ("doc", 64, 1024, 1024, {}, (128, 2)),                        # Dc (1, 1152, 2, 2, 64)
    ("doc", 128, 128, 128, {}, (64, 2)),                          # Dc (1, 320, 4, 1, 128)
    ("doc", 128, 2048, 2048, {}, (64, 2)),
    ("span", 64, 128, 128, {}, (64, 2)),                          # U  (2, 192, 4, 2)
    ("span", 64, 1152, 1152, {}, (64, 2)),                        # U  (1, 1152, 2, 2)
    ("span", 64, 1152, 1152, {"span_tile": 64}, (64, 2)),         # U  tile 64 by name
    ("span", 64, 1152, 1152, {"span_tile": 128}, (128, 2)),       # U  tile 128
    ("span", 128, 128, 128, {}, None),
    ("span", 64, 128, 128, {"max_token_stride": 1 << 24}, None),
    ("span", 64, 128, 128, {"span_tile": 32}, None),
    ("span", 64, 128, 128, {"causal": True}, None),
    ("span", 64, 128, 128, {"has_kv_lens": True}, None),
    ("span", 64, 128, 64, {}, None),
    ("doc", 64, 128, 128, {"causal": False}, None),
    ("doc", 64, 128, 128, {"has_kv_lens": True}, None),
    ("doc", 64, 128, 64, {}, None),
    ("plain", 64, 128, 128, {"span_tile": 64}, None),
]


@pytest.mark.parametrize("mask,D,Sq,Sk,kw,want", FWD)
def test_forward_plan(C, mask, D, Sq, Sk, kw, want):
    p = _plan(C, mask, D, Sq, Sk, **kw)
    assert p["ok"] == (want is not None), p
    if want is None:
        assert p["reason"]
    else:
        assert (p["fwd"]["tile"], p["fwd"]["nb"]) == want and p["reason"] == ""


THREE = dict(one_block=False)
# mask, D, B, Sq, Sk, Hq, Hkv, causal, the fields of plan["bwd"] that the row pins
BWD = [
    ("plain", 64, 2, 128, 128, 4, 4, False, dict(one_block=True, dkv_split=1, needs_rowkey=False)),       # A
    ("plain", 64, 2, 128, 128, 4, 2, False, dict(THREE, tile=64, qs=1)),                   # A  (2, 128, 4, 2, 64)
    ("plain", 64, 64, 192, 192, 12, 12, False, dict(THREE, tile=64, qs=2)),                # AR with 2 CUs planned
    ("plain", 64, 2, 192, 192, 2, 2, False, dict(THREE, tile=64, qs=1)),                   # A  (2, 200, 4, 4, 64)
    ("plain", 64, 2, 1024, 1024, 2, 2, False, dict(THREE, tile=128, qs=1, dkv_split=1)),   # A  (2, 1024, 2, 2, 64)
    ("plain", 64, 64, 1024, 1024, 12, 12, False, dict(THREE, tile=128, qs=1)),             # (no QS = 2 on 128-wide tiles)
    ("plain", 64, 2, 1024, 128, 4, 4, False, dict(THREE, tile=128, qs=1)),                 # AR: the backward picks by Sq
    ("plain", 128, 2, 192, 192, 4, 4, False, dict(THREE, tile=64, qs=1)),                  # A  (2, 192, 4, 4, 128)
    ("plain", 128, 64, 192, 192, 12, 12, False, dict(THREE, tile=64, qs=1)),
    ("plain", 64, 1, 1024, 1024, 4, 2, True, dict(THREE, dkv_split=4)),                    # A  (1, 1100, 4, 2, 64)
    ("plain", 64, 8, 1024, 1024, 8, 4, True, dict(THREE, dkv_split=2)),                    # A  (1, 4096, 32, 8, 128)
    ("plain", 64, 16, 1024, 1024, 16, 16, True, dict(THREE, dkv_split=1)),                 # AR with 4 CUs planned
    ("plain", 128, 1, 256, 256, 8, 2, True, dict(THREE, dkv_split=1)),                     # A  (1, 256, 8, 2, 128)
    ("plain", 64, 1, 4096, 4096, 4, 2, False, dict(THREE, dkv_split=1)),                   # A  (1, 2048, 12, 12, 64)
    ("drop", 64, 2, 100, 100, 4, 4, False, dict(one_block=True, needs_rowkey=False)),      # Dr (2, 100, 4)
    ("drop", 64, 2, 128, 128, 4, 2, False, dict(THREE, tile=64, qs=1, needs_rowkey=True)),  # DL (2, 128, 128, 4, 2)
    ("drop", 64, 32, 256, 256, 8, 8, False, dict(THREE, tile=64, qs=2, needs_rowkey=True)),  # DL (32, 256, 256, 8, 8)
    ("drop", 64, 1, 1024, 1024, 1, 1, False, dict(THREE, tile=128, qs=1, needs_rowkey=True)),  # DL (1, 1024, 1024, 1, 1)
    ("drop", 64, 1, 512, 512, 2, 2, True, dict(THREE, dkv_split=4, needs_rowkey=True)),    # DL (1, 512, 512, 2, 2)
    ("doc", 64, 2, 128, 128, 4, 4, True, dict(THREE, tile=64, qs=1, dkv_split=1)),         # Dc (2, 96, 2, 2, 64)
    ("doc", 64, 64, 192, 192, 12, 12, True, dict(THREE, tile=64, qs=1)),                   # (never QS = 2)
    ("doc", 64, 1, 1024, 1024, 4, 2, True, dict(THREE, tile=128, qs=1, dkv_split=4)),      # Dc (1, 1152, 2, 2, 64)
    ("doc", 128, 8, 1024, 1024, 8, 4, True, dict(THREE, tile=64, qs=1, dkv_split=2)),
    ("doc", 128, 1, 320, 320, 4, 1, True, dict(THREE, tile=64, qs=1, dkv_split=1)),        # Dc (1, 320, 4, 1, 128)
    ("span", 64, 2, 128, 128, 4, 4, False, dict(THREE, tile=64, qs=1, dkv_split=1)),       # U  (2, 192, 4, 2)
    ("span", 64, 64, 192, 192, 12, 12, False, dict(THREE, tile=64, qs=1, dkv_split=1)),    # (never QS = 2)
    ("span", 64, 1, 1152, 1152, 2, 2, False, dict(THREE, tile=64, qs=1, dkv_split=1)),     # U  (1, 1152, 2, 2)
]


@pytest.mark.parametrize("mask,D,B,Sq,Sk,Hq,Hkv,causal,want", BWD)
def test_backward_plan(C, mask, D, B, Sq, Sk, Hq, Hkv, causal, want):
    p = C.flash_plan(D, B, Sq, Sk, Hq, Hkv, causal=causal, mask=mask)
    assert p["ok"] and p["reason"] == "", p
    assert {k: p["bwd"][k] for k in want} == want, p
    if mask != "drop":
        assert not p["bwd"]["needs_rowkey"]
    else:  # the row-key table exactly when the three kernels run
        assert p["bwd"]["needs_rowkey"] == (not p["bwd"]["one_block"])
    if mask == "doc":  # dK/dV chunks as the causal plain call's
        assert p["bwd"]["dkv_split"] == C.flash_plan(D, B, Sq, Sk, Hq, Hkv, causal=True)["bwd"]["dkv_split"]


def test_span_tile_128_backward(C):
    p = _plan(C, "span", 64, 1152, B=1, Hq=2, span_tile=128)
    assert p["ok"] and p["bwd"] == dict(one_block=False, tile=128, qs=1, dkv_split=1, needs_rowkey=False)  # U tile 128


@pytest.mark.parametrize("mask,D,S,Hkv,ok", [
    ("plain", 64, 128, 4, True), ("drop", 64, 100, 4, True),      # one-block shapes
    ("doc", 64, 128, 4, False), ("span", 64, 128, 4, False),      # a table mask has no one-block form
    ("plain", 64, 128, 2, False), ("plain", 64, 192, 4, False), ("plain", 128, 128, 4, False),
    ("drop", 64, 256, 4, False)])
def test_bias_gradient_needs_the_one_block_backward(C, mask, D, S, Hkv, ok):
    p = _plan(C, mask, D, S, Hkv=Hkv, want_dbias=True)
    assert p["ok"] == ok and bool(p["reason"]) == (not ok), p
    assert _plan(C, mask, D, S, Hkv=Hkv)["ok"]  # (the same call without the bias gradient is taken)


def test_old_predicates_are_views_of_the_plan(C):
    for mask, D, B, Sq, Sk, Hq, Hkv, causal, _ in BWD:
        p = C.flash_plan(D, B, Sq, Sk, Hq, Hkv, causal=causal)  # (the predicates know no mask kind)
        assert C.flash_bwd_one_block(D, Sq, Sk, Hq, Hkv, causal, B) == p["bwd"]["one_block"]
        assert C.flash_dkv_splits(B, Sq, Sk, Hkv, causal) == p["bwd"]["dkv_split"]
        assert C.flash_dropout_fused(D, Sq, Sk, Hq, Hkv, causal, B) == \
            C.flash_plan(D, B, Sq, Sk, Hq, Hkv, causal=causal, mask="drop")["ok"]
    for mask, D, Sq, Sk, kw, want in FWD:
        if mask == "drop" and not kw:
            assert C.flash_dropout_fused(D, Sq, Sk, 4, 4, False, 2) == (want is not None)
        if mask == "span" and set(kw) <= {"max_token_stride"}:
            stride = kw.get("max_token_stride", 768)
            assert C.flash_span_ok(D, 2, Sq, Sk, 4, stride) == (want is not None)
    assert C.flash_span_tile(128) == C.flash_span_tile(1152) == _plan(C, "span", 64, 1152)["fwd"]["tile"] == 64
    assert not C.flash_span_ok(64, 1, 1 << 24, 1 << 24, 1, 768)
    assert not C.flash_span_ok(64, 1 << 10, 1 << 12, 1 << 12, 1 << 9, 768)
    assert C.flash_span_ok(64, 1, 131072, 131072, 12, 2304)


def test_the_plan_follows_the_planned_compute_units(C):
    args = (64, 1, 192, 192, 2, 2)
    assert C.flash_plan(*args)["bwd"]["qs"] == 1
    C.set_planner_cus(2)
    try:
        assert C.flash_plan(*args)["bwd"]["qs"] == 2
        assert C.flash_plan(64, 1, 512, 512, 2, 2, causal=True)["bwd"]["dkv_split"] == 1
    finally:
        C.set_planner_cus(256)
