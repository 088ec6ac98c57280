"""The fused augmentation kernel, the loader's two modes and training on a dataset, on the GPU.

The oracle is ``ops.reference.augment`` (float64, one fp32 and one bf16 rounding): copy rows must match it bit for bit,
resized rows within one bf16 step (the kernel interpolates in fp32, whose error is far below half a bf16 step, so the
two roundings can differ by at most one)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _norm():
    from k8s_amd.ops import data as kdata

    return kdata.norm_constants([125.3, 123.0, 113.9], [63.0, 62.1, 66.7])


def _src(M, Hs, Ws, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (M, Hs, Ws, 3), generator=g, dtype=torch.uint8)


def _bits(t):
    return t.cpu().contiguous().view(torch.int16)


def _ordered(t):
    """bf16 -> integers in value order (adjacent representable values differ by 1; +0 and -0 coincide)."""
    i = _bits(t).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from k8s_amd.tools.make_dataset import make_toy

    path = str(tmp_path_factory.mktemp("toy"))
    make_toy(path)
    return path


# ------------------------------------------------------------------------------------------------ copy rows
COPY_ROWS = [  # 5 sources of 12 x 10, S = 8: repeated and descending indices, offsets -3 and Hs-S+3, both flips
    (4, 0, 0, 8, 8, 0), (4, -3, -3, 8, 8, 1), (3, 7, 5, 8, 8, 0), (2, 7, -3, 8, 8, 1), (2, -3, 5, 8, 8, 0),
    (0, 2, 1, 8, 8, 1), (0, 4, 2, 8, 8, 0)]


@pytest.mark.parametrize("layout", ["nhwc8", "s2d"])
def test_copy_rows_bit_exact(cuda, layout):
    from k8s_amd.ops import data as kdata
    from k8s_amd.ops import reference as ref

    src, (a, b) = _src(5, 12, 10, 1), _norm()
    table = torch.tensor(COPY_ROWS, dtype=torch.int32)
    assert table[:, 1].max() == 12 - 8 + 3 and table[:, 2].max() == 10 - 8 + 3 and table[:, 1:3].min() == -3
    got = kdata.augment(src.to(cuda), table, a, b, 8, layout)
    want = ref.augment(src, table, a, b, 8, layout)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == ((7, 8, 8, 8) if layout == "nhwc8" else (7, 7, 7, 16))
    assert torch.equal(_bits(got), _bits(want))
    if layout == "s2d":  # the stem's padding of 3: the outer ring of the 7 x 7 s2d image holds no source pixel
        g = got.cpu().float()
        assert g[:, 0].abs().max() == 0 and g[:, 6].abs().max() == 0
        assert g[:, :, 0].abs().max() == 0 and g[:, :, 6].abs().max() == 0
        assert g[:, 1:6, 1:6].abs().max() > 0
    else:
        assert got[..., 3:].float().abs().max() == 0


@pytest.mark.parametrize("S,N,Hs", [(32, 3, 32), (224, 2, 256)])
def test_s2d_layout_is_stem_s2d_input_of_nhwc8(cuda, S, N, Hs):
    from k8s_amd.data import sampler
    from k8s_amd.ops import data as kdata
    from k8s_amd.ops import nn as K

    src, (a, b) = _src(N + 1, Hs, Hs, 2).to(cuda), _norm()
    idx = np.arange(N, 0, -1)
    table = sampler.train_table(idx, 3, 0, 0, Hs, Hs, S, "rrc" if Hs != S else "crop", 4)
    if Hs != S:
        table[0, 1:5] = (Hs - S + 3, -3, S, S)  # a copy row that hangs over two edges among the resized ones
    table = torch.from_numpy(table)
    x8 = kdata.augment(src, table, a, b, S, "nhwc8")
    xs = kdata.augment(src, table, a, b, S, "s2d")
    assert tuple(xs.shape) == (N, S // 2 + 3, S // 2 + 3, 16)
    assert torch.equal(_bits(xs), _bits(K.stem_s2d_input(x8, 3)))


# ------------------------------------------------------------------------------------------------ resized rows
def _resize_rows(Hs, Ws, S):
    rows = [(0, 2 % Hs, 1 % Ws, 1, 1, 0), (1, 0, 0, Hs, Ws, 1), (2, 0, Ws - 3, Hs, 3, 0), (1, 1, 1, 3, 2, 1),
            (0, 0, 0, Hs, Ws - 1, 0), (2, Hs - 4, 0, 4, Ws, 1),
            # copy rows (h == w == S) in the same call: they stay bit-exact
            (1, -1, 0, S, S, 1), (2, 0, -2, S, S, 0)]
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("Hs,Ws", [(40, 36), (5, 5)])
@pytest.mark.parametrize("S", [8, 32])
@pytest.mark.parametrize("layout", ["nhwc8", "s2d"])
def test_resized_rows_within_one_bf16_step(cuda, Hs, Ws, S, layout):
    from k8s_amd.ops import data as kdata
    from k8s_amd.ops import reference as ref

    src, (a, b) = _src(3, Hs, Ws, 5), _norm()
    table = _resize_rows(Hs, Ws, S)
    boxes = table[:6, 3:5].tolist()
    assert [1, 1] in boxes and [Hs, Ws] in boxes and [Hs, 3] in boxes  # 1x1, the whole source, a 3-wide strip
    assert any(h < S and w < S for h, w in boxes) and (Hs < S or any(h > S or w > S for h, w in boxes))
    assert set(table[:6, 5].tolist()) == {0, 1}
    got = kdata.augment(src.to(cuda), table, a, b, S, layout)
    want = ref.augment(src, table, a, b, S, layout)
    step = (_ordered(got) - _ordered(want)).abs()
    print("resized rows: max bf16 steps from the oracle %d, elements off by one %d of %d"
          % (int(step.max()), int((step == 1).sum()), step.numel()))
    assert int(step.max()) <= 1
    assert torch.equal(_bits(got[6:]), _bits(want[6:]))


# ------------------------------------------------------------------------------------------------ validation
GOOD = (1, 0, 0, 8, 8, 0)
BAD_ROWS = {"index below 0": (-1, 0, 0, 8, 8, 0), "index past M": (3, 0, 0, 8, 8, 0), "h of 0": (0, 0, 0, 0, 8, 0),
            "w of 0": (0, 0, 0, 8, 0, 1), "negative w": (0, 0, 0, 4, -2, 0), "flip of 2": (0, 0, 0, 8, 8, 2),
            "resized box past the bottom": (0, 6, 0, 7, 4, 0), "resized box past the right": (0, 0, 8, 4, 4, 0),
            "resized box at a negative offset": (0, -1, 0, 4, 4, 0)}


@pytest.mark.parametrize("kind", sorted(BAD_ROWS))
def test_bad_table_row_raises_before_any_launch(cuda, kind):
    from k8s_amd.ops import data as kdata

    src, (a, b) = _src(3, 12, 10, 7).to(cuda), _norm()
    table = torch.tensor([GOOD, BAD_ROWS[kind], GOOD], dtype=torch.int32)
    before = kdata.launches()
    with pytest.raises(RuntimeError, match="table row 1"):
        kdata.augment(src, table, a, b, 8, "s2d")
    assert kdata.launches() == before


def test_bad_arguments_raise_before_any_launch(cuda):
    from k8s_amd.ops import data as kdata

    src, (a, b) = _src(3, 12, 10, 7).to(cuda), _norm()
    table = torch.tensor([GOOD, GOOD], dtype=torch.int32)
    before = kdata.launches()
    bad = [
        (src.to(torch.int32), table, a, b, 8, "s2d"),            # a non-uint8 source
        (src, table.to(cuda), a, b, 8, "s2d"),                   # a device-resident table
        (src, table.long(), a, b, 8, "s2d"),                     # table dtype
        (src, table[:, :5].contiguous(), a, b, 8, "s2d"),        # table shape
        (src, table, a, b, 7, "s2d"),                            # odd S for the space-to-depth layout
        (src, table, a, b, 8, "nchw"),                           # unknown layout
        (src[..., :2].contiguous(), table, a, b, 8, "nhwc8"),    # not 3 channels
        (src, table, a[:2], b, 8, "nhwc8"),                      # two normalisation values
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            kdata.augment(*args)
    assert kdata.launches() == before
    kdata.augment(src, table, a, b, 8, "s2d")
    assert kdata.launches() == before + 1


# ------------------------------------------------------------------------------------------------ loader
def test_loader_resident_and_streamed_give_the_same_bits(cuda, toy):
    from k8s_amd.data import open_dataset
    from k8s_amd.data.loader import Loader
    from k8s_amd.ops import reference as ref

    ds = open_dataset(toy)
    res = Loader(ds, "train", cuda, 16, image=32, seed=3, resident_gb=4.0)
    stm = Loader(ds, "train", cuda, 16, image=32, seed=3, resident_gb=0.0)
    try:
        assert res.resident and not stm.resident and stm.streamer is not None
        E = res.steps_per_epoch
        assert E == 2048 // 16
        images = torch.from_numpy(np.array(ds.split("train").images))
        for t in (0, E - 1, E, 2):
            (xr, yr), (xs, ys) = res.batch(t), stm.batch(t)
            idx, labels = res.rows(t)
            want = ref.augment(images, torch.from_numpy(res.table(t, idx)), res.a, res.b, 32, "s2d")
            assert torch.equal(_bits(xr), _bits(want)), "resident batch %d differs from the reference" % t
            assert torch.equal(_bits(xs), _bits(xr)), "streamed batch %d differs from the resident one" % t
            assert torch.equal(yr.cpu(), torch.from_numpy(labels)) and torch.equal(ys, yr)
        assert stm.streamer.restarts == 2  # at E-1 and at 2: 1 and E+1 had been prefetched; E was the prefetch
    finally:
        res.close()
        stm.close()


def test_model_takes_the_s2d_batch(cuda, toy):
    from k8s_amd.models.registry import build
    from k8s_amd.ops import conv as kconv
    from k8s_amd.parallel.ddp import GradReducer

    w = build("resnet_tiny", cuda, 4, image=32, data={"dir": toy})
    try:
        x, y = w.batch(0)
        assert tuple(x.shape) == (4, 19, 19, 16) and x.dtype == torch.bfloat16 and y.dtype == torch.int64
        assert w.meta["classes"] == 10
        before = kconv.STATS["hip_fwd"]
        GradReducer(w.store, enabled=False).begin_step()
        loss = w.loss((x, y))
        assert torch.isfinite(loss.detach().float()).item()
        assert kconv.STATS["hip_fwd"] > before
        loss.backward()
        torch.cuda.synchronize()
        sums = w.evaluate(w.eval_batch(15, 32))  # val has 256 images: batch 15 of 32 holds none
        assert int(sums["count"]) == 0
        assert int(w.evaluate(w.eval_batch(7, 32))["count"]) == 32
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------ learning
# top-1 on the 256 val images after 120 steps through the trainer on an MI355X (bf16), seeds 0, 1, 2: 1.00, 1.00, 1.00
# (the trainer's default crop keeps the whole 40 x 40 source in view, so the toy set is learnt completely; the fp32 CPU
# runs measure the same). Chance is 0.10; the threshold lies halfway between chance and the lowest of the three.
GPU_TOP1 = (1.0, 1.0, 1.0)
GPU_THRESHOLD = (0.10 + min(GPU_TOP1)) / 2


def test_trainer_learns_the_toy_set_on_the_gpu(cuda, toy):
    r = subprocess.run([sys.executable, "-m", "k8s_amd.trainer", "--model", "resnet_tiny", "--device", "cuda",
                        "--data-dir", toy, "--batch", "32", "--lr", "0.02", "--steps", "120", "--eval-every", "120",
                        "--eval-batches", "8"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    events = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    ev = [e for e in events if e.get("event") == "eval"][-1]
    done = [e for e in events if e.get("event") == "done"][-1]
    print("gpu toy top1 %.4f (examples %d)" % (ev["top1"], ev["examples"]))
    assert ev["examples"] == 256
    assert done["gemm_fallbacks"] == {}
    assert ev["top1"] > GPU_THRESHOLD
