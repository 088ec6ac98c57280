"""Training on a dataset, on the CPU: sampler, augmentation tables, the float64 oracle against an independent
composition, make_dataset, and the trainer's --data-dir path (configuration errors, exact resume, learning)."""
import json
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from k8s_amd.data import open_dataset, sampler
from k8s_amd.ops import data as kdata
from k8s_amd.ops import reference as ref
from k8s_amd.tools import make_dataset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("toy"))
    make_dataset.make_toy(path)
    return path


# ------------------------------------------------------------------------------------------------ sampler
def test_one_epoch_is_disjoint_over_ranks_and_covers_whole_batches():
    M, batch, world, seed = 203, 8, 3, 5
    E = sampler.steps_per_epoch(M, batch, world)
    assert E == 203 // 24
    for epoch in (0, 2):
        seen = np.concatenate([sampler.batch_indices(seed, epoch * E + t, r, world, batch, M)
                               for t in range(E) for r in range(world)])
        assert seen.size == E * batch * world == np.unique(seen).size
        assert seen.min() >= 0 and seen.max() < M


def test_batch_is_a_pure_function_of_its_arguments():
    args = (7, 11, 1, 2, 16, 500)
    first = sampler.batch_indices(*args)
    for t in (0, 30, 12):  # other batches asked in between
        sampler.batch_indices(7, t, 1, 2, 16, 500)
    assert np.array_equal(first, sampler.batch_indices(*args))
    tab = sampler.train_table(first, 7, 11, 1, 40, 36, 32, "rrc")
    sampler.train_table(first, 7, 12, 1, 40, 36, 32, "rrc")
    assert np.array_equal(tab, sampler.train_table(first, 7, 11, 1, 40, 36, 32, "rrc"))
    assert not np.array_equal(tab, sampler.train_table(first, 7, 11, 0, 40, 36, 32, "rrc"))  # another rank
    assert not np.array_equal(tab, sampler.train_table(first, 8, 11, 1, 40, 36, 32, "rrc"))  # another seed


def test_epochs_differ():
    M, batch = 128, 16
    E = sampler.steps_per_epoch(M, batch, 1)
    e0 = np.concatenate([sampler.batch_indices(0, t, 0, 1, batch, M) for t in range(E)])
    e1 = np.concatenate([sampler.batch_indices(0, E + t, 0, 1, batch, M) for t in range(E)])
    assert sorted(e0) == sorted(e1) == list(range(M)) and not np.array_equal(e0, e1)


def test_too_small_a_split_is_an_error():
    from k8s_amd.data import DataError

    with pytest.raises(DataError):
        sampler.steps_per_epoch(100, 64, 2)


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("Hs,Ws", [(40, 36), (256, 256), (30, 90), (90, 30)])
def test_rrc_boxes_lie_inside_the_source(Hs, Ws):
    tab = sampler.train_table(np.zeros(4000, dtype=np.int64), 1, 0, 0, Hs, Ws, 32, "rrc")
    y0, x0, h, w = (tab[:, k].astype(np.int64) for k in (1, 2, 3, 4))
    assert (h >= 1).all() and (w >= 1).all() and (y0 >= 0).all() and (x0 >= 0).all()
    assert (y0 + h <= Hs).all() and (x0 + w <= Ws).all()
    assert set(tab[:, 5].tolist()) == {0, 1}
    area = h * w / float(Hs * Ws)
    ratio = w / h
    fallback = (abs(Ws / Hs - ratio) < 0.05) | (area > 0.3)  # the centred fallback keeps what fits of the source
    assert (area[~fallback] > 0.07).all() and (ratio[~fallback] > 0.6).all() and (ratio[~fallback] < 1.6).all()
    assert len(np.unique(h)) > 5 and len(np.unique(w)) > 5


def test_crop_offsets_reach_both_extremes():
    Hs, Ws, S, P = 40, 36, 32, 4
    tab = sampler.train_table(np.arange(4000), 3, 9, 0, Hs, Ws, S, "crop", P)
    assert (tab[:, 3] == S).all() and (tab[:, 4] == S).all() and np.array_equal(tab[:, 0], np.arange(4000))
    assert tab[:, 1].min() == -P and tab[:, 1].max() == Hs - S + P
    assert tab[:, 2].min() == -P and tab[:, 2].max() == Ws - S + P
    assert 0.4 < tab[:, 5].mean() < 0.6


def test_evaluation_rows_are_the_centred_boxes():
    idx = np.array([5, 3])
    for aug in ("crop", "none"):
        assert sampler.eval_table(idx, 40, 36, 32, aug).tolist() == [[5, 4, 2, 32, 32, 0], [3, 4, 2, 32, 32, 0]]
    side = int(round(0.875 * 36))
    assert sampler.eval_table(idx, 40, 36, 32, "rrc").tolist() == [[5, (40 - side) // 2, (36 - side) // 2, side, side, 0],
                                                                 [3, (40 - side) // 2, (36 - side) // 2, side, side, 0]]
    assert sampler.train_table(idx, 0, 0, 0, 40, 36, 32, "none").tolist() == sampler.eval_table(idx, 40, 36, 32,
                                                                                                "none").tolist()


# ------------------------------------------------------------------------------------------------ the oracle
def _independent(src, row, a, b, S):
    """One table row composed from torch's own ops in float64: F.interpolate on the sliced box for a resized row,
    slicing a zero-padded normalised image for a copy row."""
    idx, y0, x0, h, w, flip = row
    a64, b64 = torch.tensor(a, dtype=torch.float64), torch.tensor(b, dtype=torch.float64)
    if h == S and w == S:
        norm = src[idx].double() * a64 + b64
        P = 2 * S
        img = F.pad(norm.permute(2, 0, 1), (P, P, P, P)).permute(1, 2, 0)[y0 + P:y0 + P + S, x0 + P:x0 + P + S]
    else:
        box = src[idx, y0:y0 + h, x0:x0 + w].double().permute(2, 0, 1)[None]
        img = F.interpolate(box, size=(S, S), mode="bilinear", align_corners=False, antialias=False)[0]
        img = img.permute(1, 2, 0) * a64 + b64
    if flip:
        img = img.flip(1)
    return img.float().to(torch.bfloat16)


@pytest.mark.parametrize("S", [8, 32])
def test_oracle_equals_an_independent_composition(S):
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (4, 40, 36, 3), generator=g, dtype=torch.uint8)
    a, b = kdata.norm_constants([125.3, 123.0, 113.9], [63.0, 62.1, 66.7])
    rows = [(0, 3, 2, 1, 1, 0), (1, 0, 0, 40, 36, 1), (2, 0, 33, 40, 3, 0), (3, 5, 5, 3, 2, 1), (0, 10, 4, 20, 30, 1),
            (1, 0, 0, S, S, 0), (2, -3, -4, S, S, 1), (3, 40 - S + 3, 36 - S + 4, S, S, 0), (3, 2, 1, S, S, 1)]
    rows += [tuple(r) for r in sampler.train_table(np.array([1, 1, 0, 2]), 4, 0, 0, 40, 36, S, "rrc").tolist()]
    table = torch.tensor(rows, dtype=torch.int32)
    got = ref.augment(src, table, a, b, S, "nhwc8")
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (len(rows), S, S, 8)
    assert got[..., 3:].float().abs().max() == 0
    for n, row in enumerate(rows):
        want = _independent(src, row, a, b, S)
        assert torch.equal(got[n, :, :, :3].view(torch.int16), want.contiguous().view(torch.int16)), "row %d" % n
    # the space-to-depth layout: channels (dy*2 + dx)*4 + c of pixel (i, j) = image pixel (2i+dy-3, 2j+dx-3), 0 outside
    xs = ref.augment(src, table, a, b, S, "s2d")
    assert tuple(xs.shape) == (len(rows), S // 2 + 3, S // 2 + 3, 16)
    padded = F.pad(got[..., :4].float(), (0, 0, 3, 3, 3, 3))
    for dy in (0, 1):
        for dx in (0, 1):
            q = (dy * 2 + dx) * 4
            assert torch.equal(xs[..., q:q + 4].float(), padded[:, dy::2, dx::2])
    assert kdata.augment(src, table, a, b, S, "nhwc8").equal(got)  # a host source takes the reference path


def test_reference_rejects_bad_rows():
    src = torch.zeros(2, 12, 10, 3, dtype=torch.uint8)
    a, b = kdata.norm_constants([0, 0, 0], [1, 1, 1])
    for row in [(2, 0, 0, 8, 8, 0), (0, 0, 0, 0, 8, 0), (0, 0, 0, 8, 8, 2), (0, 6, 0, 7, 4, 0)]:
        with pytest.raises(ValueError):
            ref.augment(src, torch.tensor([row], dtype=torch.int32), a, b, 8)


# ------------------------------------------------------------------------------------------------ make_dataset
def _bytes_of(path):
    return {name: open(os.path.join(path, name), "rb").read() for name in sorted(os.listdir(path))}


def test_toy_twice_gives_identical_bytes(tmp_path, toy):
    again = str(tmp_path / "again")
    assert make_dataset.main(["--toy", "--out", again]) == 0
    one, two = _bytes_of(toy), _bytes_of(again)
    assert sorted(one) == ["meta.json", "train_images.npy", "train_labels.npy", "val_images.npy", "val_labels.npy"]
    assert one == two
    other = str(tmp_path / "other")
    make_dataset.make_toy(other, seed=1, train=64, val=16)
    assert _bytes_of(other)["val_images.npy"] != one["val_images.npy"][:len(_bytes_of(other)["val_images.npy"])]
    ds = open_dataset(toy, need=("train", "val"))
    assert ds.classes == 10 and ds.mean == [127.5] * 3 and ds.std == [64.0] * 3
    assert ds.split("train").images.shape == (2048, 40, 40, 3) and ds.split("val").images.shape == (256, 40, 40, 3)
    assert isinstance(ds.split("train").images, np.memmap)
    assert set(ds.split("train").labels.tolist()) == set(range(10))
    # noise around the class prototype upscaled x8
    protos = make_dataset.toy_prototypes(10)
    lab = ds.split("val").labels
    up = np.repeat(np.repeat(protos[lab], 8, axis=1), 8, axis=2).astype(np.float64)
    inner = (up > 100) & (up < 155)  # far enough from 0 and 255 that the clip does not bias the noise
    diff = (np.asarray(ds.split("val").images, dtype=np.float64) - up)[inner]
    assert abs(diff.mean()) < 1.0 and 45 < diff.std() < 51


def test_cifar_pickle_round_trips(tmp_path):
    src = tmp_path / "cifar"
    src.mkdir()
    g = np.random.default_rng(0)
    chw = {}
    for name in ["data_batch_%d" % i for i in range(1, 6)] + ["test_batch"]:
        data = g.integers(0, 256, size=(10 if name == "test_batch" else 2, 3072), dtype=np.uint8)
        labels = [int(v) for v in g.integers(0, 10, size=len(data))]
        chw[name] = (data, labels)
        with open(src / name, "wb") as f:
            pickle.dump({b"data": data, b"labels": labels, b"batch_label": name.encode()}, f)
    out = str(tmp_path / "out")
    assert make_dataset.main(["--cifar10-batches", str(src), "--out", out]) == 0
    ds = open_dataset(out, need=("train", "val"))
    val = np.asarray(ds.split("val").images)
    assert val.shape == (10, 32, 32, 3) and ds.split("train").images.shape == (10, 32, 32, 3) and ds.classes == 10
    data, labels = chw["test_batch"]
    assert np.array_equal(val.transpose(0, 3, 1, 2).reshape(10, 3072), data)  # pixel for pixel
    assert ds.split("val").labels.tolist() == labels
    train = np.asarray(ds.split("train").images).transpose(0, 3, 1, 2).reshape(10, 3072)
    assert np.array_equal(train, np.concatenate([chw["data_batch_%d" % i][0] for i in range(1, 6)]))
    assert make_dataset.main(["--cifar10-batches", str(tmp_path / "nowhere"), "--out", out]) == 1


# ------------------------------------------------------------------------------------------------ loader (CPU)
def test_cpu_loader_batches_and_evaluation_rows(toy):
    from k8s_amd.data.loader import Loader

    ds = open_dataset(toy, need=("train", "val"))
    ld = Loader(ds, "train", "cpu", 16, image=32, seed=2, rank=1, world=2)
    x, y = ld.batch(70)
    assert tuple(x.shape) == (16, 32, 32, 8) and x.dtype == torch.float32 and y.dtype == torch.int64
    idx, labels = ld.rows(70)
    want = ref.augment(torch.from_numpy(np.array(ds.split("train").images)), torch.from_numpy(ld.table(70, idx)),
                       ld.a, ld.b, 32, "nhwc8")
    assert torch.equal(x, want.float()) and torch.equal(y, torch.from_numpy(labels))
    ev = Loader(ds, "val", "cpu", 48, image=32, rank=1, world=2, train=False)
    # batch i of rank r = samples [(i * world + r) * B, + B); 256 images: batch 2 of rank 1 starts at 240
    _, y2 = ev.batch(2)
    assert (y2[:16] >= 0).all() and (y2[16:] == -100).all()
    assert torch.equal(y2[:16], torch.from_numpy(ds.split("val").labels[240:256]))
    assert (ev.batch(3)[1] == -100).all()


# ------------------------------------------------------------------------------------------------ trainer
def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""
    env["OMP_NUM_THREADS"] = "2"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        env.pop(k, None)
    return env


def _trainer(args, timeout=240):
    p = subprocess.run([sys.executable, "-m", "k8s_amd.trainer", "--device", "cpu"] + args, env=_env(),
                       capture_output=True, text=True, timeout=timeout)
    events = []
    for line in p.stdout.splitlines():
        if line.startswith("{"):
            events.append(json.loads(line))
    return p, events


def _variant(toy, tmp_path, kind):
    """A copy of the toy set with one thing wrong."""
    path = str(tmp_path / kind)
    shutil.copytree(toy, path)
    if kind == "no_meta":
        os.remove(os.path.join(path, "meta.json"))
    elif kind == "no_train":
        os.remove(os.path.join(path, "train_images.npy"))
    elif kind == "no_val":
        os.remove(os.path.join(path, "val_labels.npy"))
    elif kind == "bad_label":
        labels = np.load(os.path.join(path, "train_labels.npy"))
        labels[17] = 10
        np.save(os.path.join(path, "train_labels.npy"), labels)
    return path


CONFIG_ERRORS = {
    "bert": (None, ["--model", "bert_tiny"]),
    "llama": (None, ["--model", "llama_tiny"]),
    "graph": (None, ["--model", "resnet_tiny", "--graph"]),
    "eval_data_train": (None, ["--model", "resnet_tiny", "--eval-every", "2", "--eval-data", "train"]),
    "no_meta": ("no_meta", ["--model", "resnet_tiny"]),
    "no_train_split": ("no_train", ["--model", "resnet_tiny"]),
    "no_val_split": ("no_val", ["--model", "resnet_tiny", "--eval-every", "2"]),
    "label_outside_classes": ("bad_label", ["--model", "resnet_tiny"]),
    "odd_image": (None, ["--model", "resnet_tiny", "--image", "31"]),
    "no_whole_batch": (None, ["--model", "resnet_tiny", "--batch", "4096"]),
}


@pytest.mark.parametrize("case", sorted(CONFIG_ERRORS))
def test_configuration_error_exits_1_with_one_sentence(toy, tmp_path, case):
    kind, args = CONFIG_ERRORS[case]
    path = _variant(toy, tmp_path, kind) if kind else toy
    p, events = _trainer(["--data-dir", path, "--steps", "2"] + args)
    assert p.returncode == 1, p.stdout[-1500:] + p.stderr[-1500:]
    errors = [line for line in p.stderr.splitlines() if line.startswith("error: ")]
    assert len(errors) == 1 and "Traceback" not in p.stderr, p.stderr[-1500:]
    assert not [e for e in events if e.get("event") in ("step0", "done")]


@pytest.mark.parametrize("accum", [1, 2])
def test_resume_gives_the_uninterrupted_run(toy, tmp_path, accum):
    common = ["--model", "resnet_tiny", "--data-dir", toy, "--batch", "16", "--image", "32", "--lr", "0.02",
              "--log-every", "1", "--accum-steps", str(accum)]
    p, ev = _trainer(common + ["--steps", "6"])
    assert p.returncode == 0, p.stderr[-1500:]
    whole = [e for e in ev if e.get("event") == "done"][-1]
    start = [e for e in ev if e.get("event") == "start"][-1]
    assert start["data"]["train"] == 2048 and start["data"]["val"] == 256 and start["data"]["resident"] is False
    assert start["data"]["augment"] == "crop" and start["data"]["steps_per_epoch"] == 128
    assert all(e["epoch"] == 0 for e in ev if e.get("event") == "step")
    ck = str(tmp_path / "ckpt")
    p, _ = _trainer(common + ["--steps", "3", "--ckpt-dir", ck])
    assert p.returncode == 0, p.stderr[-1500:]
    p, ev = _trainer(common + ["--steps", "6", "--ckpt-dir", ck])
    assert p.returncode == 0, p.stderr[-1500:]
    assert [e for e in ev if e.get("event") == "restored"][-1]["step"] == 2
    resumed = [e for e in ev if e.get("event") == "done"][-1]
    assert resumed["weights_sum"] == whole["weights_sum"] and resumed["loss"] == whole["loss"]


# top-1 on the 256 val images after the 120 steps below, through the trainer on the CPU (fp32), seeds 0, 1, 2:
# 1.00, 1.00, 1.00. (The trainer's default crop keeps the whole 40 x 40 source in view -- random offsets over the
# source zero-padded by 4 -- where the hand-written loop that measured 0.80 / 0.89 / 0.93 cut random 32 x 32 pieces out
# of it.) Chance is 0.10; the threshold lies halfway between chance and the lowest of the three.
CPU_TOP1 = (1.0, 1.0, 1.0)
CPU_THRESHOLD = (0.10 + min(CPU_TOP1)) / 2


def test_trainer_learns_the_toy_set(toy):
    p, ev = _trainer(["--model", "resnet_tiny", "--data-dir", toy, "--batch", "32", "--lr", "0.02", "--steps", "120",
                      "--eval-every", "120", "--eval-batches", "8"])
    assert p.returncode == 0, p.stderr[-1500:]
    e = [x for x in ev if x.get("event") == "eval"][-1]
    print("cpu toy top1 %.4f (examples %d)" % (e["top1"], e["examples"]))
    assert e["examples"] == 256 and e["data"] == "heldout"
    assert e["top1"] > CPU_THRESHOLD
