"""Unpadded BERT on the CPU: the span mask against its definition, the unpadded batch oracle against the padded one,
``forward_unpadded`` against ``forward`` on the same plan, the loader, and the trainer with ``--unpad``."""
import filecmp
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from k8s_amd.data import DataError, open_token_dataset
from k8s_amd.data.token_loader import TokenLoader
from k8s_amd.ops import reference as ref
from k8s_amd.ops.attention import (attention, attention_qkv, attention_reference, doc_bounds, span_bounds,
                                   span_mask_reference)
from k8s_amd.tools import make_dataset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIAL = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("toytokens"))
    assert make_dataset.main(["--toy-tokens", "--out", path]) == 0
    return path


# ------------------------------------------------------------------------------------------------ span mask
STARTS12 = [0, 0, 0, 3, 3, 5, 5, 5, 5, 5, 10, 11]


def test_span_mask_is_its_definition():
    lo, hi = span_bounds(torch.tensor([STARTS12]))
    assert lo.dtype == hi.dtype == torch.int32
    assert lo.tolist() == [STARTS12] and hi.tolist() == [[3, 3, 3, 5, 5, 10, 10, 10, 10, 10, 11, 12]]
    hidden = span_mask_reference(lo, hi)
    for i in range(12):
        for j in range(12):
            sees = int(lo[0, i]) <= j < int(hi[0, i])
            assert bool(hidden[0, i, j]) == (not sees)
            assert sees == (int(lo[0, j]) <= i < int(hi[0, j]))  # consistent tables: the key's view of the same mask
        assert not bool(hidden[0, i, i])  # every query sees itself
    # the attention output of a span is that span's attention alone
    torch.manual_seed(0)
    q, k, v = (torch.randn(1, 12, 2, 8) for _ in range(3))
    out = attention(q, k, v, causal=False, span=(lo, hi))
    assert torch.equal(out, attention_reference(q, k, v, False, span_lo=lo, span_hi=hi))
    for a, b in ((0, 3), (3, 5), (5, 10), (10, 11), (11, 12)):
        alone = attention_reference(q[:, a:b], k[:, a:b], v[:, a:b], False)
        assert torch.allclose(out[:, a:b], alone, atol=1e-6)
    # the packed entry takes the same mask
    qkv = torch.cat([t.reshape(12, 16) for t in (q, k, v)], dim=1)
    assert torch.allclose(attention_qkv(qkv, 1, 12, 2, 2, 8, causal=False, span=(lo, hi)), out, atol=1e-6)


def test_span_bounds_errors():
    for bad in ([[0, 0, 3, 3]],  # start above its index
                [[0, 1, 0, 3]],  # not ascending
                [[0, 0, 1, 1]]):  # start[start[i]] != start[i]
        with pytest.raises(ValueError):
            span_bounds(torch.tensor(bad))
    with pytest.raises(ValueError):
        span_bounds(torch.tensor([0, 0, 2]))  # not [B, S]
    with pytest.raises(ValueError):
        span_bounds(torch.tensor([[0.0, 0.0]]))  # not integer


def test_span_rejected_combinations():
    q, k, v = (torch.randn(1, 12, 2, 8) for _ in range(3))
    lo, hi = span_bounds(torch.tensor([STARTS12]))
    lens = torch.tensor([10])
    from k8s_amd.ops import nn as K

    for kw in (dict(causal=True, span=(lo, hi)),
               dict(kv_lens=lens, span=(lo, hi)),
               dict(dropout=(0.1, K.DropoutState(0), 1), span=(lo, hi)),
               dict(doc=doc_bounds(torch.tensor([STARTS12])), span=(lo, hi)),
               dict(span=(lo, None)), dict(span=(None, hi)),  # one table alone
               dict(span=(lo.long(), hi.long())),  # dtype
               dict(span=(lo[:, :6], hi[:, :6]))):  # shape
        with pytest.raises(ValueError):
            attention(q, k, v, **kw)
    with pytest.raises(ValueError):  # Sq != Sk
        attention(q, k[:, :6], v[:, :6], span=(lo, hi))
    qkv = torch.randn(12, 48)
    for kw in (dict(causal=True, span=(lo, hi)), dict(kv_lens=lens, span=(lo, hi)),
               dict(span=(lo.long(), hi.long())), dict(span=(lo[:, :6], hi[:, :6]))):
        with pytest.raises(ValueError):
            attention_qkv(qkv, 1, 12, 2, 2, 8, **kw)
    with pytest.raises(ValueError):  # the doc keyword still refuses a bidirectional call
        attention(q, k, v, causal=False, doc=doc_bounds(torch.tensor([STARTS12])))


# ------------------------------------------------------------------------------------------------ batch oracle
def _plan(toy, S, N, dtype, seed=5):
    """(src, table, cu, T, loader) of one toy batch, the tokens as ``dtype`` (int16: uint16 data)."""
    ds = open_token_dataset(toy, need=("train",), pairs=True)
    ld = TokenLoader(ds, "train", "cpu", N, S, kind="bert", max_predictions=max(1, S * 15 // 100), seed=seed)
    plan = ld.plan(1)
    cu, T = ld.stream_offsets(plan)
    tok = np.array(ld.tokens)
    src = torch.from_numpy(tok.astype(np.uint16).view(np.int16) if dtype == torch.int16 else tok.astype(np.int32))
    return src, torch.from_numpy(plan["table"]), torch.from_numpy(cu), T, ld


@pytest.mark.parametrize("S", [32, 128])
@pytest.mark.parametrize("dtype", [torch.int16, torch.int32])
def test_unpadded_oracle_is_the_padded_one_gathered(toy, S, dtype):
    N = 5
    src, table, cu, T, ld = _plan(toy, S, N, dtype)
    P = ld.P
    ids2, types2, labels2, pos2 = ref.mlm_batch(src, table, S, P, 512, SPECIAL, 7)
    ids, types, pos, labels, rows, cls_rows, lo, hi = ref.mlm_batch_unpadded(src, table, cu, T, S, P, 512, SPECIAL, 7)
    total = int(cu[-1])
    assert T % 128 == 0 and 0 <= T - total < 128 and T == ref.unpad_stream_rows(total)
    assert ids.shape == types.shape == pos.shape == (T,) and lo.shape == hi.shape == (1, T)
    assert lo.dtype == hi.dtype == torch.int32 and rows.shape == labels.shape == (N, P)
    for n in range(N):
        a, b = int(cu[n]), int(cu[n + 1])
        L = b - a
        assert L == int(table[n, 1] + table[n, 3] + 3)
        assert torch.equal(ids[a:b], ids2[n, :L]) and torch.equal(types[a:b], types2[n, :L])
        assert torch.equal(pos[a:b], torch.arange(L))
        assert bool((lo[0, a:b] == a).all()) and bool((hi[0, a:b] == b).all())
        assert bool((ids2[n, L:] == SPECIAL[0]).all())  # what the stream leaves out is padding
        k = int(table[n, 4])
        assert torch.equal(rows[n, :k], a + pos2[n, :k]) and bool((rows[n, k:] == a).all())
        assert torch.equal(ids[rows[n, :k]], ids2[n, pos2[n, :k]])
    assert torch.equal(labels, labels2) and torch.equal(cls_rows, cu[:N])
    assert bool((ids[cls_rows] == SPECIAL[1]).all())
    # the tail: one pad span
    assert bool((ids[total:] == SPECIAL[0]).all()) and bool((types[total:] == 0).all()) and bool((pos[total:] == 0).all())
    assert bool((lo[0, total:] == total).all()) and bool((hi[0, total:] == T).all())
    # consistent tables: span_bounds of lo gives them back
    again = span_bounds(lo.long())
    assert torch.equal(again[0], lo) and torch.equal(again[1], hi)


def test_unpadded_oracle_rejects_bad_cu_and_T(toy):
    src, table, cu, T, ld = _plan(toy, 32, 5, torch.int32)
    args = (32, ld.P, 512, SPECIAL, 7)
    ref.mlm_batch_unpadded(src, table, cu, T, *args)
    shifted = cu.clone()
    shifted[0] = 1
    longer = cu.clone()
    longer[2:] += 1
    for bad_cu, bad_T in ((cu[:-1], T),  # length
                          (cu.int(), T),  # dtype
                          (shifted, T),  # cu[0] != 0
                          (longer, T),  # a difference that is not la + lb + 3
                          (cu, int(cu[-1]) // 128 * 128),  # T below cu[N]
                          (cu, T + 1),  # not a multiple of 128
                          (cu, T + 128)):  # more than one tile of tail
        with pytest.raises(ValueError):
            ref.mlm_batch_unpadded(src, table, bad_cu, bad_T, *args)
    bad_table = table.clone()
    bad_table[0, 1] = 0  # what mlm_batch rejects is rejected
    with pytest.raises(ValueError):
        ref.mlm_batch_unpadded(src, bad_table, cu, T, *args)


# ------------------------------------------------------------------------------------------------ model
def test_forward_unpadded_equals_forward_in_fp32(toy):
    """``bert_tiny`` in fp32, batch 8, S = 32: the same plan padded (``kv_lens``) and unpadded. In exact arithmetic
    the losses and gradients are equal; fp32 sums in another order differ by far less than 1e-4, the bound
    ``tests/test_doc_mask_cpu.py`` uses for its fp32 "row against documents alone" comparison."""
    from k8s_amd.models.registry import build

    grads, losses = [], []
    for unpad in (False, True):
        w = build("bert_tiny", "cpu", batch=8, seq=32, seed=2, data={"dir": toy, "unpad": unpad})
        try:
            b = w.batch(3)
            assert len(b) == (9 if unpad else 6)
            w.store.begin_step()
            loss = w.loss(b)
            loss.backward()
            w.store.zero_unwritten()
            losses.append(float(loss.detach()))
            grads.append({p.name: p.grad.detach().clone() for p in w.store.params})
            if unpad:
                assert b[0].dim() == 1 and b[0].numel() % 128 == 0 and b[0].numel() <= 8 * 32
        finally:
            w.close()
    print("padded %.7f unpadded %.7f" % tuple(losses))
    assert abs(losses[0] - losses[1]) <= 1e-4 * abs(losses[0])
    assert grads[0].keys() == grads[1].keys()
    for name, g in grads[0].items():
        norm = float(g.norm())
        err = float((grads[1][name] - g).norm())
        assert norm > 0 and err <= 1e-4 * norm, (name, err, norm)


def test_forward_unpadded_refuses_dropout(toy):
    import dataclasses

    from k8s_amd.models import bert as M
    from k8s_amd.models.registry import build
    from k8s_amd.parallel.flat import ParamStore

    with pytest.raises(ValueError):
        build("bert_tiny", "cpu", batch=8, seq=32, dropout=0.1, data={"dir": toy, "unpad": True})
    model = M.BertForPreTraining(ParamStore(), dataclasses.replace(M.BERT_TINY, hidden_dropout=0.1)).finalize("cpu")
    z = torch.zeros(128, dtype=torch.int64)
    with pytest.raises(ValueError):
        model.forward_unpadded(z, z, z, z[:12].reshape(1, 12), z[:1], z[:12].reshape(1, 12), z[:1], z.int(), z.int())


# ------------------------------------------------------------------------------------------------ loader
def test_loader_is_a_pure_function_of_seed_t_rank(toy):
    ds = open_token_dataset(toy, need=("train", "val"), pairs=True)
    kw = dict(kind="bert", max_predictions=12, unpad=True)
    a = TokenLoader(ds, "train", "cpu", 8, 32, seed=4, **kw)
    b = TokenLoader(ds, "train", "cpu", 8, 32, seed=4, **kw)
    first = a.batch(5)
    a.batch(2)
    for x, y in zip(first, b.batch(5)):
        assert torch.equal(x, y)
    assert len(first) == 9 and a.last_real_tokens == a.real_tokens(2)
    assert not all(torch.equal(x, y) for x, y in zip(first, TokenLoader(ds, "train", "cpu", 8, 32, seed=5, **kw).batch(5)))
    other = TokenLoader(ds, "train", "cpu", 8, 32, seed=4, rank=1, world=2, **kw).batch(5)
    assert not torch.equal(first[0][:64], other[0][:64])
    assert a.info()["unpad"] is True and a.info()["stream_rows"] == a.batch(0)[0].numel() == a.stream_rows(0)
    # the same plan padded: the unpadded stream is its real positions
    padded = TokenLoader(ds, "train", "cpu", 8, 32, seed=4, kind="bert", max_predictions=12).batch(5)
    lens = padded[5].long()
    real = torch.arange(32)[None, :] < lens[:, None]
    total = int(lens.sum())
    assert torch.equal(first[0][:total], padded[0][real]) and torch.equal(first[3], padded[2])
    assert torch.equal(first[4], padded[3])
    # evaluation rows past the end of the split keep -100 labels and nsp = -100
    ev = TokenLoader(ds, "val", "cpu", 16, 32, train=False, **kw)
    last = ev.batch((ev.items + 15) // 16 - 1)
    plan = ev.plan((ev.items + 15) // 16 - 1)
    assert plan["real"] is not None and bool((last[3][~torch.from_numpy(plan["real"])] == -100).all())
    assert bool((last[4][~torch.from_numpy(plan["real"])] == -100).all())
    with pytest.raises(DataError):
        TokenLoader(ds, "train", "cpu", 8, 32, kind="llama", unpad=True)
    with pytest.raises(DataError):
        TokenLoader(ds, "train", "cpu", 8, 32, kind="llama", doc_mask=True, unpad=True)


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
    return p, [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]


# tests/test_token_data_cpu.py's threshold for the same command without --unpad: halfway between chance
# (ln 504 + ln 2) and the worst of the three padded runs, 4.3779
CPU_THRESHOLD = (math.log(504) + math.log(2) + 4.3779) / 2


def test_bert_learns_the_toy_tokens_unpadded(toy):
    p, ev = _trainer(["--model", "bert_tiny", "--data-dir", toy, "--batch", "32", "--lr", "0.001", "--steps", "300",
                      "--eval-every", "300", "--eval-batches", "8", "--unpad"])
    assert p.returncode == 0, p.stderr[-1500:]
    e = [x for x in ev if x.get("event") == "eval"][-1]
    print("cpu toy tokens unpadded eval loss %.4f (examples %d)" % (e["loss"], e["examples"]))
    assert round(CPU_THRESHOLD, 3) == 5.647
    assert e["data"] == "heldout" and e["examples"] > 249
    assert e["loss"] < CPU_THRESHOLD
    start = [x for x in ev if x.get("event") == "start"][-1]["data"]
    assert start["unpad"] is True and start["stream_rows"] % 128 == 0 and 0 < start["stream_rows"] <= 32 * 32
    steps = [x for x in ev if x.get("event") == "step"]
    assert steps and all(0 < x["real_tokens_per_sec"] < x["tokens_per_sec"] for x in steps)


@pytest.mark.parametrize("accum", [1, 2])
def test_unpadded_resume_gives_the_uninterrupted_run(toy, tmp_path, accum):
    common = ["--model", "bert_tiny", "--data-dir", toy, "--batch", "8", "--unpad", "--log-every", "1",
              "--accum-steps", str(accum)]
    p, ev = _trainer(common + ["--steps", "6"])
    assert p.returncode == 0, p.stderr[-1500:]
    whole = [e for e in ev if e.get("event") == "done"][-1]
    whole_losses = {e["step"]: e["loss"] for e in ev if e.get("event") in ("step", "step0")}
    ck = str(tmp_path / "ckpt")
    p, _ = _trainer(common + ["--steps", "3", "--ckpt-dir", ck])
    assert p.returncode == 0, p.stderr[-1500:]
    p, ev = _trainer(common + ["--steps", "6", "--ckpt-dir", ck])
    assert p.returncode == 0, p.stderr[-1500:]
    assert [e for e in ev if e.get("event") == "restored"][-1]["step"] == 2
    resumed = [e for e in ev if e.get("event") == "done"][-1]
    losses = {e["step"]: e["loss"] for e in ev if e.get("event") in ("step", "step0")}
    assert sorted(losses) == [3, 4, 5] and all(losses[s] == whole_losses[s] for s in losses)
    assert resumed["weights_sum"] == whole["weights_sum"] and resumed["loss"] == whole["loss"]
    assert whole["data"]["unpad"] is True


@pytest.mark.parametrize("args", [["--model", "bert_tiny", "--unpad"],  # no --data-dir
                                  ["--model", "llama_tiny", "--data-dir", "TOY", "--unpad"],
                                  ["--model", "bert_tiny", "--data-dir", "TOY", "--unpad", "--dropout", "0.1"]])
def test_unpad_configuration_error_exits_1_with_one_sentence(toy, args):
    p, events = _trainer([toy if a == "TOY" else a for a in args] + ["--steps", "2"])
    assert p.returncode == 1, p.stdout[-1500:] + p.stderr[-1500:]
    errors = [line for line in p.stderr.splitlines() if line.startswith("error: ")]
    assert len(errors) == 1 and "--unpad" in errors[0] and "Traceback" not in p.stderr, p.stderr[-1500:]
    assert not [e for e in events if e.get("event") in ("start", "step0", "done")]  # before the model is built


def test_tokens_per_segment_default_leaves_the_toy_files_unchanged(toy, tmp_path):
    same, other = str(tmp_path / "same"), str(tmp_path / "other")
    assert make_dataset.main(["--toy-tokens", "--out", same, "--tokens-per-segment", "4", "12"]) == 0
    names = sorted(os.listdir(toy))
    assert names == sorted(os.listdir(same)) and any(n.endswith(".npy") for n in names)
    match, mismatch, errors = filecmp.cmpfiles(toy, same, names, shallow=False)
    assert sorted(match) == names and not mismatch and not errors
    # what the set looked like before the option existed: 512 documents, 2057 segments, 16457 tokens
    ds = open_token_dataset(toy, need=("train",), pairs=True)
    assert (ds.split("train").T, ds.split("train").G, ds.split("train").D) == (16457, 2057, 512)
    assert make_dataset.main(["--toy-tokens", "--out", other, "--tokens-per-segment", "8", "56", "--train-docs", "64",
                              "--val-docs", "8"]) == 0
    sp = open_token_dataset(other, need=("train",), pairs=True).split("train")
    lens = np.diff(sp.segments)
    assert lens.min() >= 8 and lens.max() <= 56 and 28 < lens.mean() < 36
    assert make_dataset.main(["--toy-tokens", "--out", other, "--tokens-per-segment", "9", "8"]) == 1
