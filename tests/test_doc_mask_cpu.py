"""Document-boundary attention masks on the CPU: the reference mask against its literal definition, ``doc_bounds``,
the ``causal_doc_batch`` definition on the toy token set, independence of the documents of a row in the fp32 model,
the trainer's ``--doc-mask`` and the toy generator's ``--segments-per-doc``."""
import hashlib
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from k8s_amd.data import DataError, open_token_dataset
from k8s_amd.data.token_loader import TokenLoader
from k8s_amd.ops import reference as ref
from k8s_amd.ops.attention import attention, attention_reference, doc_bounds, doc_mask_reference
from k8s_amd.tools import make_dataset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("toytokens"))
    assert make_dataset.main(["--toy-tokens", "--out", path]) == 0
    return path


def _lo_of(S, starts):
    s = torch.tensor(starts)
    return s[torch.searchsorted(s, torch.arange(S), right=True) - 1]


def _consistent(lo, hi, S):
    lo, hi = lo.long(), hi.long()
    i = torch.arange(S).expand_as(lo)
    assert bool((lo[:, 1:] >= lo[:, :-1]).all()) and bool((hi[:, 1:] >= hi[:, :-1]).all())
    assert bool((0 <= lo).all()) and bool((lo <= i).all()) and bool((i < hi).all()) and bool((hi <= S).all())
    assert torch.equal(torch.gather(lo, 1, lo), lo)
    for b in range(lo.shape[0]):
        for a, e in set(zip(lo[b].tolist(), hi[b].tolist())):
            assert bool((lo[b, a:e] == a).all()) and bool((hi[b, a:e] == e).all())


# ------------------------------------------------------------------------------------------------ mask and bounds
def test_reference_mask_is_the_literal_definition():
    S = 16
    lo = torch.stack([_lo_of(S, [0, 1, 5, 6, 15]), _lo_of(S, [0]), _lo_of(S, list(range(S)))])
    lo32, hi32 = doc_bounds(lo)
    _consistent(lo32, hi32, S)
    masked = doc_mask_reference(lo32)
    for b in range(lo.shape[0]):
        for i in range(S):
            for j in range(S):
                sees = int(lo[b, i]) <= j <= i
                assert bool(masked[b, i, j]) == (not sees)
                assert sees == (j <= i < int(hi32[b, j]))  # the key-side form of the same mask
    # through the op: each document's rows equal causal attention over the document alone
    torch.manual_seed(0)
    q, k, v = (torch.randn(3, S, 2, 8) for _ in range(3))
    out = attention(q, k, v, causal=True, doc=(lo32, hi32))
    assert torch.equal(out, attention_reference(q, k, v, True, doc_lo=lo32))
    alone = attention_reference(q[:1, 6:15], k[:1, 6:15], v[:1, 6:15], True)
    assert torch.allclose(out[:1, 6:15], alone, atol=1e-6)
    qq = q.clone().requires_grad_(True)
    attention(qq, k, v, causal=True, doc=(lo32, hi32))[0, 6:15].sum().backward()
    assert qq.grad[0, :6].abs().max() == 0 and qq.grad[0, 15:].abs().max() == 0 and qq.grad[0, 6:15].abs().max() > 0


def test_doc_bounds_round_trips_and_rejects_inconsistent_starts():
    S = 12
    lo = torch.stack([_lo_of(S, [0, 3, 4, 11]), _lo_of(S, [0])])
    lo32, hi32 = doc_bounds(lo)
    assert lo32.dtype == hi32.dtype == torch.int32 and torch.equal(lo32.long(), lo)
    assert hi32[0].tolist() == [3, 3, 3, 4, 11, 11, 11, 11, 11, 11, 11, 12] and hi32[1].tolist() == [S] * S
    assert torch.equal(doc_bounds(lo.int())[1], hi32)
    for bad in ([0, 0, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1],       # not ascending
                [0, 0, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3],       # lo[2] = 3 > 2
                [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]):      # lo[1] = 0 but tokens 2.. claim a start at 1
        with pytest.raises(ValueError) as e:
            doc_bounds(torch.tensor([bad]))
        assert str(e.value).count(".") == 0 and "\n" not in str(e.value)
    with pytest.raises(ValueError):
        doc_bounds(torch.zeros(12, dtype=torch.int64))
    q = torch.randn(1, S, 1, 8)
    for kw in (dict(causal=False), dict(causal=True, kv_lens=torch.tensor([5]))):
        with pytest.raises(ValueError):
            attention(q, q, q, doc=(lo32[:1], hi32[:1]), **kw)


# ------------------------------------------------------------------------------------------------ batch definition
def test_causal_doc_batch_reference_on_the_toy_set(toy):
    ds = open_token_dataset(toy, need=("train", "val"))
    S = 64
    ld = TokenLoader(ds, "train", "cpu", 8, S, kind="llama", doc_mask=True, seed=0)
    sp = ds.split("train")
    doc_tok = sp.segments[sp.docs]
    assert np.diff(doc_tok).min() == 9 and np.diff(doc_tok).max() == 63
    W = (sp.T - 1) // S
    at = np.arange(W, dtype=np.int64) * S
    ids, labels, lo, hi, pos = ref.causal_doc_batch(torch.from_numpy(np.array(sp.tokens).view(np.int16)),
                                                    torch.from_numpy(at), torch.from_numpy(at),
                                                    torch.from_numpy(doc_tok), S)
    assert lo.dtype == hi.dtype == pos.dtype == torch.int32 and ids.dtype == labels.dtype == torch.int64
    _consistent(lo, hi, S)
    assert torch.equal(pos.long(), torch.arange(S).expand(W, S) - lo.long()) and int(pos.min()) == 0
    per_row = np.array([len(set(r.tolist())) for r in lo])
    assert per_row.min() == 2 and per_row.max() == 5 and abs(per_row.mean() - 2.96) < 0.01
    assert ld.info()["doc_mask"] is True
    # a document's last token predicts nothing: as many -100 labels as document ends inside the windows
    ends = doc_tok[1:] - 1  # the last token of every document
    inside = ends[ends < W * S]
    assert int((labels == -100).sum()) == len(inside) == int(np.searchsorted(doc_tok, W * S, side="right")) - 1
    flat = labels.reshape(-1)
    assert bool((flat[torch.from_numpy(inside)] == -100).all())
    tok = torch.from_numpy(np.array(sp.tokens).astype(np.int64))
    keep = flat != -100
    assert torch.equal(flat[keep], tok[1:W * S + 1][keep]) and torch.equal(ids.reshape(-1), tok[:W * S])
    # the loader: out of order, and the ranks partition the global batch
    a, b = ld.batch(5), ld.batch(2)
    again = TokenLoader(ds, "train", "cpu", 8, S, kind="llama", doc_mask=True, seed=0)
    for x, y in zip(a + b, again.batch(5) + again.batch(2)):
        assert torch.equal(x, y)
    assert len(a) == 5 and round(ld.docs_per_row(5), 6) == round(np.mean([len(set(r.tolist())) for r in a[2]]), 6)
    whole = TokenLoader(ds, "train", "cpu", 8, S, kind="llama", doc_mask=True, seed=0).batch(3)
    halves = [TokenLoader(ds, "train", "cpu", 4, S, kind="llama", doc_mask=True, seed=0, rank=r, world=2).batch(3)
              for r in range(2)]
    rows = {tuple(r.tolist()) for r in whole[0]}
    assert rows == {tuple(r.tolist()) for h in halves for r in h[0]} and len(rows) == 8
    plain = TokenLoader(ds, "train", "cpu", 8, S, kind="llama", seed=0).batch(5)
    assert len(plain) == 2 and torch.equal(plain[0], a[0])  # the flag off: the batch of before
    assert torch.equal(torch.where(a[1] == -100, plain[1], a[1]), plain[1])


def test_reference_and_loader_reject_bad_inputs(toy, tmp_path):
    src = torch.arange(100, dtype=torch.int32)
    doc_tok = torch.tensor([0, 10, 40, 100])
    ok = torch.tensor([0, 35])
    ref.causal_doc_batch(src, ok, ok, doc_tok, 64)
    for bad in (dict(doc_tok=torch.tensor([0, 10, 10, 100])), dict(doc_tok=torch.tensor([1, 10, 100])),
                dict(abs_starts=torch.tensor([0, 36])), dict(abs_starts=torch.tensor([0])),
                dict(starts=torch.tensor([0, 36]))):
        kw = dict(dict(starts=ok, abs_starts=ok, doc_tok=doc_tok), **bad)
        with pytest.raises(ValueError):
            ref.causal_doc_batch(src, kw["starts"], kw["abs_starts"], kw["doc_tok"], 64)
    path = str(tmp_path / "nodocs")
    shutil.copytree(toy, path)
    os.remove(os.path.join(path, "train_docs.npy"))
    with pytest.raises(DataError):
        TokenLoader(open_token_dataset(path), "train", "cpu", 8, 64, kind="llama", doc_mask=True)


# ------------------------------------------------------------------------------------------------ model
def test_documents_of_a_row_are_independent_in_the_fp32_model():
    """A row of two documents with the mask and restarted positions: its loss times its label count is the sum over
    the two documents run alone, within relative 1e-4 -- two orders above fp32 accumulation error over 256-wide dot
    products, three below what a leak changes; without the mask the same row differs by more."""
    from k8s_amd.models.registry import build

    w = build("llama_tiny", "cpu", batch=1, seed=5)
    gen = torch.Generator().manual_seed(3)
    n1, n2 = 23, 41
    S = n1 + n2
    ids = torch.randint(4, 512, (1, S), generator=gen)

    def shifted(x):  # next-token labels inside one document: the last token predicts nothing
        return torch.cat([x[:, 1:], torch.full((1, 1), -100)], 1)

    d1, d2 = ids[:, :n1], ids[:, n1:]
    labels = torch.cat([shifted(d1), shifted(d2)], 1)
    lo, hi = doc_bounds(_lo_of(S, [0, n1])[None])
    pos = torch.arange(S, dtype=torch.int32)[None] - lo
    with torch.no_grad():
        row = float(w.loss((ids, labels, lo, hi, pos))) * (S - 2)
        alone = float(w.loss((d1, shifted(d1)))) * (n1 - 1) + float(w.loss((d2, shifted(d2)))) * (n2 - 1)
        leaky = float(w.loss((ids, labels))) * (S - 2)
    print("row %.6f alone %.6f unmasked %.6f" % (row, alone, leaky))
    assert abs(row - alone) <= 1e-4 * abs(alone)
    assert abs(leaky - alone) > 1e-4 * abs(alone)
    with pytest.raises(ValueError):
        w.loss((ids, labels, lo, hi))


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


def _val_labels(toy, S=64):
    """Real labels of the val split's windows, from the host arrays: every token but its document's last."""
    ds = open_token_dataset(toy, need=("val",))
    sp = ds.split("val")
    W = (sp.T - 1) // S
    ends = sp.segments[sp.docs][1:] - 1
    return W * S - int((ends < W * S).sum())


def test_trainer_doc_mask_trains_evaluates_and_resumes(toy, tmp_path):
    common = ["--model", "llama_tiny", "--data-dir", toy, "--doc-mask", "--batch", "8", "--log-every", "1"]
    p, ev = _trainer(common + ["--steps", "4", "--eval-every", "4", "--eval-batches", "50"])
    assert p.returncode == 0, p.stderr[-1500:]
    start = [e for e in ev if e.get("event") == "start"][-1]["data"]
    assert start["doc_mask"] is True and 2.0 <= start["docs_per_row"] <= 5.0
    e = [x for x in ev if x.get("event") == "eval"][-1]
    assert e["examples"] == _val_labels(toy) and math.isfinite(e["loss"])
    whole = [x for x in ev if x.get("event") == "done"][-1]
    assert whole["data"]["doc_mask"] is True and whole["data"]["docs_per_row"] == start["docs_per_row"]
    ck = str(tmp_path / "ckpt")
    p, _ = _trainer(common + ["--steps", "2", "--ckpt-dir", ck])
    assert p.returncode == 0, p.stderr[-1500:]
    p, ev = _trainer(common + ["--steps", "4", "--ckpt-dir", ck])
    assert p.returncode == 0, p.stderr[-1500:]
    assert [x for x in ev if x.get("event") == "restored"][-1]["step"] == 1
    resumed = [x for x in ev if x.get("event") == "done"][-1]
    assert resumed["weights_sum"] == whole["weights_sum"] and resumed["loss"] == whole["loss"]
    # without the flag the start event says nothing of documents
    p, ev = _trainer(common[:4] + ["--batch", "8", "--steps", "1"])
    assert p.returncode == 0 and "doc_mask" not in [x for x in ev if x.get("event") == "start"][-1]["data"]


@pytest.mark.parametrize("case", ["no_data_dir", "bert", "no_docs"])
def test_doc_mask_configuration_error_exits_1_with_one_sentence(toy, tmp_path, case):
    if case == "no_data_dir":
        args = ["--model", "llama_tiny"]
    elif case == "bert":
        args = ["--model", "bert_tiny", "--data-dir", toy]
    else:
        path = str(tmp_path / "nodocs")
        shutil.copytree(toy, path)
        os.remove(os.path.join(path, "train_docs.npy"))
        args = ["--model", "llama_tiny", "--data-dir", path]
    p, events = _trainer(args + ["--doc-mask", "--steps", "2"])
    assert p.returncode == 1, p.stdout[-1500:] + p.stderr[-1500:]
    errors = [line for line in p.stderr.splitlines() if line.startswith("error: ")]
    assert len(errors) == 1 and "Traceback" not in p.stderr, p.stderr[-1500:]
    assert not [e for e in events if e.get("event") in ("step0", "done")]


# Held-out loss on the toy val split after the 300 steps below, through the trainer on the CPU (fp32), seeds 0, 1, 2,
# with --doc-mask: MASKED_EVAL_LOSS; without it: PLAIN_EVAL_LOSS (the README's table). Chance is ln 504, uniform over
# the 504 non-special ids; the threshold lies halfway between chance and the worst of the three masked runs. (The two
# rows are means over different label sets: the masked runs do not score the first token of a document, which nothing
# in its own document predicts.)
MASKED_EVAL_LOSS = (1.8295, 1.8557, 1.8515)
PLAIN_EVAL_LOSS = (2.2332, 2.2493, 2.2719)
CHANCE = math.log(504)
THRESHOLD = (CHANCE + max(MASKED_EVAL_LOSS)) / 2


def test_llama_learns_the_toy_tokens_with_the_mask(toy):
    p, ev = _trainer(["--model", "llama_tiny", "--data-dir", toy, "--doc-mask", "--batch", "8", "--lr", "0.001",
                      "--steps", "300", "--eval-every", "300", "--eval-batches", "50"])
    assert p.returncode == 0, p.stderr[-1500:]
    e = [x for x in ev if x.get("event") == "eval"][-1]
    print("cpu toy tokens eval loss with the document mask %.4f (examples %d)" % (e["loss"], e["examples"]))
    assert e["data"] == "heldout" and e["examples"] == _val_labels(toy)
    assert e["loss"] < THRESHOLD


# ------------------------------------------------------------------------------------------------ toy generator
# sha256 of the arrays' bytes (int64) from the generator before --segments-per-doc existed, seed 0
TOY_HASHES = {0: ("bae1d9877c8b5909", "b6935c23a8c89929", "3944fda839390a6a"),
              1: ("7b9fb332f924603f", "76f33b188d1dd5b6", "d7a9c046cb159dbb")}


def test_toy_generator_default_is_unchanged_and_segments_per_doc_sets_the_lengths(tmp_path):
    for which, n in ((0, 512), (1, 64)):
        got = tuple(hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]
                    for x in make_dataset.toy_token_split(0, which, n))
        assert got == TOY_HASHES[which]
    path = str(tmp_path / "long")
    assert make_dataset.main(["--toy-tokens", "--out", path, "--train-docs", "16", "--val-docs", "4",
                              "--segments-per-doc", "40", "40"]) == 0
    sp = open_token_dataset(path).split("train")
    assert np.diff(sp.docs).tolist() == [40] * 16
    lengths = np.diff(sp.segments[sp.docs])
    assert lengths.min() >= 40 * 4 and lengths.max() <= 40 * 12 and 250 < lengths.mean() < 400
    assert make_dataset.main(["--toy-tokens", "--out", path, "--segments-per-doc", "3", "2"]) == 1
