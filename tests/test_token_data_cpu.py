"""Token datasets on the CPU: the format, the sampler, the MLM batch definition (``ops.reference.mlm_batch``, the GPU
kernel's oracle) and training BERT / Llama on the toy token set through the trainer."""
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
from k8s_amd.data import token_sampler as ts
from k8s_amd.data.token_loader import TokenLoader
from k8s_amd.ops import reference as ref
from k8s_amd.tools import make_dataset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("toytokens"))
    assert make_dataset.main(["--toy-tokens", "--out", path]) == 0
    return path


@pytest.fixture(scope="module")
def image_toy(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("toyimages"))
    make_dataset.make_toy(path, train=64, val=16)
    return path


# ------------------------------------------------------------------------------------------------ format
def test_toy_tokens_round_trip_and_follow_the_rule(toy, tmp_path):
    ds = open_token_dataset(toy, need=("train", "val"), pairs=True)
    assert ds.vocab == 512 and ds.special == (0, 1, 2, 3)
    tr, va = ds.split("train"), ds.split("val")
    assert tr.D == 512 and va.D == 64 and isinstance(tr.tokens, np.memmap) and tr.tokens.dtype == np.uint16
    assert tr.segments[-1] == tr.T and tr.docs[-1] == tr.G
    seg_len, doc_len = np.diff(tr.segments), np.diff(tr.docs)
    assert seg_len.min() == 4 and seg_len.max() == 12 and doc_len.min() == 2 and doc_len.max() == 6
    tok = np.asarray(tr.tokens, dtype=np.int64)
    assert tok.min() >= 8 and tok.max() < 8 + 8 * 63
    topic = (tok - 8) // 63
    for d in range(tr.D):  # one topic per document
        a, b = tr.segments[tr.docs[d]], tr.segments[tr.docs[d + 1]]
        assert len(set(topic[a:b].tolist())) == 1
    # inside a segment, token i + 1 follows base + (5 off + 1) mod 63 with probability 0.9 + 0.1 / 63
    off = (tok - 8) % 63
    inner = np.ones(tr.T, dtype=bool)
    inner[tr.segments[:-1]] = False
    follows = (off[1:] == (5 * off[:-1] + 1) % 63)[inner[1:]]
    p = 0.9 + 0.1 / 63
    assert abs(follows.mean() - p) < 4 * math.sqrt(p * (1 - p) / len(follows))
    # a pure function of the seed
    again, other = str(tmp_path / "again"), str(tmp_path / "other")
    make_dataset.make_toy_tokens(again)
    make_dataset.make_toy_tokens(other, seed=1)
    for f in ("train_tokens.npy", "val_segments.npy", "val_docs.npy", "meta.json"):
        assert open(os.path.join(again, f), "rb").read() == open(os.path.join(toy, f), "rb").read()
    assert not np.array_equal(np.load(os.path.join(other, "train_tokens.npy"))[:1000], tok[:1000])
    # int32 storage above 65536 ids
    big = str(tmp_path / "big")
    make_dataset.make_toy_tokens(big, vocab=70000)
    assert open_token_dataset(big, pairs=True).split("train").tokens.dtype == np.int32


def _variant(toy, tmp_path, kind):
    path = str(tmp_path / kind)
    shutil.copytree(toy, path)
    f = lambda name: os.path.join(path, name)  # noqa: E731
    meta = json.load(open(f("meta.json")))
    if kind == "bad_dtype":
        np.save(f("train_tokens.npy"), np.load(f("train_tokens.npy")).astype(np.int64))
    elif kind == "bad_offsets_dtype":
        np.save(f("train_segments.npy"), np.load(f("train_segments.npy")).astype(np.int32))
    elif kind == "non_monotone":
        seg = np.load(f("train_segments.npy"))
        seg[5] = seg[4]
        np.save(f("train_segments.npy"), seg)
    elif kind == "segments_short":
        np.save(f("train_segments.npy"), np.load(f("train_segments.npy"))[:-1])
    elif kind == "token_outside_vocab":
        tok = np.load(f("train_tokens.npy"))
        tok[123] = 512
        np.save(f("train_tokens.npy"), tok)
    elif kind == "one_document":
        np.save(f("train_docs.npy"), np.array([0, len(np.load(f("train_segments.npy"))) - 1], dtype=np.int64))
    elif kind == "specials_clash":
        meta["mask"] = meta["sep"]
    elif kind == "special_outside_vocab":
        meta["mask"] = 512
    elif kind == "uint16_vocab":
        meta["vocab"] = 70000
    elif kind == "no_vocab":
        del meta["vocab"]
    elif kind == "no_train":
        os.remove(f("train_tokens.npy"))
    json.dump(meta, open(f("meta.json"), "w"))
    return path


FORMAT_ERRORS = ["bad_dtype", "bad_offsets_dtype", "non_monotone", "segments_short", "token_outside_vocab",
                 "one_document", "specials_clash", "special_outside_vocab", "uint16_vocab", "no_vocab", "no_train"]


@pytest.mark.parametrize("kind", FORMAT_ERRORS)
def test_format_errors_are_one_sentence(toy, tmp_path, kind):
    with pytest.raises(DataError) as e:
        open_token_dataset(_variant(toy, tmp_path, kind), pairs=True)
    assert "\n" not in str(e.value)


def test_llama_needs_only_kind_and_vocab(toy, tmp_path, image_toy):
    path = str(tmp_path / "stream")
    os.makedirs(path)
    shutil.copy(os.path.join(toy, "train_tokens.npy"), path)
    json.dump({"kind": "tokens", "vocab": 512}, open(os.path.join(path, "meta.json"), "w"))
    ds = open_token_dataset(path)
    assert ds.special is None and ds.split("train").segments is None
    ids, labels = TokenLoader(ds, "train", "cpu", 4, 64, kind="llama").batch(0)
    assert torch.equal(ids[:, 1:], labels[:, :-1])
    with pytest.raises(DataError):
        open_token_dataset(path, pairs=True)
    with pytest.raises(DataError):
        open_token_dataset(image_toy)


# ------------------------------------------------------------------------------------------------ sampler
def test_truncation_rule_and_prediction_count():
    def slow(la, lb, budget):
        while la + lb > budget:
            if la >= lb:
                la -= 1
            else:
                lb -= 1
        return la, lb

    for la in range(1, 24):
        for lb in range(1, 24):
            for budget in (2, 3, 7, 10, 29, 60):
                assert ts.truncate_pair(la, lb, budget) == slow(la, lb, budget)
    assert ts.truncate_pair(10, 4, 9) == (5, 4) and ts.truncate_pair(6, 6, 9) == (4, 5)
    # n = min(P, max(1, round-half-up(0.15 L)), candidates) at L = 4, 10, 32, 128, 512
    assert [ts.n_predictions(L, 76, L - 3) for L in (4, 10, 32, 128, 512)] == [1, 2, 5, 19, 76]
    assert [ts.n_predictions(L, 20, L - 3) for L in (4, 10, 32, 128, 512)] == [1, 2, 5, 19, 20]
    assert ts.n_predictions(512, 512, 509) == 77 and ts.n_predictions(30, 20, 27) == 5  # 76.8 -> 77, 4.5 -> 5
    assert ts.n_predictions(5, 20, 2) == 1 and ts.n_predictions(20, 20, 2) == 2


def test_batches_are_reproducible_out_of_order_and_ranks_partition(toy):
    ds = open_token_dataset(toy, pairs=True)
    one = TokenLoader(ds, "train", "cpu", 32, 32, max_predictions=12, seed=5)
    first = {t: one.batch(t) for t in (0, 63, 64, 200)}
    for t in (200, 64, 0, 63):  # any order, and from a loader that never saw the others
        again = TokenLoader(ds, "train", "cpu", 32, 32, max_predictions=12, seed=5).batch(t)
        assert all(torch.equal(a, b) for a, b in zip(first[t], again))
        assert all(torch.equal(a, b) for a, b in zip(first[t], one.batch(t)))
    assert one.steps_per_epoch == 2057 // 32 == 64
    assert not torch.equal(first[0][0], first[64][0])  # a new epoch: another permutation and other masks
    # two ranks of world 2 at batch 16 hold world 1's global batch of 32, ordinals included
    for t in (3, 70):
        whole = one.plan(t)
        halves = [TokenLoader(ds, "train", "cpu", 16, 32, max_predictions=12, seed=5, rank=r, world=2) for r in (0, 1)]
        plans = [h.plan(t) for h in halves]
        assert np.array_equal(np.concatenate([p["table"] for p in plans]), whole["table"])
        assert np.array_equal(np.concatenate([p["nsp"] for p in plans]), whole["nsp"])
        assert np.array_equal(whole["table"][:, 5], t * 32 + np.arange(32))
        got = [h.batch(t) for h in halves]
        for k in range(6):
            assert torch.equal(torch.cat([got[0][k], got[1][k]]), one.batch(t)[k])
    from k8s_amd.data import sampler

    for t, r in ((0, 0), (129, 1), (64, 0)):  # the image sampler's epochs and permutations
        assert np.array_equal(ts.train_items(5, t, r, 2, 16, 2057)[0], sampler.batch_indices(5, t, r, 2, 16, 2057))
    # an epoch of anchors is a permutation of the segments (minus the dropped partial batch)
    seg = ds.split("train").segments
    anchors = np.concatenate([one.plan(t)["table"][:, 0] for t in range(64)])
    assert len(set(anchors.tolist())) == 64 * 32 and set(anchors.tolist()) <= set(seg[:-1].tolist())


def test_next_sentence_rule(toy):
    ds = open_token_dataset(toy, pairs=True)
    sp = ds.split("train")
    seg, docs = sp.segments, sp.docs
    anchors = np.arange(sp.G, dtype=np.int64)
    tab, nsp, lens = ts.pair_rows(seg, docs, anchors, anchors + 10 ** 6, seed=9, S=64, P=12)
    doc_of = lambda s: np.searchsorted(docs, s, side="right") - 1  # noqa: E731
    a_doc = doc_of(anchors)
    b_seg = np.searchsorted(seg, tab[:, 2], side="right") - 1
    assert np.array_equal(seg[b_seg], tab[:, 2])  # B starts a segment
    assert np.array_equal(b_seg[nsp == 0], anchors[nsp == 0] + 1)
    assert bool((doc_of(b_seg[nsp == 0]) == a_doc[nsp == 0]).all())
    assert bool((doc_of(b_seg[nsp == 1]) != a_doc[nsp == 1]).all())  # never A's own document
    last = np.isin(anchors + 1, docs)  # the anchor ends its document
    assert bool((nsp[last] == 1).all()) and 0 < nsp[~last].mean() < 1
    # u < 1/2 among the anchors that have a next segment: within 4 sigma of one half
    k = int((~last).sum())
    assert abs((nsp[~last] == 0).mean() - 0.5) < 4 * math.sqrt(0.25 / k)
    assert np.array_equal(lens, tab[:, 1] + tab[:, 3] + 3) and lens.max() <= 64
    # at S = 16 most pairs are truncated to exactly S - 3 tokens by the rule
    short = ts.pair_rows(seg, docs, anchors, anchors, seed=9, S=16, P=12)[0]
    full = ts.pair_rows(seg, docs, anchors, anchors, seed=9, S=64, P=12)[0]
    assert np.array_equal(short[:, [0, 2]], full[:, [0, 2]])
    for (la, lb), (fa, fb) in zip(short[:, [1, 3]].tolist(), full[:, [1, 3]].tolist()):
        assert (la, lb) == ts.truncate_pair(fa, fb, 13)


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.fixture(scope="module")
def big_batch(toy):
    """About 10^5 selected tokens of the toy set: (table, outputs, unmasked tokens)."""
    ds = open_token_dataset(toy, pairs=True)
    sp = ds.split("train")
    reps = 17  # 17 passes over the 2057 anchors, each with ordinals of its own
    anchors = np.tile(np.arange(sp.G, dtype=np.int64), reps)
    tab, _, _ = ts.pair_rows(sp.segments, sp.docs, anchors, np.arange(len(anchors)), seed=3, S=32, P=12)
    src = torch.from_numpy(np.array(sp.tokens).view(np.int16))
    table = torch.from_numpy(tab)
    out = ref.mlm_batch(src, table, 32, 12, 512, ds.special, 3)
    plain = ref.mlm_batch(src, torch.cat([table[:, :4], torch.ones(len(table), 1, dtype=torch.int64), table[:, 5:]], 1),
                          32, 12, 512, ds.special, 3)
    tok = plain[0].clone()  # n = 1: undo the one selected position to get the unmasked row
    tok[torch.arange(len(tok)), plain[3][:, 0]] = plain[2][:, 0]
    return table, out, tok


def test_oracle_invariants(big_batch):
    table, (ids, types, labels, positions), tok = big_batch
    N = len(table)
    la, lb, n = table[:, 1], table[:, 3], table[:, 4]
    used = labels != -100
    assert torch.equal(used.sum(1), n)  # exactly n labels
    slot = torch.arange(12).unsqueeze(0)
    assert torch.equal(used, slot < n.unsqueeze(1))  # in the first n slots
    assert bool((positions[~used] == 0).all())
    pos = torch.where(used, positions, torch.full_like(positions, 10 ** 6))
    assert bool((pos[:, 1:] > pos[:, :-1])[used[:, 1:]].all())  # strictly ascending
    j = positions
    special = (j == 0) | (j == la.unsqueeze(1) + 1) | (j >= (la + lb).unsqueeze(1) + 2)
    assert not bool(special[used].any())  # never [CLS], a [SEP] or padding
    assert torch.equal(labels[used], tok.gather(1, positions)[used])  # labels are the unmasked tokens
    sel = torch.zeros(N, 32, dtype=torch.bool)
    sel[torch.arange(N).unsqueeze(1).expand(N, 12)[used], positions[used]] = True
    assert torch.equal(ids[~sel], tok[~sel])  # unselected ids unchanged
    L = (la + lb + 3).unsqueeze(1)
    col = torch.arange(32).unsqueeze(0)
    assert bool((tok[:, 0] == 1).all()) and bool((tok[col >= L] == 0).all())
    assert torch.equal(types, ((col >= la.unsqueeze(1) + 2) & (col < L)).long())


def test_mask_random_keep_shares(big_batch):
    table, (ids, _, labels, positions), tok = big_batch
    used = labels != -100
    k = int(used.sum())
    assert k > 9 * 10 ** 4
    new, old = ids.gather(1, positions)[used], labels[used]
    masked = float((new == 3).sum()) / k  # the toy set holds no id 3, and a random id is 3 once in 512
    kept = float((new == old).sum()) / k  # includes the random ids that hit the old one: 0.1 / 512
    other = float(((new != 3) & (new != old)).sum()) / k
    for share, p in ((masked, 0.8 + 0.1 / 512), (kept, 0.1 + 0.1 / 512), (other, 0.1 - 0.2 / 512)):
        assert abs(share - p) < 4 * math.sqrt(p * (1 - p) / k), (share, p, k)
    rnd = new[(new != 3) & (new != old)]
    assert int(rnd.min()) < 8 and int(rnd.max()) >= 8 + 8 * 63 - 8  # uniform over the whole vocabulary, not the topic


def test_val_batch_is_fixed_and_differs_from_the_training_stream(toy):
    ds = open_token_dataset(toy, need=("train", "val"), pairs=True)
    a = TokenLoader(ds, "val", "cpu", 16, 32, max_predictions=12, seed=2, train=False).batch(1)
    b = TokenLoader(ds, "val", "cpu", 16, 32, max_predictions=12, seed=2, train=False)
    b.batch(0)
    assert all(torch.equal(x, y) for x, y in zip(a, b.batch(1)))
    sp = ds.split("val")
    src = torch.from_numpy(np.array(sp.tokens).view(np.int16))
    table = torch.from_numpy(ts.pair_rows(sp.segments, sp.docs, np.arange(16, 32), np.arange(16, 32), 2, 32, 12, 1)[0])
    s1 = ref.mlm_batch(src, table, 32, 12, 512, ds.special, 2, stream=1)
    s0 = ref.mlm_batch(src, table, 32, 12, 512, ds.special, 2, stream=0)
    assert all(torch.equal(x, y) for x, y in zip(s1, (a[0], a[1], a[2], a[4])))
    assert not torch.equal(s1[3], s0[3])
    # past the end: 249 segments, batch 15 of 16 holds 9 real rows
    ids, _, labels, nsp, _, lens = TokenLoader(ds, "val", "cpu", 16, 32, max_predictions=12, train=False).batch(15)
    assert bool((labels[9:] == -100).all()) and bool((nsp[9:] == -100).all()) and bool((nsp[:9] >= 0).all())
    assert bool((labels[:9] != -100).any(1).all()) and lens.dtype == torch.int32


def test_reference_rejects_bad_rows(toy):
    src = torch.arange(100, dtype=torch.int32)
    ok = [10, 5, 50, 6, 2, 0]
    ref.mlm_batch(src, torch.tensor([ok]), 32, 12, 512, (0, 1, 2, 3), 0)
    for col, v in ((1, 0), (3, 0), (1, 30), (0, 96), (2, -1), (4, 0), (4, 13), (4, 12), (5, -1)):
        row = list(ok)
        row[col] = v
        with pytest.raises(ValueError):
            ref.mlm_batch(src, torch.tensor([row]), 32, 12, 512, (0, 1, 2, 3), 0)
    with pytest.raises(ValueError):
        ref.mlm_batch(src, torch.tensor([ok]), 513, 12, 512, (0, 1, 2, 3), 0)
    with pytest.raises(ValueError):
        ref.causal_batch(src, torch.tensor([36]), 64)
    ids, labels = ref.causal_batch(src, torch.tensor([35, 0]), 64)
    assert labels[0, -1] == 99 and torch.equal(ids[1], torch.arange(64))


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


@pytest.mark.parametrize("accum", [1, 2])
def test_bert_resume_gives_the_uninterrupted_run(toy, tmp_path, accum):
    common = ["--model", "bert_tiny", "--data-dir", toy, "--batch", "8", "--dropout", "0.1", "--log-every", "1",
              "--accum-steps", str(accum)]
    p, ev = _trainer(common + ["--steps", "6"])
    assert p.returncode == 0, p.stderr[-1500:]
    whole = [e for e in ev if e.get("event") == "done"][-1]
    start = [e for e in ev if e.get("event") == "start"][-1]["data"]
    assert start["kind"] == "tokens" and start["train"] == {"tokens": 16457, "segments": 2057, "documents": 512}
    assert start["steps_per_epoch"] == 2057 // 8 and start["resident"] is False and start["seq"] == 32
    assert 0.2 < start["pad_fraction"] < 0.7
    assert all(e["epoch"] == 0 for e in ev if e.get("event") == "step")
    ck = str(tmp_path / "ckpt")
    p, _ = _trainer(common + ["--steps", "3", "--ckpt-dir", ck])
    assert p.returncode == 0, p.stderr[-1500:]
    p, ev = _trainer(common + ["--steps", "6", "--ckpt-dir", ck])
    assert p.returncode == 0, p.stderr[-1500:]
    assert [e for e in ev if e.get("event") == "restored"][-1]["step"] == 2
    resumed = [e for e in ev if e.get("event") == "done"][-1]
    assert resumed["weights_sum"] == whole["weights_sum"] and resumed["loss"] == whole["loss"]


def test_llama_trains_and_evaluates_the_split_once(toy):
    p, ev = _trainer(["--model", "llama_tiny", "--data-dir", toy, "--batch", "8", "--steps", "3", "--eval-every", "3",
                      "--eval-batches", "50"])
    assert p.returncode == 0, p.stderr[-1500:]
    e = [x for x in ev if x.get("event") == "eval"][-1]
    assert e["examples"] == ((2053 - 1) // 64) * 64 and math.isfinite(e["loss"]) and e["perplexity"] > 1
    assert math.isfinite([x for x in ev if x.get("event") == "done"][-1]["loss"])


def test_bert_generous_eval_batches_evaluate_the_split_once(toy):
    args = ["--model", "bert_tiny", "--data-dir", toy, "--batch", "8", "--steps", "1", "--eval-every", "1",
            "--eval-batch", "16"]
    p, ev = _trainer(args + ["--eval-batches", "16"])  # 256 rows for 249 segments
    assert p.returncode == 0, p.stderr[-1500:]
    exact = [x for x in ev if x.get("event") == "eval"][-1]
    p, ev = _trainer(args + ["--eval-batches", "40"])  # 24 batches without one real row
    assert p.returncode == 0, p.stderr[-1500:]
    generous = [x for x in ev if x.get("event") == "eval"][-1]
    assert math.isfinite(generous["loss"]) and generous["examples"] == exact["examples"] > 249
    assert generous["loss"] == exact["loss"]


CONFIG_ERRORS = {
    "resnet_on_tokens": (None, ["--model", "resnet_tiny"]),
    "bert_on_images": ("images", ["--model", "bert_tiny"]),
    "llama_on_images": ("images", ["--model", "llama_tiny"]),
    "augment": (None, ["--model", "bert_tiny", "--augment", "crop"]),
    "crop_pad": (None, ["--model", "bert_tiny", "--crop-pad", "4"]),
    "image": (None, ["--model", "llama_tiny", "--image", "32"]),
    "graph": (None, ["--model", "bert_tiny", "--graph"]),
    "eval_data_train": (None, ["--model", "bert_tiny", "--eval-every", "2", "--eval-data", "train"]),
    "every_token_head": (None, ["--model", "bert_tiny", "--mlm-head", "every-token"]),
    "seq_above_max_position": (None, ["--model", "bert_tiny", "--seq", "129"]),
    "seq_above_512": (None, ["--model", "bert_base", "--seq", "513"]),
    "llama_seq_above_max_position": (None, ["--model", "llama_tiny", "--seq", "257"]),
    "no_whole_batch": (None, ["--model", "bert_tiny", "--batch", "4096"]),
    "llama_no_whole_batch": (None, ["--model", "llama_tiny", "--batch", "512"]),
    "vocab_above_model": ("vocab_1001", ["--model", "bert_tiny"]),
    "one_document": ("one_document", ["--model", "bert_tiny"]),
    "no_val_split": ("no_val", ["--model", "llama_tiny", "--eval-every", "2"]),
    "token_outside_vocab": ("token_outside_vocab", ["--model", "llama_tiny"]),
}


@pytest.mark.parametrize("case", sorted(CONFIG_ERRORS))
def test_configuration_error_exits_1_with_one_sentence(toy, image_toy, tmp_path, case):
    kind, args = CONFIG_ERRORS[case]
    if kind == "images":
        path = image_toy
    elif kind == "vocab_1001":
        path = str(tmp_path / kind)
        make_dataset.make_toy_tokens(path, train_docs=8, val_docs=2, vocab=1001)
    elif kind == "no_val":
        path = str(tmp_path / kind)
        shutil.copytree(toy, path)
        os.remove(os.path.join(path, "val_tokens.npy"))
    else:
        path = _variant(toy, tmp_path, kind) if kind else toy
    p, events = _trainer(["--data-dir", path, "--steps", "2"] + args)
    assert p.returncode == 1, p.stdout[-1500:] + p.stderr[-1500:]
    errors = [line for line in p.stderr.splitlines() if line.startswith("error: ")]
    assert len(errors) == 1 and "Traceback" not in p.stderr, p.stderr[-1500:]
    assert not [e for e in events if e.get("event") in ("step0", "done")]


# Held-out loss (MLM + NSP, on the 249 val pairs) after the 300 steps below, through the trainer on the CPU (fp32),
# seeds 0, 1, 2: 4.3779, 4.2069, 4.1968. Chance is ln 504 + ln 2 = 6.9156 (uniform over the 504 non-special ids, plus
# a coin); the threshold lies halfway between chance and the worst of the three. All three runs also pass below
# ln 63 + ln 2 = 4.8363, what a model that only knows the topic can reach.
CPU_EVAL_LOSS = (4.3779, 4.2069, 4.1968)
CHANCE = math.log(504) + math.log(2)
CPU_THRESHOLD = (CHANCE + max(CPU_EVAL_LOSS)) / 2


def test_bert_learns_the_toy_tokens(toy):
    p, ev = _trainer(["--model", "bert_tiny", "--data-dir", toy, "--batch", "32", "--lr", "0.001", "--steps", "300",
                      "--eval-every", "300", "--eval-batches", "8"])
    assert p.returncode == 0, p.stderr[-1500:]
    e = [x for x in ev if x.get("event") == "eval"][-1]
    print("cpu toy tokens eval loss %.4f (examples %d)" % (e["loss"], e["examples"]))
    assert e["data"] == "heldout" and e["examples"] > 249
    assert e["loss"] < CPU_THRESHOLD
