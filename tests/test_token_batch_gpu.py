"""The fused token batch kernels, the token loader's modes and training BERT / Llama on a token dataset, on the GPU.

The oracle is ``ops.reference.mlm_batch`` / ``causal_batch`` (torch integer ops, run on the CPU): the kernels are
integer arithmetic and must match it bit for bit, so every comparison is ``torch.equal``.

Ties between scores: within a row ``score[j] = mix32(ksel ^ (j * G))`` is injective in ``j`` -- ``G`` is odd, so
``j -> j * G mod 2^32`` is a bijection, xor with a constant is one, and ``mix32`` (xor-shifts and odd multipliers) is
one. Two positions of a row therefore never share a score and the (score, position) tie-break never decides an output;
``test_scores_of_a_row_are_distinct`` checks that on the CPU oracle instead of searching for a tied row that cannot
exist."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIAL = (0, 1, 2, 3)
T = 3001  # tokens in the synthetic source
SEED = 0x5EED0123456789


def _src(dtype):
    """[T] tokens: uint16 data with ids above 32767 (as the int16 view the ops take), or int32 ids up to 2^31 - 2."""
    g = torch.Generator().manual_seed(11)
    if dtype == "uint16":
        v = torch.randint(0, 65536, (T,), generator=g)
        v[::7] = 65535 - torch.arange(len(v[::7]))  # the top of the range is present whatever the draw
        return torch.from_numpy(v.numpy().astype(np.uint16).view(np.int16)), 65536
    v = torch.randint(0, 2 ** 31 - 1, (T,), generator=g, dtype=torch.int64)
    v[::7] = 2 ** 31 - 2 - torch.arange(len(v[::7]))
    return v.to(torch.int32), 2 ** 31 - 1


def _table(S, P):
    """Five rows (the last block of four waves is partial): an exact fill, la = lb = 1 with n = 1, n == P, every
    candidate selected, and segments that end exactly at the last token."""
    from k8s_amd.data.token_sampler import n_predictions

    la = (S - 3) // 2
    lb = S - 3 - la
    wide = (P - P // 2 + 2, P // 2 + 3)  # la + lb = P + 5 <= S - 3 for every (S, P) below
    few = (3, min(P, 7) - 3)
    rows = [
        (5, la, 900, lb, n_predictions(S, P, la + lb), 0),
        (17, 1, 40, 1, 1, 1),
        (100, wide[0], 333, wide[1], P, 2 ** 33 + 5),
        (2000, few[0], 50, few[1], few[0] + few[1], 3),
        (T - 9, 9, T - 6, 6, n_predictions(18, P, 15), 2 ** 40),
    ]
    return torch.tensor(rows, dtype=torch.int64)


def _equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and g.shape == w.shape
        assert torch.equal(g.cpu(), w)


# ------------------------------------------------------------------------------------------------ mlm_batch
@pytest.mark.parametrize("dtype", ["uint16", "int32"])
@pytest.mark.parametrize("P", [12, 20])
@pytest.mark.parametrize("S", [32, 64, 96, 128, 512])
def test_mlm_batch_matches_the_oracle(cuda, S, P, dtype):
    from k8s_amd.ops import data as kdata
    from k8s_amd.ops import reference as ref

    src, vocab = _src(dtype)
    table = _table(S, P)
    for stream in (0, 1):
        want = ref.mlm_batch(src, table, S, P, vocab, SPECIAL, SEED, stream)
        got = kdata.mlm_batch(src.to(cuda), table, S, P, vocab, SPECIAL, SEED, stream)
        _equal(got, want)
    labels = want[2]
    assert ((labels != -100).sum(1) == table[:, 4]).all()  # exactly n labels per row
    if dtype == "uint16":
        assert int(want[0].max()) > 32767 and int(want[0].min()) >= 0  # read unsigned


def test_mlm_batch_every_slot_and_many_blocks(cuda):
    """P = S (labels as wide as the row) and 67 samples (17 blocks, the last with three waves)."""
    from k8s_amd.ops import data as kdata
    from k8s_amd.ops import reference as ref

    src, vocab = _src("uint16")
    g = np.random.default_rng(3)
    S = 96
    la, lb = g.integers(1, 46, size=67), g.integers(1, 46, size=67)
    n = np.minimum(np.maximum(1, (3 * (la + lb + 3) + 10) // 20), la + lb)
    table = torch.from_numpy(np.stack([g.integers(0, T - 46, size=67), la, g.integers(0, T - 46, size=67), lb, n,
                                       np.arange(67) + 1000], axis=1).astype(np.int64))
    _equal(kdata.mlm_batch(src.to(cuda), table, S, S, vocab, SPECIAL, 7), ref.mlm_batch(src, table, S, S, vocab,
                                                                                       SPECIAL, 7))


def test_scores_of_a_row_are_distinct():
    """See the module docstring: no row holds two equal scores, so the position tie-break never decides."""
    from k8s_amd.ops import reference as ref

    s = ref.mlm_scores(SEED, 0, torch.arange(4096), 512).sort(dim=1).values
    assert bool((s[:, 1:] != s[:, :-1]).all())


# ------------------------------------------------------------------------------------------------ causal_batch
@pytest.mark.parametrize("dtype", ["uint16", "int32"])
@pytest.mark.parametrize("S", [64, 100])
def test_causal_batch_matches_the_oracle(cuda, S, dtype):
    from k8s_amd.ops import data as kdata
    from k8s_amd.ops import reference as ref

    src, _ = _src(dtype)
    starts = torch.tensor([0, S, 7, T - S - 1, 1234, 5 * S], dtype=torch.int64)  # one window ends at token T - 1
    want = ref.causal_batch(src, starts, S)
    _equal(kdata.causal_batch(src.to(cuda), starts, S), want)
    v = src.to(torch.int64) & 0xFFFF if dtype == "uint16" else src.to(torch.int64)
    assert torch.equal(want[0][3], v[T - S - 1:T - 1]) and torch.equal(want[1][3], v[T - S:T])


# ------------------------------------------------------------------------------------------------ binding checks
def _ok_args(cuda):
    src, vocab = _src("uint16")
    return dict(src=src.to(cuda), table=_table(64, 12), S=64, P=12, vocab=vocab, special=SPECIAL, seed=1)


def _row(col, value, row=1):
    def change(a):
        a["table"] = a["table"].clone()
        a["table"][row, col] = value
    return change


BAD_CALLS = {
    "src_dtype": lambda a: a.update(src=a["src"].to(torch.int64)),
    "src_shape": lambda a: a.update(src=a["src"].view(-1, 1)),
    "table_dtype": lambda a: a.update(table=a["table"].to(torch.int32)),
    "table_shape": lambda a: a.update(table=a["table"][:, :5].contiguous()),
    "table_on_gpu": lambda a: a.update(table=a["table"].to(a["src"].device)),
    "S_zero": lambda a: a.update(S=0),
    "S_above_512": lambda a: a.update(S=513),
    "P_zero": lambda a: a.update(P=0),
    "P_above_S": lambda a: a.update(P=65),
    "la_zero": _row(1, 0),
    "lb_zero": _row(3, 0),
    "row_too_long": _row(1, 61),
    "a_before_src": _row(0, -1),
    "a_past_src": _row(0, T),
    "b_past_src": _row(2, T - 0),
    "b_before_src": _row(2, -5),
    "n_zero": _row(4, 0),
    "n_above_P": _row(4, 13, row=0),
    "n_above_candidates": _row(4, 3),
    "ord_negative": _row(5, -1),
    "special_outside_vocab": lambda a: a.update(special=(0, 1, 2, 65536)),
    "vocab_one": lambda a: a.update(vocab=1),
    "vocab_2_31": lambda a: a.update(vocab=2 ** 31),
    "uint16_vocab": lambda a: a.update(vocab=65537),
}


@pytest.mark.parametrize("case", sorted(BAD_CALLS))
def test_bad_call_raises_before_any_launch(cuda, case):
    from k8s_amd.ops import data as kdata

    a = _ok_args(cuda)
    BAD_CALLS[case](a)
    before = kdata.token_launches()
    with pytest.raises((RuntimeError, TypeError)):
        kdata.mlm_batch(**a)
    assert kdata.token_launches() == before


def test_bad_causal_call_raises_before_any_launch(cuda):
    from k8s_amd.ops import data as kdata

    src = _src("int32")[0].to(cuda)
    before = kdata.token_launches()
    for starts in ([-1], [T - 64], [0, T]):
        with pytest.raises(RuntimeError):
            kdata.causal_batch(src, torch.tensor(starts, dtype=torch.int64), 64)
    with pytest.raises(RuntimeError):
        kdata.causal_batch(src, torch.tensor([0], dtype=torch.int32), 64)
    assert kdata.token_launches() == before
    kdata.causal_batch(src, torch.tensor([T - 65], dtype=torch.int64), 64)
    assert kdata.token_launches() == before + 1


# ------------------------------------------------------------------------------------------------ loader
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from k8s_amd.tools.make_dataset import make_toy_tokens

    path = str(tmp_path_factory.mktemp("toytokens"))
    make_toy_tokens(path)
    return path


@pytest.mark.parametrize("kind", ["bert", "llama"])
def test_loader_resident_streamed_and_cpu_give_the_same_bits(cuda, toy, kind):
    from k8s_amd.data import open_token_dataset
    from k8s_amd.data.token_loader import TokenLoader

    ds = open_token_dataset(toy, need=("train", "val"), pairs=True)
    # (split, train, batch index): a training batch of the second epoch; the val batch that runs past the split's end
    last = {"bert": ds.split("val").G // 16, "llama": ((ds.split("val").T - 1) // 48) // 16}[kind]
    for split, train, t in (("train", True, 70), ("val", False, last)):
        kw = dict(batch=16, seq=48, kind=kind, max_predictions=12, seed=4, rank=1 if train else 0,
                  world=2 if train else 1, train=train)
        cpu = TokenLoader(ds, split, "cpu", **kw)
        res = TokenLoader(ds, split, cuda, resident_gb=4.0, **kw)
        stream = TokenLoader(ds, split, cuda, resident_gb=0.0, **kw)
        try:
            assert res.resident and not stream.resident and stream.streamer is not None
            want = cpu.batch(t)
            for ld in (res, stream):
                got = ld.batch(t)
                assert len(got) == len(want)
                for g, w in zip(got, want):
                    assert g.is_cuda and g.dtype == w.dtype and torch.equal(g.cpu(), w)
            _ = stream.batch(t + 1), stream.batch(t)  # the prefetched batch, then a restart
            for g, w in zip(stream.batch(t), want):
                assert torch.equal(g.cpu(), w)
            if not train:
                labels = want[2] if kind == "bert" else want[1]
                real = (labels != -100).any(1)
                assert 0 < int(real.sum()) < 16 and not bool(real[int(real.sum()):].any())
        finally:
            stream.close()


# ------------------------------------------------------------------------------------------------ trainer
def _trainer(args):
    r = subprocess.run([sys.executable, "-m", "k8s_amd.trainer", "--device", "cuda"] + args, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def test_bert_trains_on_tokens_on_the_fused_paths(cuda, toy):
    ev = _trainer(["--model", "bert_tiny", "--data-dir", toy, "--batch", "16", "--seq", "128", "--dropout", "0.1",
                   "--steps", "4", "--log-every", "1", "--eval-every", "4", "--eval-batches", "2"])
    done = [e for e in ev if e.get("event") == "done"][-1]
    start = [e for e in ev if e.get("event") == "start"][-1]
    print("bert done:", done)
    assert start["data"]["kind"] == "tokens" and start["data"]["resident"] is True
    assert 0.5 < start["data"]["pad_fraction"] < 1.0
    assert done["dropout_fallbacks"] == 0 and done["gemm_fallbacks"] == {}
    e = [x for x in ev if x.get("event") == "eval"][-1]
    assert np.isfinite(e["loss"]) and e["examples"] > 0 and np.isfinite(done["loss"])


def test_llama_trains_on_tokens_on_the_fused_paths(cuda, toy):
    ev = _trainer(["--model", "llama_tiny", "--data-dir", toy, "--batch", "8", "--steps", "4", "--log-every", "1",
                   "--eval-every", "4", "--eval-batches", "8"])
    done = [e for e in ev if e.get("event") == "done"][-1]
    print("llama done:", done)
    assert done["gemm_fallbacks"] == {} and np.isfinite(done["loss"])
    e = [x for x in ev if x.get("event") == "eval"][-1]
    assert np.isfinite(e["loss"]) and e["examples"] == 32 * 64  # the 32 whole windows of the val split, once
