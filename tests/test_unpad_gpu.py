"""Unpadded BERT on the GPU: the SPAN forms of the flash kernels against the fp32 reference on both tile widths, no
leak across a span edge bit for bit, the packed path, the calls that keep the mask outside the flash contract and the
binding's rejections; the ``mlm_batch_unpadded`` kernel against its torch definition (integer arithmetic:
``torch.equal``), the loader's three paths, a ``bert_tiny`` unpadded step against the fp32 CPU model and a trainer
run."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from k8s_amd.ops import attention as kattn
from k8s_amd.ops.attention import _Flash, attention, attention_qkv, attention_reference, span_bounds

pytestmark = pytest.mark.gpu


def _close(a, b, tol, what):  # tests/test_doc_mask_gpu.py's measure and tolerances
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    assert err <= tol * max(1.0, scale), "%s: max err %g (scale %g)" % (what, err, scale)


def _lo_rows(S, rows):
    """int64 [B, S]: every token's span start, from each row's list of span starts."""
    out = torch.empty(len(rows), S, dtype=torch.int64)
    for b, starts in enumerate(rows):
        assert starts[0] == 0 and list(starts) == sorted(set(starts)) and starts[-1] < S
        s = torch.tensor(list(starts))
        out[b] = s[torch.searchsorted(s, torch.arange(S), right=True) - 1]
    return out


CASES = [
    # B, S, Hq, Hkv, span starts per row (D = 64)
    (2, 192, 4, 2, [[0, 1, 2, 63, 64, 65, 130], [0]]),
    (1, 200, 2, 2, [[0, 5, 199]]),
    (1, 1152, 2, 2, [[0, 127, 128, 129, 640, 1151]]),
]
D = 64
# (case, span_tile): every case on the dispatch's default; the S = 1152 one on both tile forms by name
RUNS = [(0, None), (1, None), (2, None), (2, 64), (2, 128)]


@pytest.fixture
def span_tile():
    """Sets ``ops.attention.SPAN_TILE`` (the dispatch's selector) for one test and restores it."""
    saved = kattn.SPAN_TILE

    def use(tile):
        kattn.SPAN_TILE = tile

    yield use
    kattn.SPAN_TILE = saved


def _operands(cuda, B, S, Hq, Hkv, seed=0):
    """q, k, v as column slices of one packed tensor (the models' layout), and dO."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, generator=g).to(cuda).bfloat16()
    do = torch.randn(B, S, Hq, D, generator=g).to(cuda).bfloat16()
    return qkv, do


def _views(qkv, Hq, Hkv):
    B, S = qkv.shape[:2]
    return (qkv[..., :Hq * D].view(B, S, Hq, D), qkv[..., Hq * D:(Hq + Hkv) * D].view(B, S, Hkv, D),
            qkv[..., (Hq + Hkv) * D:].view(B, S, Hkv, D))


def _flash(qkv, do, Hq, Hkv, span, tile):
    """(O, lse, dQ, dK, dV) of the flash path."""
    from k8s_amd.ops._ext import load

    q, k, v = _views(qkv, Hq, Hkv)
    scale = 1.0 / math.sqrt(D)
    kw = dict(span_lo=span[0], span_hi=span[1], span_tile=tile)
    o, lse = load().flash_fwd(q, k, v, False, None, scale, **kw)
    dq, dk, dv = load().flash_bwd(do, q, k, v, o, lse, False, None, scale, **kw)
    return o, lse[..., :qkv.shape[1]], dq, dk, dv


@pytest.mark.parametrize("case,tile", RUNS)
def test_flash_span_fwd_bwd(cuda, span_tile, case, tile):
    B, S, Hq, Hkv, rows = CASES[case]
    span_tile(tile)
    qkv, do = _operands(cuda, B, S, Hq, Hkv)
    lo, hi = span_bounds(_lo_rows(S, rows))
    span = (lo.to(cuda), hi.to(cuda))
    q, k, v = _views(qkv, Hq, Hkv)
    scale = 1.0 / math.sqrt(D)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    want = attention_reference(qr, kr, vr, False, None, scale, span_lo=span[0], span_hi=span[1])
    want.backward(do.float())
    qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = attention(qq, kk, vv, causal=False, span=span)
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith(_Flash.__name__)
    _close(out, want, 2e-2, "O")
    out.backward(do)
    _close(qq.grad, qr.grad, 3e-2, "dQ")
    _close(kk.grad, kr.grad, 3e-2, "dK")
    _close(vv.grad, vr.grad, 3e-2, "dV")
    # the mask is in force: the unmasked call differs from the masked reference wherever a row holds two spans
    plain = _Flash.apply(q, k, v, False, None, scale)
    for b, r in enumerate(rows):
        if len(r) > 1:
            assert (plain[b].float() - want[b].float()).abs().max().item() > 0.1


def test_span_tile_default_is_64(cuda):
    from k8s_amd.ops._ext import load

    assert kattn.SPAN_TILE is None
    assert all(load().flash_span_tile(S) == 64 for S in (128, 1152, 131072))


@pytest.mark.parametrize("case,index,tile", [(0, 5, 0), (0, 3, 0), (2, 4, 64), (2, 3, 64), (2, 4, 128), (2, 1, 128)])
def test_flash_span_no_leak(cuda, case, index, tile):
    """Replacing q, k, v and dO of every token outside one span leaves that span's O, lse, dQ, dK and dV unchanged bit
    for bit: masked scores are overwritten before the max, and p = 0 times a finite value adds nothing."""
    B, S, Hq, Hkv, rows = CASES[case]
    starts = rows[0]
    a, b = starts[index], (starts[index + 1] if index + 1 < len(starts) else S)
    lo, hi = span_bounds(_lo_rows(S, rows))
    span = (lo.to(cuda), hi.to(cuda))
    qkv, do = _operands(cuda, B, S, Hq, Hkv, seed=1)
    first = _flash(qkv, do, Hq, Hkv, span, tile)
    qkv2, do2 = _operands(cuda, B, S, Hq, Hkv, seed=2)
    qkv2, do2 = qkv2 * 8, do2 * 8  # other finite values (no inf: 0 * inf is NaN)
    qkv2[0, a:b], do2[0, a:b] = qkv[0, a:b], do[0, a:b]
    second = _flash(qkv2, do2, Hq, Hkv, span, tile)
    for name, x, y in zip(("O", "lse", "dQ", "dK", "dV"), first, second):
        sel = (lambda t: t[0, :, a:b]) if name == "lse" else (lambda t: t[0, a:b])
        assert torch.isfinite(sel(x).float()).all(), name
        assert torch.equal(sel(x), sel(y)), name


def test_attention_qkv_span_packed_matches_split(cuda):
    """attention_qkv with a span mask against the fp32 split + reference composition, forward and the packed
    gradient."""
    torch.manual_seed(7)
    B, S, H, Hkv = 2, 320, 8, 2
    W = (H + 2 * Hkv) * D
    lo, hi = span_bounds(_lo_rows(S, [[0, 100, 101, 256], [0, 64, 300]]))
    lo, hi = lo.to(cuda), hi.to(cuda)
    qkv = (torch.randn(B * S, W, device=cuda) * 0.5).bfloat16().requires_grad_(True)
    o = attention_qkv(qkv, B, S, H, Hkv, D, causal=False, span=(lo, hi))
    assert type(o.grad_fn).__name__.startswith(kattn._FlashQKV.__name__)
    go = torch.randn_like(o)
    (g,) = torch.autograd.grad(o, qkv, go)

    xr = qkv.detach().float().requires_grad_(True)
    q, k, v = xr.split([H * D, Hkv * D, Hkv * D], dim=-1)
    want = attention_reference(q.reshape(B, S, H, D), k.reshape(B, S, Hkv, D), v.reshape(B, S, Hkv, D), False,
                               span_lo=lo, span_hi=hi)
    (gr,) = torch.autograd.grad(want, xr, go.float())
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()  # noqa: E731
    assert rel(o, want) < 2e-2
    assert rel(g, gr) < 3e-2


def test_span_mask_outside_flash_contract_keeps_the_mask(cuda):
    """fp32 operands and head_dim 128 run the reference with the mask, not without it."""
    torch.manual_seed(3)
    B, S, H = 1, 48, 2
    lo, hi = (t.to(cuda) for t in span_bounds(_lo_rows(S, [[0, 20]])))
    for d, dtype in ((32, torch.float32), (128, torch.bfloat16)):
        q, k, v = (torch.randn(B, S, H, d, device=cuda).to(dtype) for _ in range(3))
        out = attention(q, k, v, causal=False, span=(lo, hi))
        want = attention_reference(q, k, v, False, span_lo=lo, span_hi=hi)
        assert torch.equal(out, want)
        assert (out.float() - attention(q, k, v, causal=False).float()).abs().max().item() > 1e-2
    # the packed entry at head_dim 128 takes the split composition, mask included
    W = 3 * H * 128
    qkv = torch.randn(B * S, W, device=cuda).bfloat16()
    out = attention_qkv(qkv, B, S, H, H, 128, causal=False, span=(lo, hi))
    q, k, v = (t.reshape(B, S, H, 128) for t in qkv.split(H * 128, dim=-1))
    assert torch.equal(out, attention_reference(q, k, v, False, span_lo=lo, span_hi=hi))


def test_span_rejected_combinations(cuda):
    from k8s_amd.ops._ext import load

    B, S, H = 1, 128, 2
    q, k, v = (torch.randn(B, S, H, D, device=cuda).bfloat16() for _ in range(3))
    lo, hi = (t.to(cuda) for t in span_bounds(_lo_rows(S, [[0, 50]])))
    lens = torch.tensor([100], device=cuda, dtype=torch.int32)
    C = load()
    for kw in (dict(span_lo=lo), dict(span_hi=hi),  # one table alone
               dict(span_lo=lo.long(), span_hi=hi.long()),  # dtype
               dict(span_lo=lo[:, :64].contiguous(), span_hi=hi[:, :64].contiguous()),  # shape
               dict(span_lo=lo.cpu(), span_hi=hi.cpu()),  # host tables
               dict(span_lo=lo, span_hi=hi, span_tile=32), dict(span_tile=64),  # tile
               dict(span_lo=lo, span_hi=hi, doc_lo=lo, doc_hi=hi)):
        with pytest.raises(RuntimeError):
            C.flash_fwd(q, k, v, False, None, 0.125, **kw)
    with pytest.raises(RuntimeError):
        C.flash_fwd(q, k, v, True, None, 0.125, span_lo=lo, span_hi=hi)  # causal
    with pytest.raises(RuntimeError):
        C.flash_fwd(q, k, v, False, lens, 0.125, span_lo=lo, span_hi=hi)  # kv_lens
    with pytest.raises(RuntimeError):
        C.flash_fwd(q, k[:, :64], v[:, :64], False, None, 0.125, span_lo=lo, span_hi=hi)  # Sq != Sk
    q128 = torch.randn(B, S, H, 128, device=cuda).bfloat16()
    with pytest.raises(RuntimeError):
        C.flash_fwd(q128, q128, q128, False, None, 0.125, span_lo=lo, span_hi=hi)  # head_dim 128
    assert not C.flash_span_ok(64, 1, 1 << 24, 1 << 24, 1, 768)  # the index limits the binding checks
    assert not C.flash_span_ok(64, 1 << 10, 1 << 12, 1 << 12, 1 << 9, 768)
    assert not C.flash_span_ok(64, 1, 128, 128, 2, 1 << 24)
    assert C.flash_span_ok(64, 1, 131072, 131072, 12, 2304)
    o, lse = C.flash_fwd(q, k, v, False, None, 0.125, span_lo=lo, span_hi=hi)
    x = torch.empty(B * S, 3 * H * D, device=cuda, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):  # no bias gradient with a span mask
        C.flash_bwd(torch.randn_like(o), q, k, v, o, lse, False, None, 0.125, x, torch.zeros(3 * H * D, device=cuda),
                    span_lo=lo, span_hi=hi)
    with pytest.raises(ValueError):
        attention(q, k, v, causal=True, span=(lo, hi))
    with pytest.raises(ValueError):
        attention(q, k, v, causal=False, kv_lens=lens, span=(lo, hi))


# ------------------------------------------------------------------------------------------------ batch kernel
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIAL = (0, 1, 2, 3)
T_SRC = 3001  # tokens in the synthetic source
SEED = 0x5EED0123456789
NAMES = ("ids", "token_types", "pos", "labels", "rows", "cls_rows", "lo", "hi")


def _src(dtype):
    """[T_SRC] tokens: uint16 data with ids above 32767 (as the int16 view the ops take), or int32 ids."""
    g = torch.Generator().manual_seed(11)
    if dtype == "uint16":
        v = torch.randint(0, 65536, (T_SRC,), generator=g)
        v[::7] = 65535 - torch.arange(len(v[::7]))  # the top of the range is present whatever the draw
        return torch.from_numpy(v.numpy().astype(np.uint16).view(np.int16)), 65536
    v = torch.randint(0, 2 ** 31 - 1, (T_SRC,), generator=g, dtype=torch.int64)
    return v.to(torch.int32), 2 ** 31 - 1


def _table(S, P):
    """Five rows (the last block of four waves is partial): an exact fill of the row, la = lb = 1 with n = 1, n == P,
    every candidate selected, and segments that end exactly at the source's last token."""
    la = (S - 3) // 2
    lb = S - 3 - la
    wide = (P - P // 2 + 2, P // 2 + 3)
    rows = [(5, la, 900, lb, min(P, la + lb), 0), (17, 1, 40, 1, 1, 1), (100, wide[0], 333, wide[1], P, 2 ** 33 + 5),
            (2000, 3, 50, 4, 7, 3), (T_SRC - 9, 9, T_SRC - 6, 6, min(P, 3), 2 ** 40)]
    return torch.tensor(rows, dtype=torch.int64)


def _cu(table):
    cu = torch.zeros(table.shape[0] + 1, dtype=torch.int64)
    cu[1:] = (table[:, 1] + table[:, 3] + 3).cumsum(0)
    return cu, (int(cu[-1]) + 127) // 128 * 128


def _equal(got, want):
    assert len(got) == len(want) == 8
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert torch.equal(g.cpu(), w), name


@pytest.mark.parametrize("dtype", ["uint16", "int32"])
@pytest.mark.parametrize("S,P", [(32, 12), (128, 20), (512, 76)])
def test_mlm_batch_unpadded_matches_the_oracle(cuda, S, P, dtype):
    from k8s_amd.ops import data as kdata
    from k8s_amd.ops import reference as ref

    src, vocab = _src(dtype)
    table = _table(S, P)
    cu, T = _cu(table)
    before = kdata.token_launches()
    for stream in (0, 1):
        want = ref.mlm_batch_unpadded(src, table, cu, T, S, P, vocab, SPECIAL, SEED, stream)
        _equal(kdata.mlm_batch_unpadded(src.to(cuda), table, cu, T, S, P, vocab, SPECIAL, SEED, stream), want)
    assert kdata.token_launches() == before + 2  # one launch per batch, the tail included
    assert int(cu[-1]) < T  # these tables leave a tail
    if dtype == "uint16":
        assert int(want[0].max()) > 32767 and int(want[0].min()) >= 0  # read unsigned


def test_mlm_batch_unpadded_without_a_tail(cuda):
    """cu[N] is a multiple of 128: no tail row is written or needed."""
    from k8s_amd.ops import data as kdata
    from k8s_amd.ops import reference as ref

    src, vocab = _src("uint16")
    rows = [(5, 15, 900, 14, 4, 0), (17, 20, 40, 9, 4, 1), (100, 1, 333, 28, 4, 2), (2000, 6, 50, 7, 2, 3),
            (300, 5, 70, 8, 2, 4)]  # L = 32, 32, 32, 16, 16
    table = torch.tensor(rows, dtype=torch.int64)
    cu, T = _cu(table)
    assert int(cu[-1]) == T == 128
    _equal(kdata.mlm_batch_unpadded(src.to(cuda), table, cu, T, 64, 12, vocab, SPECIAL, 3),
           ref.mlm_batch_unpadded(src, table, cu, T, 64, 12, vocab, SPECIAL, 3))


def _ok_args(cuda):
    src, vocab = _src("uint16")
    table = _table(64, 12)
    cu, T = _cu(table)
    return dict(src=src.to(cuda), table=table, cu=cu, T=T, S=64, P=12, vocab=vocab, special=SPECIAL, seed=1)


def _row(col, value, row=1):
    def change(a):
        a["table"] = a["table"].clone()
        a["table"][row, col] = value
    return change


def _cu_at(i, delta):
    def change(a):
        a["cu"] = a["cu"].clone()
        a["cu"][i:] += delta
    return change


BAD_CALLS = {
    # what mlm_batch rejects
    "src_dtype": lambda a: a.update(src=a["src"].to(torch.int64)),
    "table_dtype": lambda a: a.update(table=a["table"].to(torch.int32)),
    "table_on_gpu": lambda a: a.update(table=a["table"].to(a["src"].device)),
    "S_above_512": lambda a: a.update(S=513),
    "P_above_S": lambda a: a.update(P=65),
    "la_zero": _row(1, 0),
    "a_past_src": _row(0, T_SRC),
    "n_above_candidates": _row(4, 3),
    "ord_negative": _row(5, -1),
    "special_outside_vocab": lambda a: a.update(special=(0, 1, 2, 65536)),
    # cu
    "cu_short": lambda a: a.update(cu=a["cu"][:-1].contiguous()),
    "cu_dtype": lambda a: a.update(cu=a["cu"].to(torch.int32)),
    "cu_on_gpu": lambda a: a.update(cu=a["cu"].to(a["src"].device)),
    "cu_first_not_zero": _cu_at(0, 1),
    "cu_difference": _cu_at(2, 1),
    "cu_row_longer_than_table": _row(1, 2),  # the table changes under an unchanged cu
    # T
    "T_below_total": lambda a: a.update(T=a["T"] - 128),
    "T_not_multiple_of_128": lambda a: a.update(T=a["T"] + 1),
    "T_tail_of_a_whole_tile": lambda a: a.update(T=a["T"] + 128),
}


@pytest.mark.parametrize("case", sorted(BAD_CALLS))
def test_bad_unpadded_call_raises_before_any_launch(cuda, case):
    """Host-side rejections: nothing is allocated or launched, and the device is healthy afterwards."""
    from k8s_amd.ops import data as kdata

    a = _ok_args(cuda)
    BAD_CALLS[case](a)
    before = kdata.token_launches()
    with pytest.raises((RuntimeError, TypeError)):
        kdata.mlm_batch_unpadded(**a)
    assert kdata.token_launches() == before
    torch.cuda.synchronize()  # no kernel error follows


# ------------------------------------------------------------------------------------------------ loader
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from k8s_amd.tools.make_dataset import make_toy_tokens

    path = str(tmp_path_factory.mktemp("toytokens"))
    make_toy_tokens(path)
    return path


def test_unpadded_loader_resident_streamed_and_cpu_give_the_same_bits(cuda, toy):
    from k8s_amd.data import open_token_dataset
    from k8s_amd.data.token_loader import TokenLoader

    ds = open_token_dataset(toy, need=("train", "val"), pairs=True)
    last = ds.split("val").G // 16  # the val batch that runs past the split's end
    for split, train, t in (("train", True, 70), ("val", False, last)):
        kw = dict(batch=16, seq=48, kind="bert", max_predictions=12, seed=4, rank=1 if train else 0,
                  world=2 if train else 1, train=train, unpad=True)
        cpu = TokenLoader(ds, split, "cpu", **kw)
        res = TokenLoader(ds, split, cuda, resident_gb=4.0, **kw)
        stream = TokenLoader(ds, split, cuda, resident_gb=0.0, **kw)
        try:
            assert res.resident and not stream.resident and stream.streamer is not None
            want = cpu.batch(t)
            assert len(want) == 9 and want[0].numel() % 128 == 0
            for ld in (res, stream):
                got = ld.batch(t)
                assert len(got) == len(want)
                for g, w in zip(got, want):
                    assert g.is_cuda and g.dtype == w.dtype and torch.equal(g.cpu(), w)
            _ = stream.batch(t + 1), stream.batch(t)  # the prefetched batch, then a restart
            for g, w in zip(stream.batch(t), want):
                assert torch.equal(g.cpu(), w)
            if not train:
                real = (want[3] != -100).any(1)
                assert 0 < int(real.sum()) < 16 and bool((want[4][~real] == -100).all())
        finally:
            stream.close()


# ------------------------------------------------------------------------------------------------ model and trainer
def test_bert_tiny_unpadded_step_matches_cpu_fp32(cuda, toy):
    from k8s_amd.models.registry import build
    from k8s_amd.ops import gemm

    gemm.FALLBACKS.clear()
    data = {"dir": toy, "unpad": True}
    g = build("bert_tiny", cuda, batch=8, seq=128, seed=3, data=data)
    c = build("bert_tiny", "cpu", batch=8, seq=128, seed=3, data=data)
    try:
        batch = g.batch(2)
        assert batch[0].numel() % 128 == 0 and batch[0].numel() < 8 * 128
        lc = c.loss(tuple(t.cpu() for t in batch)).item()
        g.store.begin_step()
        loss = g.loss(batch)
        loss.backward()
        lg = loss.float().item()
        assert abs(lg - lc) < 3e-2 * max(1.0, abs(lc)), (lg, lc)  # tests/test_models_gpu.py's tolerance for BERT
        assert gemm.FALLBACKS == {}, gemm.FALLBACKS
    finally:
        g.close()
        c.close()


def test_bert_trains_unpadded_on_the_fused_paths(cuda, toy):
    r = subprocess.run([sys.executable, "-m", "k8s_amd.trainer", "--device", "cuda", "--model", "bert_tiny",
                        "--data-dir", toy, "--seq", "128", "--unpad", "--steps", "20", "--log-every", "5"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    ev = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    done = [e for e in ev if e.get("event") == "done"][-1]
    start = [e for e in ev if e.get("event") == "start"][-1]
    print("bert unpadded done:", done)
    assert start["data"]["unpad"] is True and start["data"]["stream_rows"] % 128 == 0
    assert done["gemm_fallbacks"] == {} and np.isfinite(done["loss"])
    steps = [e for e in ev if e.get("event") == "step"]
    assert steps and all(0 < e["real_tokens_per_sec"] < e["tokens_per_sec"] for e in steps)
