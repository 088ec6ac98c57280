"""Document-boundary attention masks on the GPU: the DOC forms of the flash kernels against the fp32 reference, no leak
across a boundary bit for bit, the packed path with positions that restart per document, the ``causal_doc_batch``
kernel against its torch definition, and a ``llama_tiny`` step on such a batch against the fp32 CPU model."""
import math

import numpy as np
import pytest
import torch

from k8s_amd.ops import data as kdata
from k8s_amd.ops import reference as ref
from k8s_amd.ops.attention import _Flash, attention, attention_qkv, attention_reference, doc_bounds

pytestmark = pytest.mark.gpu


def _close(a, b, tol, what):  # tests/test_attention_gpu.py's measure and tolerances
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    assert err <= tol * max(1.0, scale), "%s: max err %g (scale %g)" % (what, err, scale)


def _lo_rows(S, rows):
    """int64 [B, S]: every token's document start, from each row's list of document starts."""
    out = torch.empty(len(rows), S, dtype=torch.int64)
    for b, starts in enumerate(rows):
        assert starts[0] == 0 and list(starts) == sorted(set(starts)) and starts[-1] < S
        s = torch.tensor(list(starts))
        out[b] = s[torch.searchsorted(s, torch.arange(S), right=True) - 1]
    return out


CASES = [
    # B, S, Hq, Hkv, D, document starts per row
    (2, 192, 4, 2, 64, [[0, 1, 2, 63, 64, 65, 130], [0]]),
    (2, 96, 2, 2, 64, [[0, 17, 50], [0, 95]]),
    (1, 320, 4, 1, 128, [[0, 100, 101, 256]]),
    (1, 1152, 2, 2, 64, [[0, 127, 128, 129, 640, 1151]]),
]


def _operands(cuda, B, S, Hq, Hkv, D, seed=0):
    """q, k, v as column slices of one packed tensor (the models' layout), and dO."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, generator=g).to(cuda).bfloat16()
    do = torch.randn(B, S, Hq, D, generator=g).to(cuda).bfloat16()
    return qkv, do


def _views(qkv, Hq, Hkv, D):
    B, S = qkv.shape[:2]
    return (qkv[..., :Hq * D].view(B, S, Hq, D), qkv[..., Hq * D:(Hq + Hkv) * D].view(B, S, Hkv, D),
            qkv[..., (Hq + Hkv) * D:].view(B, S, Hkv, D))


def _flash(qkv, do, Hq, Hkv, D, doc):
    """(O, lse, dQ, dK, dV) of the flash path."""
    from k8s_amd.ops._ext import load

    q, k, v = _views(qkv, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    o, lse = load().flash_fwd(q, k, v, True, None, scale, doc_lo=doc[0], doc_hi=doc[1])
    dq, dk, dv = load().flash_bwd(do, q, k, v, o, lse, True, None, scale, doc_lo=doc[0], doc_hi=doc[1])
    return o, lse[..., :qkv.shape[1]], dq, dk, dv


@pytest.mark.parametrize("B,S,Hq,Hkv,D,rows", CASES)
def test_flash_doc_fwd_bwd(cuda, B, S, Hq, Hkv, D, rows):
    qkv, do = _operands(cuda, B, S, Hq, Hkv, D)
    lo, hi = doc_bounds(_lo_rows(S, rows))
    doc = (lo.to(cuda), hi.to(cuda))
    q, k, v = _views(qkv, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    want = attention_reference(qr, kr, vr, True, None, scale, doc_lo=doc[0])
    want.backward(do.float())
    qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = attention(qq, kk, vv, causal=True, doc=doc)
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith(_Flash.__name__)
    _close(out, want, 2e-2, "O")
    out.backward(do)
    _close(qq.grad, qr.grad, 3e-2, "dQ")
    _close(kk.grad, kr.grad, 3e-2, "dK")
    _close(vv.grad, vr.grad, 3e-2, "dV")
    # the mask is in force: the plain causal call differs from the masked reference wherever a row holds two documents
    plain = _Flash.apply(q, k, v, True, None, scale)
    if any(len(r) > 1 for r in rows):
        assert (plain.float() - want.float()).abs().max().item() > 0.1


@pytest.mark.parametrize("case,doc_index", [(0, 5), (0, 1), (3, 4), (3, 3)])
def test_flash_doc_no_leak(cuda, case, doc_index):
    """Replacing q, k, v and dO of every token outside one document leaves that document's O, lse, dQ, dK and dV
    unchanged bit for bit: masked scores are overwritten before the max, and p = 0 times a finite value adds nothing."""
    B, S, Hq, Hkv, D, rows = CASES[case]
    starts = rows[0]
    a, b = starts[doc_index], (starts[doc_index + 1] if doc_index + 1 < len(starts) else S)
    lo, hi = doc_bounds(_lo_rows(S, rows))
    doc = (lo.to(cuda), hi.to(cuda))
    qkv, do = _operands(cuda, B, S, Hq, Hkv, D, seed=1)
    first = _flash(qkv, do, Hq, Hkv, D, doc)
    qkv2, do2 = _operands(cuda, B, S, Hq, Hkv, D, seed=2)
    qkv2, do2 = qkv2 * 8, do2 * 8  # other finite values (no inf: 0 * inf is NaN)
    qkv2[0, a:b], do2[0, a:b] = qkv[0, a:b], do[0, a:b]
    second = _flash(qkv2, do2, Hq, Hkv, D, doc)
    for name, x, y in zip(("O", "lse", "dQ", "dK", "dV"), first, second):
        sel = (lambda t: t[0, :, a:b]) if name == "lse" else (lambda t: t[0, a:b])
        assert torch.isfinite(sel(x).float()).all(), name
        assert torch.equal(sel(x), sel(y)), name


def test_attention_qkv_doc_packed_matches_split(cuda):
    """attention_qkv with a document mask and positions that restart at every document against the fp32 split + rope +
    reference composition, forward and the packed gradient."""
    from k8s_amd.ops import nn as K

    torch.manual_seed(7)
    B, S, H, Hkv, D = 2, 320, 8, 2, 128
    W = (H + 2 * Hkv) * D
    lo, hi = doc_bounds(_lo_rows(S, [[0, 100, 101, 256], [0, 64, 300]]))
    lo, hi = lo.to(cuda), hi.to(cuda)
    pos = (torch.arange(S, device=cuda, dtype=torch.int32)[None] - lo).reshape(-1).contiguous()
    qkv = (torch.randn(B * S, W, device=cuda) * 0.5).bfloat16().requires_grad_(True)
    table = K.rope_table(S, D, device=cuda)
    o = attention_qkv(qkv, B, S, H, Hkv, D, causal=True, rope=(pos, table), doc=(lo, hi))
    go = torch.randn_like(o)
    (g,) = torch.autograd.grad(o, qkv, go)

    xr = qkv.detach().float().requires_grad_(True)
    q, k, v = xr.split([H * D, Hkv * D, Hkv * D], dim=-1)
    q, k = K._rope_ref(q, pos, table), K._rope_ref(k, pos, table)
    want = attention_reference(q.reshape(B, S, H, D), k.reshape(B, S, Hkv, D), v.reshape(B, S, Hkv, D), True,
                               doc_lo=lo)
    (gr,) = torch.autograd.grad(want, xr, go.float())
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()  # noqa: E731
    assert rel(o, want) < 2e-2
    assert rel(g, gr) < 3e-2


def test_doc_mask_outside_flash_contract_keeps_the_mask(cuda):
    """GPU operands the flash kernels do not take (fp32) run the reference with the mask, not without it."""
    torch.manual_seed(3)
    B, S, H, D = 1, 48, 2, 32
    q, k, v = (torch.randn(B, S, H, D, device=cuda) for _ in range(3))
    lo, hi = doc_bounds(_lo_rows(S, [[0, 20]]))
    out = attention(q, k, v, causal=True, doc=(lo.to(cuda), hi.to(cuda)))
    want = attention_reference(q, k, v, True, doc_lo=lo.to(cuda))
    assert torch.equal(out, want)
    assert (out - attention(q, k, v, causal=True)).abs().max().item() > 1e-3


def test_doc_mask_rejected_combinations(cuda):
    from k8s_amd.ops._ext import load

    B, S, H, D = 1, 128, 2, 64
    q, k, v = (torch.randn(B, S, H, D, device=cuda).bfloat16() for _ in range(3))
    lo, hi = (t.to(cuda) for t in doc_bounds(_lo_rows(S, [[0, 50]])))
    lens = torch.tensor([100], device=cuda, dtype=torch.int32)
    with pytest.raises(ValueError):
        attention(q, k, v, causal=False, doc=(lo, hi))
    with pytest.raises(ValueError):
        attention(q, k, v, causal=True, kv_lens=lens, doc=(lo, hi))
    with pytest.raises(ValueError):
        attention(q, k, v, causal=True, doc=(lo.long(), hi.long()))
    C = load()
    with pytest.raises(RuntimeError):
        C.flash_fwd(q, k, v, True, None, 0.125, doc_lo=lo)  # one table alone
    with pytest.raises(RuntimeError):
        C.flash_fwd(q, k, v, False, None, 0.125, doc_lo=lo, doc_hi=hi)
    with pytest.raises(RuntimeError):
        C.flash_fwd(q, k, v, True, lens, 0.125, doc_lo=lo, doc_hi=hi)
    with pytest.raises(RuntimeError):
        C.flash_fwd(q, k, v, True, None, 0.125, doc_lo=lo[:, :64].contiguous(), doc_hi=hi[:, :64].contiguous())
    o, lse = C.flash_fwd(q, k, v, True, None, 0.125, doc_lo=lo, doc_hi=hi)
    x = torch.empty(B * S, 3 * H * D, device=cuda, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):  # no bias gradient with a document mask
        C.flash_bwd(torch.randn_like(o), q, k, v, o, lse, True, None, 0.125, x, torch.zeros(3 * H * D, device=cuda),
                    doc_lo=lo, doc_hi=hi)


# ------------------------------------------------------------------------------------------------ batch kernel
def _doc_tok(lengths):
    return torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64)


@pytest.mark.parametrize("S,dtype", [(64, torch.int16), (64, torch.int32), (512, torch.int16), (512, torch.int32)])
def test_causal_doc_batch_matches_reference(cuda, S, dtype):
    rng = np.random.default_rng(S)
    lengths = np.concatenate([rng.integers(9, 64, size=150), [3 * S], rng.integers(1, 5, size=40), [2 * S]])
    doc_tok = _doc_tok(lengths)
    T = int(doc_tok[-1])
    vals = rng.integers(0, 60000 if dtype == torch.int16 else 2 ** 31 - 1, size=T)
    src = torch.from_numpy(vals.astype(np.uint16).view(np.int16) if dtype == torch.int16 else vals.astype(np.int32))
    long_doc = int(doc_tok[151 - 1])  # the 3 S document's first token
    starts = torch.tensor([0, int(doc_tok[7]), long_doc + 5, T - S - 1, int(doc_tok[100]) - 1, 1234, long_doc - 3],
                          dtype=torch.int64)  # N = 7: on a document start, inside one long document, the split's end
    want = ref.causal_doc_batch(src, starts, starts, doc_tok, S)
    dt = kdata.doc_offsets(doc_tok, cuda)
    before = kdata.token_launches()
    got = kdata.causal_doc_batch(src.to(cuda), starts, starts, dt, S, T)
    assert kdata.token_launches() == before + 1
    for name, g, w in zip(("ids", "labels", "lo", "hi", "pos"), got, want):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w), name
    assert bool((got[2][2] == 0).all()) and bool((got[3][2] == S).all())  # the window inside one document
    assert int(got[2][1].min()) == 0 and int(got[4][1][0]) == 0  # the window on a document start
    # a compact source (the streamed path): rebased starts, the same absolute positions
    w = S + 1
    at = starts[:, None] + torch.arange(w)
    compact = src[at.reshape(-1)].to(cuda)
    local = torch.arange(len(starts), dtype=torch.int64) * w
    again = kdata.causal_doc_batch(compact, local, starts, dt, S, T)
    for g, w_ in zip(again, want):
        assert torch.equal(g.cpu(), w_)


def test_causal_doc_batch_rejects_bad_inputs(cuda):
    S = 16
    doc_tok = _doc_tok([10, 20, 30])
    src = torch.arange(60, dtype=torch.int32, device=cuda)
    dt = kdata.doc_offsets(doc_tok, cuda)
    ok = torch.tensor([0, 5], dtype=torch.int64)
    before = kdata.token_launches()
    with pytest.raises(ValueError):
        kdata.doc_offsets(torch.tensor([0, 10, 10, 60]), cuda)
    with pytest.raises(ValueError):
        kdata.doc_offsets(torch.tensor([1, 10, 60]), cuda)
    for bad in (dict(starts=torch.tensor([0, 44], dtype=torch.int64)), dict(abs_starts=torch.tensor([0, -1])),
                dict(abs_starts=torch.tensor([0, 44], dtype=torch.int64)), dict(abs_starts=ok[:1]),
                dict(starts=ok.to(cuda)), dict(doc_tok=doc_tok), dict(doc_tok=dt.int()), dict(S=0)):
        kw = dict(dict(starts=ok, abs_starts=ok, doc_tok=dt, S=S), **bad)
        with pytest.raises(RuntimeError):
            kdata.causal_doc_batch(src, kw["starts"], kw["abs_starts"], kw["doc_tok"], kw["S"], 60)
    assert kdata.token_launches() == before


def test_loader_resident_streamed_and_cpu_give_the_same_bits(cuda, tmp_path):
    from k8s_amd.data import open_token_dataset
    from k8s_amd.data.token_loader import TokenLoader
    from k8s_amd.tools import make_dataset

    path = str(tmp_path / "toy")
    make_dataset.make_toy_tokens(path, train_docs=128, val_docs=16)
    ds = open_token_dataset(path, need=("train", "val"))
    for split, train in (("train", True), ("val", False)):
        kw = dict(kind="llama", doc_mask=True, seed=3, train=train)
        cpu = TokenLoader(ds, split, "cpu", 6, 64, **kw)
        resident = TokenLoader(ds, split, cuda, 6, 64, resident_gb=4.0, **kw)
        streamed = TokenLoader(ds, split, cuda, 6, 64, resident_gb=0.0, **kw)
        try:
            assert resident.resident and not streamed.resident
            for t in (0, 1, 2) if train else (0, 1):  # val: 16 documents hold fewer than 12 windows, rows past the end
                want = cpu.batch(t)
                assert len(want) == 5
                for other in (resident.batch(t), streamed.batch(t)):
                    for name, g, w in zip(("ids", "labels", "lo", "hi", "pos"), other, want):
                        assert g.dtype == w.dtype and torch.equal(g.cpu(), w), (split, t, name)
        finally:
            for ld in (cpu, resident, streamed):
                ld.close()


# ------------------------------------------------------------------------------------------------ model
def test_llama_tiny_doc_mask_step_matches_cpu_fp32(cuda):
    from k8s_amd.ops import gemm

    gemm.FALLBACKS.clear()
    g = build_llama(cuda)
    c = build_llama("cpu")
    B, S = 4, 64
    gen = torch.Generator().manual_seed(11)
    ids = torch.randint(0, 512, (B, S + 1), generator=gen)
    lo, hi = doc_bounds(_lo_rows(S, [[0, 9, 40], [0], [0, 1, 2, 63], [0, 33]]))
    pos = torch.arange(S, dtype=torch.int32)[None] - lo
    labels = torch.where(torch.arange(S)[None] + 1 < hi, ids[:, 1:], torch.full((B, S), -100))
    batch = (ids[:, :-1].contiguous(), labels, lo, hi, pos)
    lc = c.loss(batch).item()
    g.store.begin_step()
    loss = g.loss(tuple(t.to(cuda) for t in batch))
    loss.backward()
    lg = loss.float().item()
    assert abs(lg - lc) < 3e-2 * max(1.0, abs(lc)), (lg, lc)  # tests/test_models_gpu.py's tolerance for Llama
    unmasked = c.loss(batch[:2]).item()
    assert abs(unmasked - lc) > 1e-3  # the mask and the positions are in force
    assert gemm.FALLBACKS == {}, gemm.FALLBACKS


def build_llama(device):
    from k8s_amd.models.registry import build

    return build("llama_tiny", device, batch=4, seed=3)
