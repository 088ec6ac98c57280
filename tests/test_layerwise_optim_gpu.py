"""LARS / LAMB HIP kernels (csrc/kernels/layerwise.hip) through FusedLARS / FusedLAMB against the fp64 textbook.

One store for every case, with I the work-item size: slots of 1, 64, 129, I, I + 64, 5 I + 192 and (7, 5, 3)
elements (a single padded chunk, exact chunks, a ragged end, exactly one item, one item and a 64-element one, a
multi-item slot with a short last item), alternating ``decay``, mixed ``lowp``, and a padded tail.

Tolerances are the project's own (``_close`` of tests/test_kernels_gpu.py): parameters 1e-5, moments 1e-6, bf16
copy 1e-2, sums and ratios 1e-4. An fp32 textbook step on the CPU differs from the fp64 one by 5.4e-8 in the
parameters under that rule and by 1.7e-7 relative in the ratio, for tensors of 1 to 300,000 elements."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from layerwise_textbook import Textbook  # noqa: E402

pytestmark = pytest.mark.gpu

I = 16384
SHAPES = [(1,), (64,), (129,), (I,), (I + 64,), (5 * I + 192,), (7, 5, 3)]
LR = {"lars": 0.05, "lamb": 0.01}
WD = {"lars": 1e-3, "lamb": 0.01}
ETA = 1.0  # LARS trust coefficient: ratios of order 1, so the 1e-4 bound means something


def _close(a, b, tol):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    print("max err %.3g (scale %.3g, tol %g)" % (err, scale, tol))
    assert err <= tol * max(1.0, scale), "max err %g (scale %g)" % (err, scale)


def _tail(params):
    """First element beyond the last slot (a slot is its 64-aligned extent)."""
    return params[-1].offset + (params[-1].numel + 63) // 64 * 64


def _store(dev, gdt=torch.float32):
    from k8s_amd.parallel.flat import ParamStore, init_normal

    store = ParamStore()
    # decay on the odd slots (64, I and the multi-item one), no bf16 copy for slots 1 and 4: every combination
    params = [store.new("p%d" % i, s, init_normal(0.5), decay=(i % 2 == 1), lowp=(i % 3 != 1))
              for i, s in enumerate(SHAPES)]
    store.finalize(dev, grad_dtype=gdt, pad_to=4 * 64, seed=5)
    assert store.total >= _tail(params) + 64  # there is a tail beyond the last slot
    return store, params


def _opt(kind, store, clip):
    from k8s_amd.ops.optim import ITEM, FusedLAMB, FusedLARS

    assert ITEM == I
    if kind == "lars":
        return FusedLARS(store, lr=LR[kind], momentum=0.9, weight_decay=WD[kind], trust_coef=ETA, max_grad_norm=clip)
    return FusedLAMB(store, lr=LR[kind], weight_decay=WD[kind], max_grad_norm=clip)


def _book(kind, params, clip):
    return Textbook(kind, [p.master.cpu() for p in params], [p.decay for p in params], LR[kind], WD[kind], clip,
                    eta=ETA)


_GRADS = {}


def _grads(step, gdt):
    """Host gradients of one step, computed once (bf16: already rounded, so the textbook sees what the kernel sees)."""
    key = (step, gdt)
    if key not in _GRADS:
        g = torch.Generator().manual_seed(100 + step)
        _GRADS[key] = [(torch.randn(s, generator=g) * 0.3).to(gdt) for s in SHAPES]
    return _GRADS[key]


def _deposit(store, params, gs):
    for p, g in zip(params, gs):
        p.grad.copy_(g)


def _flat(store, params, tensors):
    out = torch.zeros(store.total, dtype=torch.float64)
    for p, t in zip(params, tensors):
        out[p.offset:p.offset + p.numel] = t.reshape(-1)
    return out


def _book_sums(book):
    return torch.tensor([[float((p * p).sum()), float((x * x).sum())] for p, x in zip(book.last_p, book.last_x)],
                        dtype=torch.float64)


def _check_against_book(kind, store, params, opt, book, owned=None):
    """Owned slices (default: everything) of every buffer against the textbook, sums and ratios for every slot."""
    ranges = owned or [(0, store.total)]
    P, M, V = (_flat(store, params, t) for t in (book.p, book.m, book.v))
    st = opt.state_tensors()
    off = 0
    lowp = torch.zeros(store.total, dtype=torch.bool)
    for p in params:
        lowp[p.offset:p.offset + p.numel] = p.lowp
    for lo, hi in ranges:
        so = off if owned else lo
        _close(store.master[lo:hi], P[lo:hi], 1e-5)
        _close(st[0][so:so + hi - lo], M[lo:hi], 1e-6)
        if kind == "lamb":
            _close(st[1][so:so + hi - lo], V[lo:hi], 1e-6)
        sel = lowp[lo:hi]
        _close(store.half[lo:hi].cpu()[sel], P[lo:hi][sel], 1e-2)
        assert torch.equal(store.half[lo:hi].cpu()[sel], store.master[lo:hi].cpu()[sel].to(torch.bfloat16))
        off += hi - lo
    want = _book_sums(book)
    _close(opt.last_sums, want, 1e-4)
    _close(opt.last_trust_ratio, torch.tensor(book.ratio), 1e-4)
    # each slot on its own scale too: blocked fp32 sums of at most 5 I + 192 terms are good to ~1e-6 relative
    torch.testing.assert_close(opt.last_sums.double().cpu(), want, rtol=1e-4, atol=1e-30)
    torch.testing.assert_close(opt.last_trust_ratio.double().cpu(), torch.tensor(book.ratio, dtype=torch.float64),
                               rtol=1e-4, atol=0)


@pytest.mark.parametrize("hyper", [False, True])
@pytest.mark.parametrize("clip", [None, 2.0])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_kernels_match_textbook_fp64(cuda, kind, gdt, clip, hyper):
    store, params = _store(cuda, gdt)
    opt = _opt(kind, store, clip)  # the scaled gradient norm is ~50: a clip of 2 is active
    book = _book(kind, params, clip)
    if hyper:
        opt.use_device_hyper()
    for step in range(3):
        gs = _grads(step, gdt)
        _deposit(store, params, gs)
        lr = LR[kind] / (step + 1)
        if hyper:  # the device values are the ones used: the host ones are wrong on purpose
            opt.set_hyper(lr, step + 1)
            if kind == "lamb":
                opt.step_count = 40 + step
            opt.step(grad_scale=0.5, lr=123.0)
        else:
            opt.step(grad_scale=0.5, lr=lr)
        book.step(gs, grad_scale=0.5, lr=lr)
        _check_against_book(kind, store, params, opt, book)
    for i, p in enumerate(params):
        if not p.decay:
            assert float(opt.last_trust_ratio[i]) == 1.0


def _run_three(cuda, kind):
    store, params = _store(cuda)
    # no max_grad_norm: the clip factor comes from the existing global-norm kernel, whose float atomics are not
    # reproducible run to run; what is pinned here is the layer-wise kernels' own fixed summation order
    opt = _opt(kind, store, None)
    tail = _tail(params)
    store.master[tail:] = 3.0
    store.half[tail:] = 5.0
    for t in opt.state_tensors():
        t[tail:] = 7.0
    for p in params:
        if not p.lowp:
            store.half[p.offset:p.offset + (p.numel + 63) // 64 * 64] = -9.0
    for step in range(3):
        _deposit(store, params, _grads(step, torch.float32))
        opt.step(grad_scale=0.5)
    torch.cuda.synchronize()
    return store, params, opt, tail


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_bitwise_reproducible_and_writes_only_its_slots(cuda, kind):
    a_store, params, a_opt, tail = _run_three(cuda, kind)
    b_store, _, b_opt, _ = _run_three(cuda, kind)
    bufs = lambda s, o: [s.master, s.half, o.last_sums, o.last_trust_ratio] + o.state_tensors()  # noqa: E731
    for x, y in zip(bufs(a_store, a_opt), bufs(b_store, b_opt)):
        assert torch.equal(x, y)
    assert bool((a_store.master[tail:] == 3.0).all()) and bool((a_store.half[tail:] == 5.0).all())
    for t in a_opt.state_tensors():
        assert bool((t[tail:] == 7.0).all())
    for p in params:
        if not p.lowp:
            assert bool((a_store.half[p.offset:p.offset + (p.numel + 63) // 64 * 64] == -9.0).all())
        else:
            assert torch.equal(p.half, p.master.to(torch.bfloat16))


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_zero_clip_factor_leaves_every_buffer_bit_identical(cuda, kind):
    """A NaN gradient at the third step: the clip factor is 0 and all four launches return before their first
    write, so everything equals a run that stopped after two steps."""
    store, params = _store(cuda)
    opt = _opt(kind, store, 2.0)
    for step in range(2):
        _deposit(store, params, _grads(step, torch.float32))
        opt.step(grad_scale=0.5)
    keep = [t.clone() for t in [store.master, store.half, opt.last_sums, opt.last_trust_ratio] + opt.state_tensors()]
    _deposit(store, params, _grads(2, torch.float32))
    params[5].grad[I + 7] = float("nan")
    opt.step(grad_scale=0.5)
    torch.cuda.synchronize()
    now = [store.master, store.half, opt.last_sums, opt.last_trust_ratio] + opt.state_tensors()
    for x, y in zip(keep, now):
        assert torch.equal(x, y)
    assert bool(torch.isfinite(store.master).all())


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_sharded_layout_matches_whole_model_step(cuda, kind):
    """ZeRO-1 layout in one process: this "rank" owns three ranges that start and end inside slots (the multi-item
    slot 5 is cut twice, at offsets that are no multiple of I) and cover half of the store, its state is packed, and
    ``stats_reduce`` adds what the other rank would have contributed, computed here in fp64. The only GPU case with
    state offset != flat offset."""
    store, params = _store(cuda)
    total = store.total
    owned = [(64, 8192), (24576, 57472), (98304, total)]
    assert params[3].offset < 8192 < params[4].offset < 24576 < params[5].offset < 57472 < 98304
    assert abs(sum(hi - lo for lo, hi in owned) - total // 2) < total // 50
    mine = torch.zeros(total, dtype=torch.bool)
    for lo, hi in owned:
        mine[lo:hi] = True
    clip = 2.0
    opt = _opt(kind, store, clip)
    opt.shard(owned)
    assert opt.state_numel() == len(opt.STATE) * int(mine.sum())
    book = _book(kind, params, clip)
    before = store.master.clone()
    other = {}

    def reduce(t):
        t.add_(other["clip" if t.numel() == 2 else "sums"].to(t.device, t.dtype).reshape(t.shape))

    for step in range(3):
        gs = _grads(step, torch.float32)
        _deposit(store, params, gs)
        lr = LR[kind] / (step + 1)
        book.step(gs, grad_scale=0.5, lr=lr)
        G = _flat(store, params, [g.double() for g in gs])
        other["clip"] = torch.stack([(G[~mine] ** 2).sum(), torch.zeros((), dtype=torch.float64)])
        sums = torch.zeros(len(params), 2, dtype=torch.float64)
        for i, p in enumerate(params):
            sel = ~mine[p.offset:p.offset + p.numel]
            sums[i, 0] = (book.last_p[i].reshape(-1)[sel] ** 2).sum()
            sums[i, 1] = (book.last_x[i].reshape(-1)[sel] ** 2).sum()
        other["sums"] = sums
        opt.step(grad_scale=0.5, lr=lr, ranges=owned, stats_reduce=reduce)
        _check_against_book(kind, store, params, opt, book, owned=owned)
    assert torch.equal(store.master.cpu()[~mine], before.cpu()[~mine])  # the other rank's slices are not ours to write


@pytest.mark.parametrize("name,kind", [("resnet_tiny", "lars"), ("bert_tiny", "lamb")])
def test_step_graph_matches_eager(cuda, name, kind):
    from k8s_amd.models.registry import build
    from k8s_amd.ops.optim import FusedLAMB, FusedLARS
    from k8s_amd.parallel.ddp import GradReducer
    from k8s_amd.utils.graph import StepGraph

    def make():
        torch.manual_seed(0)
        w = build(name, cuda, 4, seed=3)
        o = (FusedLARS(w.store, lr=0.02, momentum=0.9, weight_decay=1e-4, trust_coef=0.02) if kind == "lars"
             else FusedLAMB(w.store, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0))
        red = GradReducer(w.store)

        def body(inputs, lr):
            red.begin_step()
            loss = w.loss(inputs)
            loss.backward()
            red.finish()
            o.step(grad_scale=red.grad_scale, lr=lr)
            return loss

        return w, o, body

    base = 0.02 if kind == "lars" else 1e-3
    lrs = [base * (i + 1) for i in range(6)]  # a changing schedule: must reach the replayed kernels
    w1, o1, body1 = make()
    eager = [float(body1(w1.batch(i), lr)) for i, lr in enumerate(lrs)]
    w2, o2, body2 = make()
    g = StepGraph(body2, o2, warmup=2)
    graphed = [float(g(w2.batch(i), lr)) for i, lr in enumerate(lrs)]
    torch.cuda.synchronize()
    assert g.replays == 3 and o1.step_count == o2.step_count
    for a, b in zip(eager, graphed):
        assert abs(a - b) <= 2e-2 * max(1.0, abs(a)), (eager, graphed)
    # noise floor as in tests/test_graph_gpu.py: the models' reductions use float atomics, so two eager runs differ
    # too; the floor is the largest of three eager pairs
    runs = []
    for _ in range(2):
        w3, o3, body3 = make()
        for i, lr in enumerate(lrs):
            body3(w3.batch(i), lr)
        runs.append(w3)
    torch.cuda.synchronize()

    def rel(x, y):
        return ((x.store.master - y.store.master).norm() / x.store.master.norm()).item()

    floor = max(rel(w1, runs[0]), rel(w1, runs[1]), rel(runs[0], runs[1]))
    assert rel(w1, w2) <= max(5 * floor, 2e-3), (rel(w1, w2), floor)
