"""Gradient accumulation on the GPU: the two streaming kernels (``csrc/kernels/accum.hip``) bit for bit against
``torch`` on the same device (each output element is ONE fp32 add, or one add and one round-to-nearest-even), their
argument checks, 64-bit indexing, and the plumbing through ``GradAccumulator``, the two gradient transports and the
flat optimizers. No test re-runs a backward, so the atomics of the embedding backward never enter a comparison."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOTALS = [64, 192, 64 * 1031, 2 ** 20 + 64]
SENT = -12345.0  # sentinels of elements no kernel may touch (fp32 buffers / bf16 buffers)
SENT_BF = -1024.0
_inputs = {}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _same(a, b):
    """Bitwise equality that also holds for NaN (one add on the same hardware: the payloads agree too)."""
    return torch.equal(_bits(a), _bits(b))


def _ranges(total):
    out = [(0, total), (64, total), (64, total - 64), (0, 0), (total, total), (64, 64)]
    return [(lo, hi) for lo, hi in dict.fromkeys(out) if 0 <= lo <= hi <= total]


def _pair(dev, total):
    """(g, acc) for one buffer size, made once and never written (every test clones)."""
    if total not in _inputs:
        gen = torch.Generator(device=dev).manual_seed(total)
        g = torch.randn(total, device=dev, generator=gen)
        acc = torch.randn(total, device=dev, generator=gen) * 3.0
        _inputs[total] = (g, acc)
    return _inputs[total]


@pytest.mark.parametrize("total", TOTALS)
@pytest.mark.parametrize("first", [True, False])
def test_grad_accumulate_bitwise(cuda, total, first):
    from k8s_amd.ops._ext import load

    C = load()
    g, acc0 = _pair(cuda, total)
    for lo, hi in _ranges(total):
        # first: the result must not depend on what the buffer held (NaN); else a sentinel marks untouched elements
        acc = torch.full_like(acc0, float("nan")) if first else acc0.clone()
        before = acc.clone()
        gk = g.clone()
        C.grad_accumulate(acc, gk, lo, hi, first)
        want = g[lo:hi] if first else acc0[lo:hi] + g[lo:hi]
        assert _same(acc[lo:hi], want), (total, lo, hi)
        assert _same(acc[:lo], before[:lo]) and _same(acc[hi:], before[hi:]), (total, lo, hi)
        assert _same(gk, g)  # the gradient is only read


@pytest.mark.parametrize("total", TOTALS)
@pytest.mark.parametrize("with_bf", [False, True])
def test_grad_fold_bitwise(cuda, total, with_bf):
    from k8s_amd.ops._ext import load

    C = load()
    g0, acc = _pair(cuda, total)
    for lo, hi in _ranges(total):
        g = g0.clone()
        a = acc.clone()
        out_bf = torch.full((hi - lo + 64,), SENT_BF, device=cuda, dtype=torch.bfloat16) if with_bf else None
        C.grad_fold(g, a, lo, hi, out_bf)
        want = g0[lo:hi] + acc[lo:hi]
        assert _same(g[lo:hi], want), (total, lo, hi)
        assert _same(g[:lo], g0[:lo]) and _same(g[hi:], g0[hi:]), (total, lo, hi)
        assert _same(a, acc)  # the running sum is only read
        if with_bf:
            assert _same(out_bf[:hi - lo], want.bfloat16()), (total, lo, hi)
            assert bool((out_bf[hi - lo:] == SENT_BF).all()), "padding of a longer out_bf was written"


def test_result_does_not_depend_on_the_grid(cuda):
    """A 3-CU planner budget (24 blocks) makes every thread take several unrolled grid-stride trips and a tail on
    the largest buffer; the bits are those of the full grid."""
    from k8s_amd.ops._ext import load

    C = load()
    total = TOTALS[-1]
    g0, acc0 = _pair(cuda, total)
    lo, hi = 64, total - 64
    C.set_planner_cus(3)
    try:
        acc = acc0.clone()
        C.grad_accumulate(acc, g0, lo, hi, False)
        g = g0.clone()
        out_bf = torch.empty(hi - lo, device=cuda, dtype=torch.bfloat16)
        C.grad_fold(g, acc0, lo, hi, out_bf)
        g2 = g0.clone()
        C.grad_fold(g2, acc0, lo, hi, None)
        torch.cuda.synchronize()
    finally:
        C.set_planner_cus(0)
    assert _same(acc[lo:hi], acc0[lo:hi] + g0[lo:hi]) and _same(acc[:lo], acc0[:lo]) and _same(acc[hi:], acc0[hi:])
    for t in (g, g2):
        assert _same(t[lo:hi], g0[lo:hi] + acc0[lo:hi]) and _same(t[:lo], g0[:lo]) and _same(t[hi:], g0[hi:])
    assert _same(out_bf, (g0[lo:hi] + acc0[lo:hi]).bfloat16())


def test_non_finite_values_propagate(cuda):
    from k8s_amd.ops._ext import load

    C = load()
    total = 192
    g0, acc0 = _pair(cuda, total)
    g0 = g0.clone()
    g0[3], g0[70], g0[130], g0[191] = float("inf"), float("nan"), float("-inf"), float("inf")
    acc0 = acc0.clone()
    acc0[191] = float("-inf")  # inf + -inf = NaN
    for first in (True, False):
        acc = acc0.clone()
        C.grad_accumulate(acc, g0, 0, total, first)
        want = g0 if first else acc0 + g0
        assert _same(acc, want)
        assert bool(torch.isnan(acc[70])) and bool(torch.isinf(acc[3])) and bool(torch.isinf(acc[130]))
    g = g0.clone()
    out_bf = torch.zeros(total, device=cuda, dtype=torch.bfloat16)
    C.grad_fold(g, acc0, 0, total, out_bf)
    want = g0 + acc0
    assert _same(g, want) and bool(torch.isnan(g[191]))
    assert torch.equal(torch.isnan(out_bf), torch.isnan(want)) and torch.equal(torch.isinf(out_bf), torch.isinf(want))
    fin = torch.isfinite(want)
    assert torch.equal(out_bf[fin], want.bfloat16()[fin])


def test_indices_beyond_2_31(cuda):
    """total = 2^31 + 192 (two fp32 buffers, ~17 GB) and the range [64, total - 64): a 32-bit element or byte index
    would wrap. Only three windows of up to 4,096 elements (start, around element 2^31, end -- the last two overlap,
    the buffer ends 192 elements past 2^31) and the two untouched 64-element edges are compared."""
    from k8s_amd.ops._ext import load

    C = load()
    total = 2 ** 31 + 192
    lo, hi = 64, total - 64
    W = 4096
    wins = [(lo, lo + W), (2 ** 31 - W // 2, hi), (hi - W, hi)]
    gen = torch.Generator(device=cuda).manual_seed(31)
    g = torch.zeros(total, device=cuda)
    acc = torch.zeros(total, device=cuda)
    head, tail = slice(0, 2 * W), slice(total - 2 * W, total)  # the random regions that hold the windows
    for t in (g, acc):
        for region in (head, tail):
            t[region] = torch.randn(2 * W, device=cuda, generator=gen)
        t[:64] = SENT
        t[-64:] = SENT
    g0 = {r: g[slice(*r)].clone() for r in wins}
    a0 = {r: acc[slice(*r)].clone() for r in wins}
    edge = torch.full((64,), SENT, device=cuda)
    C.grad_accumulate(acc, g, lo, hi, False)  # acc = a + g
    for r in wins:
        assert _same(acc[slice(*r)], a0[r] + g0[r]), r
    assert _same(acc[:64], edge) and _same(acc[-64:], edge)
    out_bf = torch.empty(hi - lo, device=cuda, dtype=torch.bfloat16)
    C.grad_fold(g, acc, lo, hi, out_bf)  # g = g + (a + g)
    for r in wins:
        want = g0[r] + (a0[r] + g0[r])
        assert _same(g[slice(*r)], want), r
        assert _same(out_bf[r[0] - lo:r[1] - lo], want.bfloat16()), r
    assert _same(g[:64], edge) and _same(g[-64:], edge)
    C.grad_accumulate(acc, g, lo, hi, True)  # the copy form
    for r in wins:
        assert _same(acc[slice(*r)], g0[r] + (a0[r] + g0[r])), r
    assert _same(acc[:64], edge) and _same(acc[-64:], edge)
    del g, acc, out_bf
    torch.cuda.empty_cache()


def test_argument_checks(cuda):
    from k8s_amd.ops._ext import load

    C = load()
    g = torch.zeros(256, device=cuda)
    acc = torch.zeros(256, device=cuda)
    bad = [
        lambda: C.grad_accumulate(acc, g, 32, 256, False),                 # misaligned lo
        lambda: C.grad_accumulate(acc, g, 0, 200, False),                  # misaligned hi
        lambda: C.grad_accumulate(acc, g, 0, 320, False),                  # hi > numel
        lambda: C.grad_accumulate(acc, g, 128, 64, False),                 # lo > hi
        lambda: C.grad_accumulate(acc, g, -64, 64, False),                 # lo < 0
        lambda: C.grad_accumulate(acc, g.bfloat16(), 0, 256, False),       # bf16 g
        lambda: C.grad_accumulate(acc, g.cpu(), 0, 256, False),            # CPU mixed with GPU
        lambda: C.grad_accumulate(acc.cpu(), g, 0, 256, False),
        lambda: C.grad_accumulate(acc, g[:192], 0, 192, False),            # sizes differ
        lambda: C.grad_accumulate(acc, acc, 0, 256, False),                # one buffer twice
        lambda: C.grad_accumulate(acc[1:193], g[1:193], 0, 192, False),    # not 16-B aligned
        lambda: C.grad_accumulate(acc[::2], g[::2], 0, 128, False),        # not contiguous
        lambda: C.grad_fold(g, acc, 32, 256, None),
        lambda: C.grad_fold(g, acc, 0, 320, None),
        lambda: C.grad_fold(g.bfloat16(), acc, 0, 256, None),
        lambda: C.grad_fold(g, acc.cpu(), 0, 256, None),
        lambda: C.grad_fold(g, acc, 0, 256, torch.zeros(192, device=cuda, dtype=torch.bfloat16)),  # out_bf too short
        lambda: C.grad_fold(g, acc, 0, 256, torch.zeros(256, device=cuda)),                        # out_bf fp32
        lambda: C.grad_fold(g, acc, 0, 256, torch.zeros(256, dtype=torch.bfloat16)),               # out_bf on the CPU
    ]
    for i, f in enumerate(bad):
        with pytest.raises((RuntimeError, TypeError)):
            f()
            pytest.fail("bad call %d was accepted" % i)
    torch.cuda.synchronize()
    assert not g.any() and not acc.any()


# --------------------------------------------------------------------------------------------------- plumbing
def _micro_batches(w, acc, begin, n, poison=None):
    """n micro-batches through a transport's ``begin``; returns every micro-batch's own gradient (cloned after
    ``zero_unwritten``). ``poison``: micro-batch whose gradient gets a NaN before it is accumulated."""
    grads = []
    for k in range(n):
        last = k == n - 1
        if acc is not None and acc.active:
            begin(sync=last)
        else:
            begin()
        w.loss(w.batch(k)).backward()
        w.store.zero_unwritten()
        if poison == k:
            w.store.grad[w.store.params[3].offset + 1] = float("nan")
        grads.append(w.store.grad.clone())
        if not last:
            acc.accumulate(first=(k == 0))
    return grads


def test_three_micro_batches_through_the_reducer_bitwise(cuda):
    from k8s_amd.models.registry import build
    from k8s_amd.parallel.accum import GradAccumulator
    from k8s_amd.parallel.ddp import GradReducer

    w = build("bert_tiny", cuda, 4, fixed_batch=False)
    acc = GradAccumulator(w.store, 3)
    assert acc.buf is None and acc.scale == 1.0 / 3
    red = GradReducer(w.store, enabled=False, accumulator=acc)
    assert red.grad_scale == 1.0 / 3
    for _ in range(2):  # a second optimizer step reuses the buffer: nothing of the first may survive in it
        g1, g2, g3 = _micro_batches(w, acc, red.begin_step, 3)
        red.finish()
        assert not _same(g1, g2) and not _same(g2, g3)
        assert _same(w.store.grad, g3 + (g1 + g2))
    assert acc.buf.shape == w.store.grad.shape and acc.buf.dtype == torch.float32
    with pytest.raises(RuntimeError):  # a non-final micro-batch cannot be finished
        red.begin_step(sync=False)
        red.finish()


@pytest.mark.parametrize("kind", ["adam", "lamb"])
def test_optimizer_step_after_accumulation_bitwise(cuda, kind):
    """steps = 2: the optimizer stepped with the transport's grad_scale (1/2) on the unscaled sum leaves the bits of
    the same optimizer stepped with grad_scale 1 on (g1 + g2) * 0.5 -- scaling by a power of two is exact."""
    from k8s_amd.models.registry import build
    from k8s_amd.ops.optim import FusedAdam, FusedLAMB
    from k8s_amd.parallel.accum import GradAccumulator
    from k8s_amd.parallel.ddp import GradReducer

    cls = FusedAdam if kind == "adam" else FusedLAMB
    w = build("bert_tiny", cuda, 4, fixed_batch=False)
    s = w.store
    acc = GradAccumulator(s, 2)
    red = GradReducer(s, enabled=False, accumulator=acc)
    g1, g2 = _micro_batches(w, acc, red.begin_step, 2)
    red.finish()
    assert red.grad_scale == 0.5 and _same(s.grad, g2 + g1)
    master0, half0 = s.master.clone(), s.half.clone()
    a = cls(s, lr=1e-2, weight_decay=0.01)
    a.step(grad_scale=red.grad_scale)
    got = [s.master.clone(), s.half.clone()] + [t.clone() for t in a.state_tensors()]
    assert not _same(got[0], master0)
    s.master.copy_(master0)
    s.half.copy_(half0)
    s.grad.copy_((g1 + g2) * 0.5)
    b = cls(s, lr=1e-2, weight_decay=0.01)
    b.step(grad_scale=1.0)
    for x, y in zip(got, [s.master, s.half] + b.state_tensors()):
        assert _same(x, y)


@pytest.mark.parametrize("kind", ["adam", "lamb"])
def test_nan_in_an_early_micro_batch_skips_the_step(cuda, kind):
    """--max-grad-norm path: a NaN in micro-batch 1's gradient reaches the clip statistics through the accumulated
    sum, the clip factor is 0 and the step leaves masters, working copy and state as they were."""
    from k8s_amd.models.registry import build
    from k8s_amd.ops.optim import FusedAdam, FusedLAMB
    from k8s_amd.parallel.accum import GradAccumulator
    from k8s_amd.parallel.ddp import GradReducer

    cls = FusedAdam if kind == "adam" else FusedLAMB
    w = build("bert_tiny", cuda, 4, fixed_batch=False)
    s = w.store
    acc = GradAccumulator(s, 2)
    red = GradReducer(s, enabled=False, accumulator=acc)
    opt = cls(s, lr=1e-2, weight_decay=0.01, max_grad_norm=1.0)
    _micro_batches(w, acc, red.begin_step, 2)
    red.finish()
    opt.step(grad_scale=red.grad_scale)  # a healthy step first: the state is not all zeros
    keep = [t.clone() for t in [s.master, s.half] + opt.state_tensors()]
    _micro_batches(w, acc, red.begin_step, 2, poison=0)
    red.finish()
    assert bool(torch.isnan(s.grad).any())
    opt.step(grad_scale=red.grad_scale)
    torch.cuda.synchronize()
    for x, y in zip(keep, [s.master, s.half] + opt.state_tensors()):
        assert _same(x, y)
    assert bool(torch.isfinite(s.master).all())


def test_resnet_tiny_two_micro_batches(cuda):
    """The conv / BatchNorm deposit paths (``slot_for_write``, ``BnStatLink``): g2 + g1 bitwise, and the running
    statistics advanced once per micro-batch."""
    from k8s_amd.models.registry import build
    from k8s_amd.parallel.accum import GradAccumulator
    from k8s_amd.parallel.ddp import GradReducer

    w = build("resnet_tiny", cuda, 8, fixed_batch=False)
    bns = w.model.batch_norms()
    acc = GradAccumulator(w.store, 2)
    red = GradReducer(w.store, enabled=False, accumulator=acc)
    stats = [[(bn.running_mean.clone(), bn.running_var.clone()) for bn in bns]]
    grads = []
    for k in range(2):
        red.begin_step(sync=(k == 1))
        w.loss(w.batch(k)).backward()
        w.store.zero_unwritten()
        grads.append(w.store.grad.clone())
        stats.append([(bn.running_mean.clone(), bn.running_var.clone()) for bn in bns])
        if k == 0:
            acc.accumulate(first=True)
    red.finish()
    g1, g2 = grads
    assert bool(g1.any()) and not _same(g1, g2)
    assert _same(w.store.grad, g2 + g1)
    for before, mid, after in zip(*stats):  # every BatchNorm moved its running statistics in both micro-batches
        assert not torch.equal(before[1], mid[1]) and not torch.equal(mid[1], after[1])
        assert not torch.equal(before[0], mid[0]) and not torch.equal(mid[0], after[0])


def test_one_step_accumulator_is_inert(cuda):
    """``GradAccumulator(store, 1)`` allocates nothing, launches nothing, and the step is bitwise the one without
    an accumulator (fixed gradients deposited into a synthetic store: no backward is run twice)."""
    from k8s_amd.ops.optim import FusedAdam
    from k8s_amd.parallel.accum import GradAccumulator
    from k8s_amd.parallel.ddp import GradReducer
    from k8s_amd.parallel.flat import ParamStore, init_normal

    shapes = [(300, 129), (1000,), (3, 3, 64, 64), (77,), (64,)]
    gen = torch.Generator(device=cuda).manual_seed(5)
    grads = [torch.randn(sh, device=cuda, generator=gen) for sh in shapes]
    res = []
    for with_acc in (False, True):
        st = ParamStore()
        for i, sh in enumerate(shapes):
            st.new("p%d" % i, sh, init_normal(0.02), lowp=len(sh) > 1)
        st.finalize(cuda)
        acc = GradAccumulator(st, 1) if with_acc else None
        red = GradReducer(st, enabled=False, accumulator=acc)
        opt = FusedAdam(st, lr=1e-2)
        assert red.acc is None and red.grad_scale == 1.0
        torch.cuda.synchronize()
        mem = torch.cuda.memory_allocated(cuda)
        red.begin_step()
        for p in reversed(st.params[1:]):  # p0 is never used: finish() zeroes it
            st.deposit(p, grads[p.index])
        red.finish()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated(cuda) == mem
        g = st.grad.clone()
        opt.step(grad_scale=red.grad_scale)
        if with_acc:
            assert acc.buf is None and not acc.active
            with pytest.raises(RuntimeError):
                acc.accumulate(first=True)
            with pytest.raises(ValueError):
                red.begin_step(sync=False)
        res.append((g, st.master.clone(), st.half.clone()))
    for x, y in zip(res[0], res[1]):
        assert _same(x, y)
    assert bool(res[0][0].any())


def test_accumulator_refuses_a_bf16_gradient_store(cuda):
    from k8s_amd.models.registry import build
    from k8s_amd.parallel.accum import GradAccumulator

    w = build("bert_tiny", cuda, 4, grad_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        GradAccumulator(w.store, 2)
    with pytest.raises(ValueError):
        GradAccumulator(w.store, 0)


# --------------------------------------------------------------------------------------------------- one-rank RCCL group
@pytest.fixture(scope="module")
def one_rank_group(cuda):
    """A one-rank RCCL group in this process (as tests/rccl_worker.py makes one), gone again after this module."""
    from k8s_amd.parallel import dist as kdist

    kdist.init_process_group(backend="nccl", force=True)
    yield
    torch.cuda.synchronize()
    kdist.destroy()


@pytest.mark.parametrize("transport", ["reducer", "service"])
@pytest.mark.parametrize("comm", ["fp32", "bf16"])
def test_fold_before_the_collective_on_a_one_rank_group(cuda, one_rank_group, transport, comm):
    """The enabled transports on a one-rank RCCL group (every reduction is the identity): the fold runs bucket by
    bucket before each collective, in the bf16 transport as the producer of the send buffer. fp32: the exact sum;
    bf16: the sum rounded to bf16 once."""
    from k8s_amd.models.registry import build
    from k8s_amd.ops.optim import FusedSGD
    from k8s_amd.parallel.accum import GradAccumulator
    from k8s_amd.parallel.ddp import GradReducer
    from k8s_amd.parallel.ps import ShardedParameterService

    dtype = torch.bfloat16 if comm == "bf16" else torch.float32
    w = build("bert_tiny", cuda, 4, fixed_batch=False)
    acc = GradAccumulator(w.store, 3)
    launched, last = [], {}

    def spy(inner, t):
        """Records every launch and keeps the bucket's gradient as the launch finds it: the last micro-batch's own
        (its backward is complete for a ready bucket), before the fold -- the buckets are folded and reduced in
        place while the last backward still runs, so a clone after that backward would come too late."""
        def launch(b, fold=False):
            launched.append((t.sync, fold))
            last[(b.lo, b.hi)] = w.store.grad[b.lo:b.hi].clone()
            return inner(b, fold)
        return launch

    if transport == "reducer":
        t = GradReducer(w.store, bucket_mb=0.02, enabled=True, comm_dtype=dtype, accumulator=acc)
        t._launch = spy(t._launch, t)
        end = t.finish
    else:
        opt = FusedSGD(w.store, lr=0.0, momentum=0.0, weight_decay=0.0)
        t = ShardedParameterService(w.store, opt, bucket_mb=0.02, comm_dtype=dtype, enabled=True, accumulator=acc)
        t._push = spy(t._push, t)
        end = t.step
    assert len(t.buckets) > 3 and t.grad_scale == 1.0 / 3
    g1, g2, _ = _micro_batches(w, acc, t.begin_step, 3)
    assert launched and len(launched) <= len(t.buckets)  # buckets of the last backward, launched as they got ready
    end()
    w.store.wait_pending()  # (the service's lazily waited pull)
    torch.cuda.synchronize()
    # every bucket once and folded, each in the final micro-batch (sync): the non-final ones launched no collective
    assert launched == [(True, True)] * len(t.buckets)
    assert sorted(last) == sorted((b.lo, b.hi) for b in t.buckets)
    for (lo, hi), g3 in last.items():
        want = g3 + (g1[lo:hi] + g2[lo:hi])
        assert _same(w.store.grad[lo:hi], want.bfloat16().float() if comm == "bf16" else want), (lo, hi)
