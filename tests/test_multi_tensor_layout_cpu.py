"""Layout contract of the multi-tensor ops, the parts that need no GPU.

The fused SGD / cast / scale kernels index param, grad and momentum (or src
and dst) by ONE flat offset, so the tensors of a slot must share a memory
order.  Checked here: the reducer hands every param a gradient view in the
param's own strides (torch's gradient layout contract), and FusedSGD routes
any triple that breaks the contract to the logically indexed per-tensor
loop instead of the flat kernel.
"""

import warnings

import pytest
import torch

from amdtrain.ops import FusedSGD
from amdtrain.ops import functional as OF
from amdtrain.ops import sgd as sgd_mod
from amdtrain.parallel.reducer import BucketedReducer

CONTRACT_WARNING = "gradient layout contract"


def _resnet18_cl():
    from amdtrain.models import build_model
    torch.manual_seed(0)
    return build_model("resnet18", num_classes=10) \
        .to(memory_format=torch.channels_last)


def _assert_views(model, reducer):
    kxk = 0
    for b in reducer.buckets:
        lo = b.flat.data_ptr()
        hi = lo + b.flat.numel() * b.flat.element_size()
        for p in b.params:
            assert p.grad.shape == p.shape
            assert p.grad.stride() == p.stride(), (p.shape, p.grad.stride())
            assert lo <= p.grad.data_ptr() < hi
            if p.dim() == 4 and p.shape[2] * p.shape[3] > 1:
                kxk += 1
                assert not p.is_contiguous()  # really NHWC, not a no-op
    return kxk


def test_reducer_grads_keep_param_strides_resnet18():
    m = _resnet18_cl()
    params = list(m.parameters())
    r = BucketedReducer(params, bucket_cap_mb=1.0)
    assert len(r.buckets) >= 2
    assert _assert_views(m, r) == 17  # the stem 7x7 and sixteen 3x3

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        m(torch.randn(2, 3, 32, 32)
          .contiguous(memory_format=torch.channels_last)).sum().backward()
    assert not [w for w in caught if CONTRACT_WARNING in str(w.message)]
    assert _assert_views(m, r) == 17
    assert any(p.grad.abs().max() > 0 for p in params)

    # still aliases of the buckets: zeroing the flats zeroes every grad
    r.zero_grad()
    for p in params:
        assert torch.count_nonzero(p.grad) == 0


def test_reducer_view_roundtrip_and_memory_order():
    m = _resnet18_cl()
    r = BucketedReducer(list(m.parameters()), bucket_cap_mb=1.0)
    for b in r.buckets:
        off = 0
        for p in b.params:
            n = p.numel()
            vals = torch.arange(n, dtype=p.dtype).view(p.shape) + 1
            with torch.no_grad():
                p.grad.copy_(vals)  # one distinct value per LOGICAL index
            piece = b.flat[off:off + n]
            # the slice holds exactly this param's values, nothing else's
            assert torch.equal(piece.sort().values, vals.reshape(-1))
            # in the param's memory order ...
            if p.dim() == 4:
                assert torch.equal(piece,
                                   vals.permute(0, 2, 3, 1).reshape(-1))
            else:
                assert torch.equal(piece, vals.reshape(-1))
            # ... and reading back through the same view is the identity
            assert torch.equal(piece.as_strided(p.size(), p.stride()), vals)
            off += n
        assert off == b.flat.numel()


def test_layout_predicates():
    a = torch.randn(8, 4, 3, 3)
    cl = a.contiguous(memory_format=torch.channels_last)
    assert OF.mt_dense(a) and OF.mt_dense(cl)
    assert OF.mt_dense(a.permute(1, 0, 3, 2))  # dense, neither format
    assert not OF.mt_dense(a[:, ::2])
    assert not OF.mt_dense(a.expand(2, 8, 4, 3, 3))
    assert OF.mt_dense(torch.empty(0, 3)[:, ::2])
    assert OF.mt_same_layout(cl, cl.clone(), torch.zeros_like(cl))
    assert not OF.mt_same_layout(cl, a)
    assert not OF.mt_same_layout(a, cl)
    assert not OF.mt_same_layout(a, a.reshape(8, 4, 9))
    assert not OF.mt_same_layout(a[:, ::2], a[:, ::2])
    # size-1 dims address nothing: a channels_last 1x1 weight and its
    # row-major gradient share one memory order
    w = torch.randn(8, 4, 1, 1)
    wcl = torch.empty_strided((8, 4, 1, 1), (4, 1, 4, 4)).copy_(w)
    assert wcl.is_contiguous(memory_format=torch.channels_last)
    assert OF.mt_same_layout(wcl, w) and OF.mt_same_layout(w, wcl)


class _StubExt:
    def __init__(self):
        self.calls = []

    def multi_tensor_sgd(self, params, grads, bufs, *args):
        self.calls.append((list(params), list(grads), list(bufs), args))


@pytest.fixture
def stub_ext(monkeypatch):
    stub = _StubExt()
    monkeypatch.setattr(FusedSGD, "_ext_serves", staticmethod(lambda ps: True))
    monkeypatch.setattr(sgd_mod, "require_ext", lambda: stub)
    return stub


def _cl_param(shape):
    return torch.nn.Parameter(
        torch.randn(shape).contiguous(memory_format=torch.channels_last))


def test_fused_sgd_route_matching_layout_goes_fused(stub_ext):
    ps = [_cl_param((8, 4, 3, 3)), _cl_param((8, 4, 1, 1)),
          torch.nn.Parameter(torch.randn(10))]
    opt = FusedSGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-4)
    for p in ps:
        p.grad = torch.randn_like(p)  # preserve_format: the param's strides
    ps[1].grad = torch.randn(8, 4, 1, 1)  # row-major 1x1: same memory order
    opt.step(zero_grad=True)
    assert (opt.last_step_fused, opt.last_step_loop) == (1, 0)
    (params, grads, bufs, args), = stub_ext.calls
    assert [id(p) for p in params] == [id(p) for p in ps]
    assert all(g is p.grad for g, p in zip(grads, ps))
    assert all(b.stride() == p.stride() for b, p in zip(bufs, ps))
    assert args == (0.1, 0.9, 1e-4, False, True, True)


@pytest.mark.parametrize("case", ["contiguous_grad", "nondense_param",
                                  "nondense_grad", "foreign_buffer"])
def test_fused_sgd_route_bad_layout_goes_loop(stub_ext, case):
    torch.manual_seed(1)
    good = torch.nn.Parameter(torch.randn(10))
    good.grad = torch.randn(10)
    if case == "nondense_param":
        bad = torch.nn.Parameter(torch.randn(8, 8, 3, 3)[:, ::2])
    else:
        bad = _cl_param((8, 4, 3, 3))
    if case == "contiguous_grad":
        bad.grad = torch.randn(8, 4, 3, 3)
    elif case == "nondense_grad":
        bad.grad = torch.randn(8, 8, 3, 3).contiguous(
            memory_format=torch.channels_last)[:, ::2]
    else:
        bad.grad = torch.randn_like(bad)
    opt = FusedSGD([good, bad], lr=0.1, momentum=0.9)
    if case == "foreign_buffer":  # e.g. a checkpoint loaded row-major
        opt.state[bad]["momentum_buffer"] = torch.zeros(8, 4, 3, 3)
        opt.state[good]["momentum_buffer"] = torch.zeros(10)
    before = bad.detach().clone()
    opt.step()
    assert (opt.last_step_fused, opt.last_step_loop) == (0, 1)
    assert stub_ext.calls == []
    assert not torch.equal(bad, before)  # the loop did the update


@pytest.mark.parametrize("nesterov", [False, True])
def test_step_loop_matches_torch_sgd_channels_last_param_contiguous_grad(
        nesterov):
    torch.manual_seed(2)
    shapes = [(16, 8, 3, 3), (8, 3, 7, 7), (8, 8, 1, 3), (8, 4, 1, 1), (5,)]
    ps = [_cl_param(s) if len(s) == 4 else
          torch.nn.Parameter(torch.randn(s)) for s in shapes]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=nesterov)
    ours = FusedSGD(ps, **kw)
    ref = torch.optim.SGD(qs, foreach=False, **kw)
    for step in range(3):
        for p, q in zip(ps, qs):
            g = torch.randn(p.shape)  # row-major, as the old bucket views
            assert (len(p.shape) != 4 or p.shape[2] * p.shape[3] == 1
                    or g.stride() != p.stride())
            p.grad = g.clone()
            q.grad = g.clone()
        ours.step(zero_grad=True)
        ref.step()
        assert (ours.last_step_fused, ours.last_step_loop) == (0, 1)
    for p, q in zip(ps, qs):
        assert p.stride() == q.stride()
        assert torch.allclose(p, q, rtol=0, atol=1e-6), (p - q).abs().max()
        assert torch.count_nonzero(p.grad) == 0
