"""Multi-tensor SGD / cast / scale+check against fp64 (or exact) references.

The three ops (ops/csrc/sgd.hip, ops/csrc/elementwise.hip, driven by
mt_apply in ops/csrc/common.h) walk every tensor as one flat run of numel()
elements.  Tested here, with every reference built from plain torch ops in
fp64 (or an exact torch cast) on the same device and indexed logically:

  * the SGD recurrence over momentum x nesterov x weight decay x zero_grad,
    first step included, through raw ``_C`` and through ``FusedSGD``;
  * every launch edge of mt_apply: chunk boundaries, the 24-tensor flush,
    the 320-block flush mid-tensor and on a tensor boundary, empty tensors;
  * pointers at element offsets 0..3 inside flat buffers (float4 path vs
    scalar path, bit-identical);
  * casts between fp32 / bf16 / fp16 bit-for-bit, specials included;
  * scale + non-finite flag, including overflow on the store to fp16;
  * the layout contract: channels_last triples go fused and match the
    logical reference, mixed layouts are refused by ``_C`` before any launch
    and rerouted by the Python wrappers;
  * a real model under BucketedReducer, and AMP O2, against a twin stepped
    by torch.optim.SGD from logically copied gradients.

SGD tolerance.  On the same inputs torch.optim.SGD(foreach=False) in fp32 is
compared with the fp64 recurrence; its largest error over the case is E_ref.
The kernel may be off by 4 * E_ref (fma contraction and evaluation order
differ) plus 1 ulp of |p|.  E_ref is measured in every case, not assumed.
"""

import copy
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

# ops/csrc/common.h: constexpr int MT_TENSORS = 24; constexpr int MT_BLOCKS =
# 320; constexpr long MT_CHUNK = 1 << 16.  The edge cases below are built
# from these three numbers; after a retune they no longer sit on the edges,
# so test_mt_constants_match_header fails until they are updated together.
MT_TENSORS = 24
MT_BLOCKS = 320
MT_CHUNK = 1 << 16

SENTINEL = 7.5  # exact in fp32, bf16 and fp16
CANARY = 64

FLOATS = [torch.float32, torch.bfloat16, torch.float16]


def _ext():
    from amdtrain.ops import functional as OF
    assert OF.ext_available(), (
        "amdtrain._C must be built in-tree on the GPU box")
    return OF.require_ext()


def test_mt_constants_match_header():
    import os
    import re
    import amdtrain
    path = os.path.join(os.path.dirname(amdtrain.__file__), "ops", "csrc",
                        "common.h")
    text = open(path).read()
    found = {
        "MT_TENSORS": re.search(r"MT_TENSORS\s*=\s*(\d+)\s*;", text),
        "MT_BLOCKS": re.search(r"MT_BLOCKS\s*=\s*(\d+)\s*;", text),
        "MT_CHUNK": re.search(r"MT_CHUNK\s*=\s*1\s*<<\s*(\d+)\s*;", text),
    }
    assert all(found.values()), found
    assert int(found["MT_TENSORS"].group(1)) == MT_TENSORS
    assert int(found["MT_BLOCKS"].group(1)) == MT_BLOCKS
    assert 1 << int(found["MT_CHUNK"].group(1)) == MT_CHUNK


# ---------------------------------------------------------------- helpers

def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _assert_same_bits(got, want, what=""):
    """Bit-for-bit, except that NaNs only have to be NaNs."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    gn, wn = got.isnan(), want.isnan()
    assert torch.equal(gn, wn), f"{what}: NaN positions differ"
    diff = (_bits(got) != _bits(want)) & ~wn
    n = int(diff.sum())
    if n:
        i = int(diff.reshape(-1).nonzero()[0, 0])
        raise AssertionError(
            f"{what}: {n} elements differ, first at flat index {i}: got "
            f"{got.reshape(-1)[i].item()!r}, want "
            f"{want.reshape(-1)[i].item()!r}")


def _carve(numels, dtype, offsets=(0,), canary=0):
    """One flat allocation with a 1-D view per entry.  View i starts
    offsets[i % len(offsets)] elements past a 16-byte boundary and is
    followed by `canary` guard elements.  Everything starts as SENTINEL."""
    per16 = 16 // torch.empty((), dtype=dtype).element_size()
    pos, spans = 0, []
    for i, n in enumerate(numels):
        pos = -(-pos // per16) * per16 + offsets[i % len(offsets)]
        spans.append((pos, n))
        pos += n + canary
    flat = torch.full((pos + per16,), SENTINEL, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    return flat, [flat[a:a + n] for a, n in spans]


def _ulp32(x64):
    a = x64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _ref_step(p, g, b, first, lr, mu, wd, nesterov):
    """The recurrence in fp64: g' = g + wd*p; b = first ? g' : mu*b + g';
    u = nesterov ? g' + mu*b : b; p -= lr*u."""
    g = g + wd * p
    if mu != 0:
        b = g.clone() if first else mu * b + g
        u = g + mu * b if nesterov else b
    else:
        u = g
    return p - lr * u, b


def _max_err(got32, ref64):
    errs = [(a.detach().double() - r).abs().max()
            for a, r in zip(got32, ref64) if r.numel()]
    return float(torch.stack(errs).max()) if errs else 0.0


def _check_close(what, got32, ref64, e_ref):
    for i, (a, r) in enumerate(zip(got32, ref64)):
        if not r.numel():
            continue
        err = (a.detach().double() - r).abs()
        bad = err > 4 * e_ref + _ulp32(r)
        n = int(bad.sum())
        assert n == 0, (
            f"{what}[{i}] shape {tuple(a.shape)}: {n} elements beyond "
            f"4*E_ref + 1 ulp; max err {float(err.max()):.3e}, "
            f"E_ref {e_ref:.3e}")


def _run_sgd(ps, gs, bs, *, lr=0.1, mu=0.9, wd=1e-4, nesterov=False,
             zero_grad=False, steps=3, mode="raw", route="fused",
             same_data=False, seed=0):
    """Drive `steps` SGD steps over the given device tensors (param, grad and
    momentum-buffer lists) through raw _C ("raw") or FusedSGD ("opt"), next
    to the fp64 recurrence and to torch.optim.SGD(foreach=False) in fp32,
    and check params, buffers and grads after every step."""
    from amdtrain.ops import FusedSGD
    C = _ext()
    gen = torch.Generator(device=DEV).manual_seed(seed)

    def rnd(t):
        return torch.randn(t.shape, generator=gen, device=DEV)

    with torch.no_grad():
        base = rnd(ps[0]) if same_data else None
        for p in ps:
            p.copy_(base if same_data else rnd(p))
        for b in bs:
            b.fill_(SENTINEL)
    p64 = [p.detach().double() for p in ps]
    b64 = [None] * len(ps)
    qs = [nn.Parameter(p.detach().clone()) for p in ps]
    tref = torch.optim.SGD(qs, lr=lr, momentum=mu, weight_decay=wd,
                           nesterov=bool(nesterov and mu != 0), foreach=False)
    if mode == "opt":
        params = [nn.Parameter(p) for p in ps]  # same storage, same strides
        opt = FusedSGD(params, lr=lr, momentum=mu, weight_decay=wd,
                       nesterov=nesterov)
    worst = 0.0
    for step in range(steps):
        first = step == 0
        gb = rnd(gs[0]) if same_data else None
        news = [gb if same_data else rnd(g) for g in gs]
        with torch.no_grad():
            for g, q, n in zip(gs, qs, news):
                g.copy_(n)
                q.grad = torch.empty_like(q).copy_(n)
        if mode == "raw":
            C.multi_tensor_sgd(ps, gs, bs, lr, mu, wd, nesterov,
                               first and mu != 0, zero_grad)
            got_b = bs
        else:
            for p, g in zip(params, gs):
                p.grad = g
            opt.step(zero_grad=zero_grad)
            want = (1, 0) if route == "fused" else (0, 1)
            assert (opt.last_step_fused, opt.last_step_loop) == want
            got_b = [opt.state[p].get("momentum_buffer") for p in params]
        tref.step()
        for i in range(len(ps)):
            p64[i], b64[i] = _ref_step(p64[i], news[i].double(), b64[i],
                                       first, lr, mu, wd, nesterov)

        e_ref = _max_err(qs, p64)
        worst = max(worst, _max_err(ps, p64))
        _check_close(f"step {step} param", ps, p64, e_ref)
        if mu != 0:
            tb = [tref.state[q]["momentum_buffer"] for q in qs]
            _check_close(f"step {step} momentum", got_b, b64,
                         _max_err(tb, b64))
        elif mode == "raw":  # the "unused" argument really is unused
            for b in bs:
                assert torch.equal(b, torch.full_like(b, SENTINEL))
        else:
            assert all(b is None for b in got_b)
        for g, n in zip(gs, news):
            if zero_grad:  # exactly +0.0 everywhere
                assert torch.count_nonzero(_bits(g)) == 0
            else:
                assert torch.equal(g, n)
    print(f"SGD {mode} mu={mu} nesterov={nesterov} wd={wd} zg={zero_grad}: "
          f"E_ref(torch fp32 vs fp64)={e_ref:.3e} kernel max err={worst:.3e}")
    return ps, got_b


# ----------------------------------------------------------- SGD recurrence

# Measured on an MI355X with these inputs (randn params and grads): E_ref,
# the error of torch.optim.SGD(foreach=False) in fp32 against the fp64
# recurrence, is 2.7e-7 .. 3.4e-7 after the 3 steps of the 16 cases below
# and 3.6e-7 .. 4.9e-7 over the launch-edge lists; that is within 1 ulp of
# the largest |p| (ulp(4) = 4.8e-7).  The kernel's own error was 2.7e-7 ..
# 4.8e-7, equal to torch's in most cases.  The tiny model under the reducer
# and AMP O2 gave E_ref = 7.7e-8 and 7.3e-8 with the same kernel error.
HP = [(mu, nest, wd, zg) for mu in (0.0, 0.9) for nest in (False, True)
      for wd in (0.0, 1e-4) for zg in (False, True)]


def _small_lists():
    numels = [1, 3, 4, 5, 1000, 4099]
    _, ps = _carve(numels, torch.float32, offsets=(0, 1, 2, 3))
    _, gs = _carve(numels, torch.float32, offsets=(2, 0, 3, 1, 0))
    _, bs = _carve(numels, torch.float32, offsets=(3, 3, 0))
    return ps, gs, bs


@pytest.mark.parametrize("mu,nesterov,wd,zero_grad", HP)
def test_sgd_recurrence_raw(mu, nesterov, wd, zero_grad):
    ps, gs, bs = _small_lists()
    _run_sgd(ps, gs, bs, mu=mu, nesterov=nesterov, wd=wd,
             zero_grad=zero_grad, mode="raw")


# FusedSGD (like torch.optim.SGD) refuses nesterov without momentum
@pytest.mark.parametrize("mu,nesterov,wd,zero_grad",
                         [h for h in HP if h[0] != 0 or not h[1]])
def test_sgd_recurrence_fused_sgd(mu, nesterov, wd, zero_grad):
    ps, gs, bs = _small_lists()
    _run_sgd(ps, gs, bs, mu=mu, nesterov=nesterov, wd=wd,
             zero_grad=zero_grad, mode="opt")


# ------------------------------------------------- chunk and launch edges

def _fifty():
    # two 24-tensor flushes (after list index 23 and 47); empty tensors in
    # the middle, in the last slot before a flush and in the first after it;
    # multi-chunk tensors on both sides of each flush
    numels = [17 + 3 * i for i in range(50)]
    numels[10] = 0
    numels[22] = MT_CHUNK + 1
    numels[23] = 0
    numels[24] = 0
    numels[25] = MT_CHUNK + 3
    numels[47] = 2 * MT_CHUNK + 5
    numels[48] = MT_CHUNK
    return numels


EDGE_LISTS = {
    "chunk_edges": [0, 1, 3, 4, 5, MT_CHUNK - 1, MT_CHUNK, MT_CHUNK + 1,
                    MT_CHUNK + 3, 2 * MT_CHUNK + 5],
    "fifty_tensors": _fifty(),
    # 1 + 4 chunks, then 322: the 320-block flush lands inside the third
    # tensor and the re-seeded slot 0 finishes it
    "block_flush_mid_tensor": [7, 3 * MT_CHUNK + 1, 321 * MT_CHUNK + 3, 1000],
    # exactly MT_BLOCKS chunks, the last one partial, and nothing after
    "block_flush_at_end": [100 * MT_CHUNK, 219 * MT_CHUNK + 17],
    # the same, with one more tensor after the flush
    "block_flush_then_more": [100 * MT_CHUNK, 219 * MT_CHUNK + 17, 9],
}
assert len(EDGE_LISTS["fifty_tensors"]) == 50 > 2 * MT_TENSORS
assert -(-EDGE_LISTS["block_flush_at_end"][0] // MT_CHUNK) + \
    -(-EDGE_LISTS["block_flush_at_end"][1] // MT_CHUNK) == MT_BLOCKS


@pytest.mark.parametrize("name", list(EDGE_LISTS))
def test_sgd_launch_edges(name):
    numels = EDGE_LISTS[name]
    _, ps = _carve(numels, torch.float32, offsets=(0, 1, 0, 0, 2))
    _, gs = _carve(numels, torch.float32, offsets=(0, 0, 3, 0))
    _, bs = _carve(numels, torch.float32, offsets=(0, 0, 0, 1))
    _run_sgd(ps, gs, bs, mu=0.9, nesterov=True, wd=1e-4, zero_grad=True,
             steps=2, mode="raw")


def _fill_random(views, seed, lo=-4.0, hi=4.0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    for v in views:
        v.copy_(torch.empty(v.shape, device=DEV)
                .uniform_(lo, hi, generator=gen))


@pytest.mark.parametrize("pair", [(torch.float32, torch.float16),
                                  (torch.bfloat16, torch.float32)],
                         ids=["f32_f16", "bf16_f32"])
@pytest.mark.parametrize("name", list(EDGE_LISTS))
def test_cast_launch_edges(name, pair):
    C = _ext()
    numels = EDGE_LISTS[name]
    sflat, src = _carve(numels, pair[0], offsets=(0, 1, 3))
    dflat, dst = _carve(numels, pair[1], offsets=(0, 2, 1, 0), canary=CANARY)
    _fill_random(src, 1)
    want_flat = dflat.clone()
    sbefore = sflat.clone()
    C.multi_tensor_cast(src, dst)
    # the expected image of the WHOLE destination allocation: every element
    # of every tensor written, every guard element and gap untouched
    off = [d.storage_offset() for d in dst]
    for s, o in zip(src, off):
        want_flat[o:o + s.numel()] = s.to(pair[1])
    _assert_same_bits(dflat, want_flat, f"cast {name} destination")
    _assert_same_bits(sflat, sbefore, f"cast {name} source")


@pytest.mark.parametrize("name", list(EDGE_LISTS))
def test_scale_launch_edges(name):
    C = _ext()
    numels = EDGE_LISTS[name]
    flat, ts = _carve(numels, torch.float32, offsets=(0, 3, 1), canary=CANARY)
    _fill_random(ts, 2)
    want_flat = flat.clone()
    found = torch.full((1,), 0.5, device=DEV)
    C.multi_tensor_scale_check(ts, 0.375, found)
    for t in ts:  # an element scaled twice, or not at all, shows here
        o = t.storage_offset()
        want_flat[o:o + t.numel()] *= torch.tensor(0.375, device=DEV)
    _assert_same_bits(flat, want_flat, f"scale {name}")
    assert found.item() == 0.5  # clean data: the flag is not even written


# ------------------------------------------------------------- alignment

def test_sgd_alignment_scalar_and_float4_paths_agree():
    """64 triples with the same data, param / grad / momentum each carved at
    every element offset 0..3 of a flat buffer (independently): exactly one
    is 16-byte aligned in all three and takes the float4 path, nine more are
    aligned in two pointers and not the third.  All must give the same bits,
    and those must match the fp64 reference."""
    n = 1037  # float4 body + 1 tail element; 4 * 259 + 1
    combos = [(a, b, c) for a in range(4) for b in range(4) for c in range(4)]
    _, ps = _carve([n] * 64, torch.float32, offsets=[c[0] for c in combos])
    _, gs = _carve([n] * 64, torch.float32, offsets=[c[1] for c in combos])
    _, bs = _carve([n] * 64, torch.float32, offsets=[c[2] for c in combos])
    for (a, b, c), p, g, m in zip(combos, ps, gs, bs):
        assert (p.data_ptr() % 16, g.data_ptr() % 16, m.data_ptr() % 16) == \
            (4 * a, 4 * b, 4 * c)
    ps, bs = _run_sgd(ps, gs, bs, mu=0.9, nesterov=True, wd=1e-4,
                      zero_grad=False, steps=2, mode="raw", same_data=True)
    for k in range(1, 64):
        assert torch.equal(_bits(ps[k]), _bits(ps[0])), combos[k]
        assert torch.equal(_bits(bs[k]), _bits(bs[0])), combos[k]


def test_sgd_alignment_without_momentum():
    # mu == 0: the kernel's alignment test must ignore the unused pointer
    n = 1037
    combos = [(a, b) for a in range(4) for b in range(4)]
    _, ps = _carve([n] * 16, torch.float32, offsets=[c[0] for c in combos])
    _, gs = _carve([n] * 16, torch.float32, offsets=[c[1] for c in combos])
    _, bs = _carve([n] * 16, torch.float32, offsets=(1, 2, 3))
    ps, _ = _run_sgd(ps, gs, bs, mu=0.0, wd=1e-4, zero_grad=True, steps=2,
                     mode="raw", same_data=True)
    for k in range(1, 16):
        assert torch.equal(_bits(ps[k]), _bits(ps[0])), combos[k]


# ------------------------------------------------------------------ cast

def _special_sources():
    """Per source dtype, a 1-D tensor of inputs that casts get wrong."""
    inf, nan = float("inf"), float("nan")
    f16_sub = [2.0 ** -24 * k for k in (1, 2, 3, 511, 1023)]   # subnormal
    f16_sub += [2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20),     # tie -> 0, up
                3 * 2.0 ** -25, 2.0 ** -26, 2.0 ** -14 * (1 - 2.0 ** -12)]
    bf16_sub = [2.0 ** -133 * k for k in (1, 2, 3, 64, 127)]   # subnormal
    bf16_sub += [2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -135, 2.0 ** -149,
                 2.0 ** -127, 2.0 ** -126 * (1 - 2.0 ** -9)]
    ties = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23,
            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23,
            1 + 2.0 ** -8 - 2.0 ** -23, 2047.5, 2048.5, 0.1, 1 / 3]
    big = [65504.0, 65519.0, 65519.996, 65520.0, 65536.0, 70000.0, 1e5,
           1e38, 3.3895313892515355e38, 3.3961775292304983e38,
           3.4028234663852886e38]
    vals = [0.0, inf, nan, 1.0] + f16_sub + bf16_sub + ties + big
    vals = vals + [-v for v in vals]
    gen = torch.Generator(device=DEV).manual_seed(3)
    rand_bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (20000,), device=DEV,
                              dtype=torch.int64, generator=gen)
    f32 = torch.cat([torch.tensor(vals, dtype=torch.float64, device=DEV)
                     .float(), rand_bits.to(torch.int32).view(torch.float32)])
    # the 16-bit types exhaustively: every bit pattern
    all16 = torch.arange(-2 ** 15, 2 ** 15, device=DEV, dtype=torch.int16)
    return {torch.float32: f32, torch.float16: all16.view(torch.float16),
            torch.bfloat16: all16.view(torch.bfloat16)}


@pytest.fixture(scope="module")
def special_sources():
    return _special_sources()


def test_cast_every_pair_one_call_bit_exact(special_sources):
    """All nine (src, dst) dtype pairs in ONE call (six conversions, three
    same-type copies), so the grouping by pair is exercised too."""
    C = _ext()
    src, dst, guards = [], [], []
    for k, (sd, dd) in enumerate((s, d) for s in FLOATS for d in FLOATS):
        s = special_sources[sd]
        flat, (d,) = _carve([s.numel()], dd, offsets=(k % 4,), canary=CANARY)
        src.append(s)
        dst.append(d)
        guards.append((flat, d.storage_offset(), s.numel()))
    before = [s.clone() for s in src]
    C.multi_tensor_cast(src, dst)
    for s, b, d, (flat, o, n) in zip(src, before, dst, guards):
        what = f"{s.dtype} -> {d.dtype}"
        _assert_same_bits(d, s.to(d.dtype), what)
        _assert_same_bits(s, b, what + " source")
        rest = torch.cat([flat[:o], flat[o + n:]])
        assert torch.equal(rest, torch.full_like(rest, SENTINEL)), what


# ----------------------------------------------------------- scale + check

def _scale_lists():
    """Mixed list: 30 fp32 tensors (past the 24-tensor flush, one of them
    multi-chunk and late), then fp16 and bf16 groups."""
    numels = [33 + i for i in range(30)]
    numels[28] = 2 * MT_CHUNK + 5
    flat32, t32 = _carve(numels, torch.float32, offsets=(0, 1, 2, 3),
                         canary=CANARY)
    flat16, t16 = _carve([100, MT_CHUNK + 3, 7], torch.float16,
                         offsets=(0, 1, 5), canary=CANARY)
    flatbf, tbf = _carve([50, MT_CHUNK + 1, 9], torch.bfloat16,
                         offsets=(0, 3, 7), canary=CANARY)
    _fill_random(t32 + t16 + tbf, 4, -100.0, 100.0)
    return [flat32, flat16, flatbf], t32, t16, tbf


def _scale_expect(flats, tensors, scale):
    want = [f.clone() for f in flats]
    by_ptr = {f.untyped_storage().data_ptr(): w for f, w in zip(flats, want)}
    s32 = torch.tensor(scale, dtype=torch.float32, device=DEV)
    for t in tensors:
        w = by_ptr[t.untyped_storage().data_ptr()]
        o = t.storage_offset()
        w[o:o + t.numel()] = (t.float() * s32).to(t.dtype)
    return want


@pytest.mark.parametrize("scale", [1.0 / 65536, 0.1, 3.0])
def test_scale_mixed_dtypes_bit_exact(scale):
    C = _ext()
    flats, t32, t16, tbf = _scale_lists()
    # interleaved, so the op has to group by dtype itself
    tensors = t32[:5] + t16[:1] + tbf[:2] + t32[5:] + t16[1:] + tbf[2:]
    want = _scale_expect(flats, tensors, scale)
    found = torch.full((1,), 0.5, device=DEV)
    C.multi_tensor_scale_check(tensors, scale, found)
    for f, w in zip(flats, want):
        _assert_same_bits(f, w, f"scale {f.dtype} x {scale}")
    assert found.item() == 0.5


BAD_CASES = {
    # (which list, tensor index, element index, value, scale)
    "last_element_of_last_chunk_of_late_tensor": ("t32", 28, -1,
                                                  float("inf"), 0.5),
    "tensor_after_the_24_tensor_flush": ("t32", 26, 0, float("-inf"), 0.5),
    "fp16_group": ("t16", 1, MT_CHUNK + 2, float("inf"), 0.5),
    "bf16_group": ("tbf", 1, MT_CHUNK, float("inf"), 0.5),
    "nan_not_inf": ("t32", 3, 17, float("nan"), 0.5),
    "nan_in_fp16": ("t16", 2, 6, float("nan"), 0.5),
    # finite as an fp32 product, inf once stored: 40000 * 2 > 65504
    "fp16_overflow_on_store": ("t16", 1, 12345, 40000.0, 2.0),
    "fp16_overflow_on_store_negative": ("t16", 0, 99, -40000.0, 2.0),
    # 3.3895e38 is bf16's largest; * 1.0039 is still a finite fp32
    "bf16_overflow_on_store": ("tbf", 2, 8, 3.3895313892515355e38,
                               1.00390625),
}


@pytest.mark.parametrize("case", list(BAD_CASES))
def test_scale_found_inf(case):
    C = _ext()
    which, ti, ei, value, scale = BAD_CASES[case]
    flats, t32, t16, tbf = _scale_lists()
    if scale > 1:  # keep every other element finite after the multiply
        for t in t32 + t16 + tbf:
            t.mul_(0.01)
    tensors = t32 + t16 + tbf
    {"t32": t32, "t16": t16, "tbf": tbf}[which][ti][ei] = value
    want = _scale_expect(flats, tensors, scale)
    n_bad = sum(int((~torch.isfinite(w)).sum()) for w in want)
    assert n_bad == 1, "the case must contain exactly one non-finite result"
    found = torch.full((1,), 0.5, device=DEV)
    C.multi_tensor_scale_check(tensors, scale, found)
    for f, w in zip(flats, want):
        _assert_same_bits(f, w, f"{case} {f.dtype}")
    assert found.item() == 1.0
    # the flag is sticky: a following clean call must not clear it
    clean = [torch.ones(100, device=DEV),
             torch.ones(10, device=DEV, dtype=torch.float16)]
    C.multi_tensor_scale_check(clean, 0.5, found)
    assert found.item() == 1.0
    assert all(bool((c == 0.5).all()) for c in clean)


# ---------------------------------------------------------------- layouts

CL_SHAPES = [(16, 8, 3, 3), (8, 3, 7, 7), (8, 8, 1, 3), (16, 16, 1, 1), (10,)]


def _cl(shape):
    t = torch.zeros(shape, device=DEV)
    return t.contiguous(memory_format=torch.channels_last) \
        if len(shape) == 4 else t


@pytest.mark.parametrize("mode", ["raw", "opt"])
def test_sgd_channels_last_triples_go_fused(mode):
    ps = [_cl(s) for s in CL_SHAPES]
    assert not ps[0].is_contiguous() and not ps[2].is_contiguous()
    _run_sgd(ps, [_cl(s) for s in CL_SHAPES], [_cl(s) for s in CL_SHAPES],
             mu=0.9, wd=1e-4, nesterov=True, zero_grad=True, mode=mode,
             route="fused")


def test_sgd_channels_last_params_contiguous_grads_fused_sgd_falls_back():
    ps = [_cl(s) for s in CL_SHAPES]
    gs = [torch.zeros(s, device=DEV) for s in CL_SHAPES]  # row-major
    assert gs[0].stride() != ps[0].stride()
    _run_sgd(ps, gs, [_cl(s) for s in CL_SHAPES], mu=0.9, wd=1e-4,
             nesterov=True, zero_grad=True, mode="opt", route="loop")


def _snapshot(lists):
    return [[t.clone() for t in ts] for ts in lists]


def _assert_untouched(lists, snap):
    torch.cuda.synchronize()
    for ts, ss in zip(lists, snap):
        for t, s in zip(ts, ss):
            assert torch.equal(t, s), "a kernel ran before the host check"


def _good_triple(n=1000):
    return (torch.randn(n, device=DEV), torch.randn(n, device=DEV),
            torch.randn(n, device=DEV))


@pytest.mark.parametrize("case", [
    "contiguous_grad", "contiguous_momentum", "nondense_param",
    "nondense_grad", "numel_mismatch_grad", "numel_mismatch_momentum",
    "same_numel_other_shape", "fp16_grad", "cpu_grad"])
def test_sgd_raw_refuses_before_any_launch(case):
    """Host checks only: every bad triple sits AFTER a good one in the list,
    and the good one must be untouched too, so nothing was launched."""
    C = _ext()
    torch.manual_seed(5)
    shape = (16, 8, 3, 3)
    p = torch.randn(shape, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    g, b = torch.randn_like(p), torch.zeros_like(p)
    msg = "memory order"
    if case == "contiguous_grad":
        g = torch.randn(shape, device=DEV)
    elif case == "contiguous_momentum":
        b = torch.zeros(shape, device=DEV)
    elif case == "nondense_param":
        w = torch.randn(16, 16, 3, 3, device=DEV)
        p, g, b = w[:, ::2], torch.randn_like(w)[:, ::2], \
            torch.zeros_like(w)[:, ::2]
        assert p.stride() == g.stride() == b.stride()
        msg = "not dense"
    elif case == "nondense_grad":
        g = torch.randn(16, 16, 3, 3, device=DEV).contiguous(
            memory_format=torch.channels_last)[:, ::2]
        msg = "not dense"
    elif case == "numel_mismatch_grad":
        g = torch.randn(16, 8, 3, 2, device=DEV)
        msg = "sizes"
    elif case == "numel_mismatch_momentum":
        b = torch.zeros(15, 8, 3, 3, device=DEV)
        msg = "sizes"
    elif case == "same_numel_other_shape":
        g = torch.randn(16, 8, 9, device=DEV)
        msg = "sizes"
    elif case == "fp16_grad":
        g = g.half()
        msg = "fp32"
    elif case == "cpu_grad":
        g = g.cpu()
        msg = "expected cuda"
    good = _good_triple()
    lists = [[good[0], p], [good[1], g], [good[2], b]]
    snap = _snapshot(lists)
    with pytest.raises(RuntimeError, match=msg):
        C.multi_tensor_sgd(*lists, 0.1, 0.9, 1e-4, False, True, True)
    _assert_untouched(lists, snap)


def test_sgd_raw_error_names_index_and_strides():
    C = _ext()
    p = _cl((16, 8, 3, 3))
    good = _good_triple()
    with pytest.raises(RuntimeError) as e:
        C.multi_tensor_sgd([good[0], p], [good[1], torch.zeros(
            16, 8, 3, 3, device=DEV)], [good[2], torch.zeros_like(p)],
            0.1, 0.9, 0.0, False, True, False)
    text = str(e.value)
    assert "grads[1]" in text
    assert "[72, 9, 3, 1]" in text and "[72, 1, 24, 8]" in text


def test_cast_and_scale_raw_refuse_before_any_launch():
    C = _ext()
    src = torch.randn(16, 8, 3, 3, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    ok_s, ok_d = torch.randn(100, device=DEV), \
        torch.zeros(100, device=DEV, dtype=torch.bfloat16)
    for dst, msg in [
            (torch.zeros(16, 8, 3, 3, device=DEV, dtype=torch.float16),
             "memory order"),
            (torch.zeros(16, 8, 3, 2, device=DEV, dtype=torch.float16),
             "sizes"),
            (torch.zeros(16, 16, 3, 3, device=DEV, dtype=torch.float16)
             .contiguous(memory_format=torch.channels_last)[:, ::2],
             "not dense"),
            (torch.zeros(16, 8, 3, 3, device=DEV, dtype=torch.int32)
             .contiguous(memory_format=torch.channels_last), "Int")]:
        lists = [[ok_s, src], [ok_d, dst]]
        snap = _snapshot(lists)
        with pytest.raises(RuntimeError, match=msg):
            C.multi_tensor_cast(*lists)
        _assert_untouched(lists, snap)

    found = torch.full((1,), 0.5, device=DEV)
    ok = torch.randn(100, device=DEV)
    bad = torch.randn(16, 16, device=DEV)[:, ::2]
    snap = _snapshot([[ok, bad, found]])
    with pytest.raises(RuntimeError, match="not dense"):
        C.multi_tensor_scale_check([ok, bad], 0.5, found)
    with pytest.raises(RuntimeError, match="found_inf"):
        C.multi_tensor_scale_check([ok], 0.5, found.cpu())
    _assert_untouched([[ok, bad, found]], snap)


def test_functional_wrappers_reroute_offending_tensors():
    """functional.multi_tensor_cast / _scale_check: pairs that break the
    contract take copy_ / mul_, the others still go through the kernel, and
    the result is logically right either way."""
    from amdtrain.ops import functional as OF
    _ext()
    torch.manual_seed(6)
    cl = torch.randn(16, 8, 3, 3, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    flat = torch.randn(3000, device=DEV)
    strided = torch.randn(16, 16, device=DEV)[:, ::2]
    src = [flat, cl, strided, cl]
    dst = [torch.zeros(3000, device=DEV, dtype=torch.float16),
           torch.zeros(16, 8, 3, 3, device=DEV, dtype=torch.float16),
           torch.zeros(16, 8, device=DEV, dtype=torch.bfloat16),
           torch.zeros_like(cl, dtype=torch.bfloat16)]
    assert dst[1].stride() != cl.stride() and dst[3].stride() == cl.stride()
    OF.multi_tensor_cast(src, dst)
    for s, d in zip(src, dst):
        _assert_same_bits(d, s.to(d.dtype), "wrapper cast")

    ts = [flat.clone(), strided.clone()[:, ::1],
          torch.randn(16, 16, device=DEV)[:, ::2], cl.half()]
    ts[2][3, 5] = float("inf")
    want = [(t.float() * 0.25).to(t.dtype) for t in ts]
    found = torch.zeros(1, device=DEV)
    OF.multi_tensor_scale_check(ts, 0.25, found)
    for t, w in zip(ts, want):
        _assert_same_bits(t, w, "wrapper scale")
    assert found.item() == 1.0  # the bad value sat in the rerouted tensor


# ------------------------------------------ a real model under the reducer

class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 8, 7, padding=3, bias=False)
        self.bn = nn.BatchNorm2d(8)
        self.conv2 = nn.Conv2d(8, 16, 3, padding=1, bias=False)
        self.conv3 = nn.Conv2d(16, 16, 1, bias=False)
        self.fc = nn.Linear(16, 10)

    def forward(self, x):
        x = F.relu(self.bn(self.conv1(x)))
        x = F.relu(self.conv3(F.relu(self.conv2(x))))
        return self.fc(x.mean((2, 3)))


SGD_KW = dict(lr=0.1, momentum=0.9, weight_decay=1e-4)


def _batch(step, dtype=torch.float32):
    gen = torch.Generator(device=DEV).manual_seed(100 + step)
    x = torch.randn(4, 3, 16, 16, device=DEV, generator=gen).to(dtype) \
        .contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, 10, (4,), device=DEV, generator=gen)
    return x, t


def reducer_vs_twin():
    """Two FusedSGD steps of the tiny channels_last model whose grads are
    BucketedReducer bucket views, next to a twin stepped by torch.optim.SGD
    from logically copied grads and to the fp64 recurrence."""
    from amdtrain.ops import FusedSGD
    from amdtrain.parallel.reducer import BucketedReducer
    torch.manual_seed(0)
    model = _Tiny().to(DEV).to(memory_format=torch.channels_last)
    twin = copy.deepcopy(model)
    names = [n for n, _ in model.named_parameters()]
    ps, qs = list(model.parameters()), list(twin.parameters())
    red = BucketedReducer(ps, bucket_cap_mb=0.005)
    opt = FusedSGD(ps, **SGD_KW)
    tref = torch.optim.SGD(qs, foreach=False, **SGD_KW)
    p64 = [p.detach().double() for p in ps]
    b64 = [None] * len(ps)
    routes = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for step in range(2):
            red.zero_grad()
            x, t = _batch(step)
            F.cross_entropy(model(x), t).backward()
            for p, q in zip(ps, qs):
                q.grad = torch.empty_like(q).copy_(p.grad)  # logical copy
            g64 = [p.grad.double() for p in ps]
            opt.step()
            tref.step()
            routes.append((getattr(opt, "last_step_fused", None),
                           getattr(opt, "last_step_loop", None)))
            for i in range(len(ps)):
                p64[i], b64[i] = _ref_step(
                    p64[i], g64[i], b64[i], step == 0, SGD_KW["lr"],
                    SGD_KW["momentum"], SGD_KW["weight_decay"], False)
    torch.cuda.synchronize()
    return dict(names=names, ps=ps, qs=qs, p64=p64, routes=routes,
                caught=caught, buckets=len(red.buckets))


def test_fused_sgd_under_reducer_matches_twin():
    r = reducer_vs_twin()
    assert r["buckets"] >= 2
    e_ref = _max_err(r["qs"], r["p64"])
    for n, p, q in zip(r["names"], r["ps"], r["qs"]):
        print(f"{n} {tuple(p.shape)}: max |fused - twin| = "
              f"{float((p - q).abs().max()):.3e}")
    print(f"E_ref (twin fp32 vs fp64) = {e_ref:.3e}, fused max err = "
          f"{_max_err(r['ps'], r['p64']):.3e}")
    _check_close("param", r["ps"], r["p64"], e_ref)
    for p in r["ps"]:  # the grads obey torch's gradient layout contract
        assert p.grad.stride() == p.stride()
    assert r["routes"] == [(1, 0), (1, 0)]  # and so the fused kernel ran
    assert not [w for w in r["caught"]
                if "gradient layout contract" in str(w.message)]


# ----------------------------------------------------------------- AMP O2

@pytest.mark.parametrize("with_reducer", [False, True])
def test_amp_o2_fp16_masters_match_fp64_update(with_reducer):
    from amdtrain.ops import FusedSGD
    from amdtrain.parallel import amp
    from amdtrain.parallel.reducer import BucketedReducer
    torch.manual_seed(0)
    model = _Tiny().to(DEV).to(memory_format=torch.channels_last)
    opt = FusedSGD(model.parameters(), **SGD_KW)
    scale = 128.0  # a power of two: unscaling is exact in fp32 and fp64
    model, opt = amp.initialize(model, opt, "O2", dtype=torch.float16,
                                init_scale=scale)
    h = opt._amp_handle
    assert len(h.master_params) == 5  # 3 conv weights + fc weight and bias
    red = BucketedReducer(list(model.parameters()), bucket_cap_mb=0.005) \
        if with_reducer else None
    if red is not None:
        assert len(red.buckets) >= 2
    half_of = {id(mp): hp for mp, hp in zip(h.master_params, h.model_params)}
    stepped = [p for g in opt.param_groups for p in g["params"]]
    assert len(stepped) == 7  # the masters and the two fp32 BN params
    qs = [nn.Parameter(p.detach().clone()) for p in stepped]
    tref = torch.optim.SGD(qs, foreach=False, **SGD_KW)
    p64 = [p.detach().double() for p in stepped]
    b64 = [None] * len(stepped)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for step in range(2):
            if red is not None:
                red.zero_grad()
            else:
                opt.zero_grad()
            x, t = _batch(step, torch.float16)
            loss = F.cross_entropy(model(x).float(), t)
            with amp.scale_loss(loss, opt) as scaled:
                scaled.backward()
            assert not h.found_inf and h.scaler.scale == scale
            # the gradient each stepped param must see, taken LOGICALLY from
            # where backward left it: the half grad (still scaled) for a
            # master, the already unscaled fp32 grad for a BN param
            g64 = [half_of[id(p)].grad.double() / scale
                   if id(p) in half_of else p.grad.double() for p in stepped]
            for q, g in zip(qs, g64):
                q.grad = torch.empty_like(q).copy_(g)  # exact: fp16 / 2**7
            opt.step()
            tref.step()
            assert (opt.last_step_fused, opt.last_step_loop) == (1, 0)
            for i in range(len(stepped)):
                p64[i], b64[i] = _ref_step(
                    p64[i], g64[i], b64[i], step == 0, SGD_KW["lr"],
                    SGD_KW["momentum"], SGD_KW["weight_decay"], False)
            e_ref = _max_err(qs, p64)
            print(f"AMP O2 step {step}: E_ref={e_ref:.3e} fused max err="
                  f"{_max_err(stepped, p64):.3e}")
            _check_close(f"step {step} master", stepped, p64, e_ref)
            for mp, hp in zip(h.master_params, h.model_params):
                assert hp.dtype == torch.float16
                _assert_same_bits(hp.detach(), mp.detach().to(torch.float16),
                                  "model half weight vs master")
    assert h.steps_skipped == 0
    assert not [w for w in caught
                if "gradient layout contract" in str(w.message)]
