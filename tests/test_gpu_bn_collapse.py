"""The BN partial fold (bn_collapse_partials): the streaming kernel against
the kernel it replaced and against the summation order spelled out in torch.
Per (slot, column) the fold starts from 0.f and adds rows slot, slot + slots,
... one by one in fp32, so all three must agree bit for bit."""

import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW, OLD = 1, 0

NPARTS = [1, 31, 32, 33, 2047, 2048, 2049, 12544, 75264]
TWO_C = [16, 48, 128, 1024, 4096, 6]   # 6: no 16-byte column groups


def _ext():
    from amdtrain.ops import functional as OF
    assert OF.ext_available()
    from amdtrain import _C
    return _C


def _slots(nparts):
    return 128 if nparts >= 2048 else 32


def _reference(parts):
    """acc = 0; acc += rows [i*slots, (i+1)*slots) for i = 0, 1, ... —
    elementwise fp32 adds, exact on either device; zero rows pad the tail
    (+0.f changes no bit of a sum that started from +0.f)."""
    nparts, two_c = parts.shape
    slots = _slots(nparts)
    if parts.numel() <= 1 << 24:
        parts = parts.cpu()
    iters = (nparts + slots - 1) // slots
    v = F.pad(parts, (0, 0, 0, iters * slots - nparts)) \
        .view(iters, slots, two_c)
    acc = torch.zeros(slots, two_c, dtype=torch.float32, device=v.device)
    for i in range(iters):
        acc += v[i]
    return acc


def _check(parts):
    C = _ext()
    new = C.bn_collapse_partials(parts, NEW)
    old = C.bn_collapse_partials(parts, OLD)
    assert new.shape == (_slots(parts.shape[0]), parts.shape[1])
    assert torch.equal(new, old)
    assert torch.equal(new.cpu(), _reference(parts).cpu())
    assert torch.equal(C.bn_collapse_partials(parts), new)  # the default


@pytest.mark.parametrize("two_c", TWO_C)
@pytest.mark.parametrize("nparts", NPARTS)
def test_fold_matches_old_kernel_and_spelled_order(nparts, two_c):
    g = torch.Generator(device=DEV).manual_seed(nparts * 8192 + two_c)
    parts = torch.randn(nparts, two_c, device=DEV, generator=g)
    _check(parts)


@pytest.mark.parametrize("nparts,two_c", [(33, 128), (2049, 48)])
def test_misaligned_base_takes_the_scalar_path(nparts, two_c):
    g = torch.Generator(device=DEV).manual_seed(7)
    buf = torch.randn(nparts * two_c + 1, device=DEV, generator=g)
    parts = buf[1:].view(nparts, two_c)
    assert parts.data_ptr() % 16 == 4
    _check(parts)


_CHILD = """
import sys, torch
sys.path.insert(0, sys.argv[1])
from amdtrain import _C
g = torch.Generator().manual_seed(5)
x = torch.randn(2, 64, 8, 8, generator=g).bfloat16().cuda() \\
    .contiguous(memory_format=torch.channels_last)
parts = torch.randn(2049, 128, generator=g).cuda()
w = torch.rand(64, generator=g).cuda() + 0.5
b = torch.randn(64, generator=g).cuda()
rm, rv = torch.zeros(64).cuda(), torch.ones(64).cuda()
out = _C.batch_norm_fwd_train_from_parts(x, parts, w, b, rm, rv, 0.1, 1e-5,
                                         True, None, False)
torch.cuda.synchronize()
torch.save([t.cpu() for t in out[:5]] + [rm.cpu(), rv.cpu()], sys.argv[2])
"""


def test_forward_from_parts_same_under_both_kernels(tmp_path):
    """batch_norm_fwd_train_from_parts over 2049 partial rows: y, mean,
    invstd, scale, shift and the running statistics do not depend on
    AMDTRAIN_BN_COLLAPSE (read once per process, hence two children)."""
    outs = []
    for flag in ("1", "0"):
        path = str(tmp_path / f"out{flag}.pt")
        env = dict(os.environ, AMDTRAIN_BN_COLLAPSE=flag)
        subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env,
                       check=True, timeout=120)
        outs.append(torch.load(path))
    assert torch.equal(outs[0][1], outs[1][1])  # mean
    for a, b in zip(*outs):
        assert torch.equal(a, b)
