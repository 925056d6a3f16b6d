"""svla_gemm_skinny (csrc/decode_batched.hip): y[M, N] = x[M, K] W^T for 1 <= M <= 64 on the weight-streaming MFMA
kernel -- against the fp32 product, exact integer sums, segments, the lm_head shape, batch invariance (row m has the
same bits for every M and every position), determinism and the refusals.

Bound: rel-L2 < 5e-3 against the fp32 product of the bf16 operands, the bound the decode-kernel tests use against fp32
restatements -- the bf16 rounding of the output alone is ~1e-3 (2^-9 / sqrt(3) relative per element), a wrong fragment
map is O(1)."""
import pytest
import torch

import harness as H
from spatialvla_amd import _lib as L
from spatialvla_amd import kernels as K

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TOL = 5e-3
SENTINEL = -7.0


def _r(cuda, g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(cuda)


def _out(cuda, m, n):
    return torch.full((m, n), SENTINEL, dtype=BF, device=cuda)


def _ref32(x, w):
    return x.float() @ w.float().t()


@pytest.mark.parametrize("N,Kd", [(48, 32), (203, 288), (1000, 2304), (64, 9216)])
@pytest.mark.parametrize("M", [9, 16, 17, 33, 64])
def test_store(cuda, M, N, Kd):
    g = torch.Generator().manual_seed(M * 1000 + N + Kd)
    x, w = _r(cuda, g, M, Kd), _r(cuda, g, N, Kd, scale=0.05)
    ld = K.round_up(N, 8) + 8
    buf = _out(cuda, M, ld)
    K.gemm_skinny(x, [w], buf)
    rel = H.rel_l2(buf[:, :N], _ref32(x, w))
    print(f"M={M} N={N} K={Kd}: rel-L2 {rel:.3e}")
    assert rel < TOL
    assert bool((buf[:, N:] == SENTINEL).all())  # columns >= N are not written


def test_three_unequal_segments(cuda):
    g = torch.Generator().manual_seed(3)
    Kd, sizes = 288, (32, 16, 24)
    x = _r(cuda, g, 17, Kd)
    ws = [_r(cuda, g, n, Kd, scale=0.05) for n in sizes]  # separate allocations
    one = torch.cat(ws, 0)
    a, b = _out(cuda, 17, 72), _out(cuda, 17, 72)
    K.gemm_skinny(x, [one], a)
    K.gemm_skinny(x, ws, b)
    assert H.rel_l2(a, _ref32(x, one)) < TOL
    assert torch.equal(a, b)


def test_head_shape(cuda):
    g = torch.Generator().manual_seed(5)
    N, Kd, M = 265347, 512, 33
    x = _r(cuda, g, M, Kd)
    w = (torch.randn(N, Kd, generator=g) * 0.05).to(BF).to(cuda)
    ld = K.round_up(N, 64)
    buf = _out(cuda, M, ld)
    K.gemm_skinny(x, [w], buf)
    rel = H.rel_l2(buf[:, :N], _ref32(x, w))
    print(f"head shape: rel-L2 {rel:.3e}")
    assert rel < TOL
    assert ld > N and bool((buf[:, N:] == SENTINEL).all())


@pytest.mark.parametrize("M", [9, 64])
def test_exact_integer_sums(cuda, M):
    """x and W integer-valued in [-2, 2], K = 2304: every partial sum is an integer below 2^24, so fp32 is exact in any
    order and the output is the bf16 rounding of the true product -- a dropped or doubled k, row or column shows."""
    g = torch.Generator().manual_seed(11 + M)
    N, Kd = 203, 2304
    x = torch.randint(-2, 3, (M, Kd), generator=g).to(BF).to(cuda)
    w = torch.randint(-2, 3, (N, Kd), generator=g).to(BF).to(cuda)
    y = _out(cuda, M, 208)
    K.gemm_skinny(x, [w], y)
    want = (x.double().cpu() @ w.double().cpu().t()).float().to(BF)
    assert torch.equal(y[:, :N].cpu(), want)


def _sub_batches(x):
    """(rows, x_sub): M = 9 on rows 20..28 (a view of the 64-row matrix) and M = 17 on a permutation."""
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(2))[:17].to(x.device)
    return [(torch.arange(20, 29, device=x.device), x[20:29]), (perm, x[perm].contiguous())]


@pytest.mark.parametrize("N,Kd", [(1000, 2304), (64, 9216)])
def test_batch_invariance_store(cuda, N, Kd):
    g = torch.Generator().manual_seed(N + Kd)
    x, w = _r(cuda, g, 64, Kd), _r(cuda, g, N, Kd, scale=0.05)
    full = _out(cuda, 64, N)
    K.gemm_skinny(x, [w], full)
    assert H.rel_l2(full, _ref32(x, w)) < TOL
    for rows, xs in _sub_batches(x):
        y = _out(cuda, xs.shape[0], N)
        K.gemm_skinny(xs, [w], y)
        assert torch.equal(y, full[rows]), xs.shape


def test_determinism(cuda):
    g = torch.Generator().manual_seed(31)
    x, w = _r(cuda, g, 33, 9216), _r(cuda, g, 203, 9216, scale=0.05)
    a, b = _out(cuda, 33, 208), _out(cuda, 33, 208)
    K.gemm_skinny(x, [w], a)
    K.gemm_skinny(x, [w], b)
    assert torch.equal(a, b)  # the kernel takes no workspace: nothing to leave zeroed


def test_refusals(cuda):
    g = torch.Generator().manual_seed(41)
    x, w = _r(cuda, g, 64, 64), _r(cuda, g, 16, 64)
    y = _out(cuda, 64, 16)

    def refused(*a, **kw):
        with pytest.raises(L.SvlaError, match="gemm_skinny"):
            K.gemm_skinny(*a, **kw)
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all())

    refused(x, [w], y, M=0)
    refused(x, [w], y, M=65)
    x40, w40 = _r(cuda, g, 9, 40), _r(cuda, g, 16, 40)
    refused(x40, [w40], y)
    flat = _r(cuda, g, 16 * 64 + 8)
    w8 = flat[4:4 + 16 * 64].view(16, 64)
    assert w8.data_ptr() % 16 == 8
    refused(x, [w8], y)
