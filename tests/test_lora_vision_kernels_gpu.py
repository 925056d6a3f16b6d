"""The GELU / RESID / SCALE epilogues of svla_lora_up (csrc/lora.hip, SLICED mode; the vision-side linears of the
"spatialvla-linear" LoRA target set): each is bitwise the two-step form -- lora_up without an epilogue, then the
elementwise op the epilogue fuses -- at ragged rows, N % 32 == 16 (the last unit has only its `a` tile; SigLIP's
I = 4304 is such an N), one and two k-steps, and a shape with many blocks.  T carries NaN in its pad columns."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHAPES = [(37, 304, 8), (37, 304, 64), (530, 1152, 32)]
ALPHA = 0.5


def _r(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).to(BF)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=BF, device="cuda")


def _case(M, N, r):
    """(c0, t, B, plain): plain = lora_up with no epilogue on a copy of c0."""
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(100 + r)
    t = _nan(M, Kn.lora_R(r))
    t[:, :r] = _r(M, r)
    B = _r(N, r, scale=0.1)
    c0 = _r(M, N)
    plain = c0.clone()
    Kn.lora_up(plain, t, [B], r, alpha=ALPHA)
    assert not torch.isnan(plain).any() and not torch.equal(plain, c0)
    return c0, t, B, plain


@pytest.mark.parametrize("M,N,r", SHAPES)
def test_lora_up_gelu(cuda, M, N, r):
    from spatialvla_amd import kernels as Kn
    c0, t, B, plain = _case(M, N, r)
    ref = torch.empty_like(plain)
    Kn.gelu_rows(Kn.GELU_TANH, plain, ref)
    hbuf = _nan(M, N + 24)  # h with a row stride above N: the columns behind it stay NaN
    c = c0.clone()
    Kn.lora_up(c, t, [B], r, alpha=ALPHA, gelu_out=hbuf[:, :N])
    torch.cuda.synchronize()
    assert torch.equal(c, plain), "C keeps the pre-activation"
    assert torch.equal(hbuf[:, :N], ref)
    assert torch.isnan(hbuf[:, N:]).all()


@pytest.mark.parametrize("M,N,r", SHAPES)
def test_lora_up_resid(cuda, M, N, r):
    from spatialvla_amd import kernels as Kn
    c0, t, B, plain = _case(M, N, r)
    res = _r(M, N + 40)[:, :N]  # row stride larger than N
    cbuf = _nan(M, N + 8)
    cbuf[:, :N] = c0
    Kn.lora_up(cbuf[:, :N], t, [B], r, alpha=ALPHA, resid=res)
    torch.cuda.synchronize()
    assert torch.equal(cbuf[:, :N], plain + res)  # the bf16 add: fp32 sum of two bf16 values, rounded once
    assert torch.isnan(cbuf[:, N:]).all()


@pytest.mark.parametrize("M,N,r", SHAPES)
def test_lora_up_scale(cuda, M, N, r):
    from spatialvla_amd import kernels as Kn
    c0, t, B, plain = _case(M, N, r)
    post = 1.0 / (2304 ** 0.5)
    c = c0.clone()
    Kn.lora_up(c, t, [B], r, alpha=ALPHA, post_scale=post)
    torch.cuda.synchronize()
    assert torch.equal(c, plain * post)  # the bf16 multiply by the fp32 scalar, as SVLA_EPI_BIAS's alpha


def test_lora_up_vision_epilogues_three_segments(cuda):
    """RESID and SCALE take any segment list (q|k|v-style slices); GELU is single-segment and says so."""
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(5)
    M, r, sizes = 50, 8, [112, 96, 96]
    N, R = sum(sizes), Kn.lora_R(r)
    t = _nan(M, 3 * R)
    for s in range(3):
        t[:, s * R:s * R + r] = _r(M, r)
    Bs = [_r(n, r, scale=0.1) for n in sizes]
    c0, res = _r(M, N), _r(M, N)
    plain = c0.clone()
    Kn.lora_up(plain, t, Bs, r, alpha=ALPHA)
    c = c0.clone()
    Kn.lora_up(c, t, Bs, r, alpha=ALPHA, resid=res)
    assert torch.equal(c, plain + res)
    c = c0.clone()
    Kn.lora_up(c, t, Bs, r, alpha=ALPHA, post_scale=0.25)
    assert torch.equal(c, plain * 0.25)
    c, h = c0.clone(), _nan(M, N)
    with pytest.raises(RuntimeError, match="one segment"):
        Kn.lora_up(c, t, Bs, r, alpha=ALPHA, gelu_out=h)
    torch.cuda.synchronize()
    assert torch.equal(c, c0) and torch.isnan(h).all()


def test_lora_up_vision_epilogue_refusals(cuda):
    """Aliased or misaligned h / res are refused before any launch: C is unchanged and h is still NaN."""
    from spatialvla_amd import kernels as Kn
    M, N, r = 37, 304, 8
    c0, t, B, _ = _case(M, N, r)
    c = c0.clone()
    h = _nan(M, N)
    pool = _nan(M * N + 64)
    odd = pool[4:4 + M * N].view(M, N)  # 8 bytes off a 16-byte boundary
    assert odd.data_ptr() % 16 == 8
    bad = [dict(gelu_out=c), dict(resid=c), dict(gelu_out=odd), dict(resid=odd)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="lora_up"):
            Kn.lora_up(c, t, [B], r, alpha=ALPHA, **kw)
    # partial overlap: h / res starting inside C's buffer
    big = torch.empty(2 * M * N, dtype=BF, device="cuda")
    cc = big[:M * N].view(M, N)
    cc.copy_(c0)
    shifted = big[8 * N:8 * N + M * N].view(M, N)
    keep = big.clone()
    for kw in (dict(gelu_out=shifted), dict(resid=shifted)):
        with pytest.raises(RuntimeError, match="overlaps"):
            Kn.lora_up(cc, t, [B], r, alpha=ALPHA, **kw)
    with pytest.raises(ValueError, match="one epilogue"):
        Kn.lora_up(c, t, [B], r, alpha=ALPHA, gelu_out=h, post_scale=0.5)
    with pytest.raises(RuntimeError, match="sliced"):
        Kn.lora_up(c, t[:, :r].contiguous(), [_r(r, N)], r, summed=True, post_scale=0.5)
    torch.cuda.synchronize()
    assert torch.equal(c, c0) and torch.isnan(h).all() and torch.isnan(odd).all()
    assert torch.equal(big[:M * N], keep[:M * N])
