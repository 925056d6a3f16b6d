"""svla_lora_up in GEGLU mode with the OCP MX e4m3 copy of h from the same pass (svla_lora_epilogue.mx_q): g | u and h
bitwise the call without the copy, the copy bitwise svla_quant_mx_rows of the stored h (a non-finite value makes its
block NaN, a zero block gets scale byte 0), run to run identical, and widths the layout cannot hold refused."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn


def _case(M, I, r, dev):
    """g | u [M, 2I] in a wider buffer (ldc > 2I), T, B_gate | B_up.  u's 32-column blocks have magnitudes 2^-10 ..
    2^10, block 1 of u is zero and its rows of B_up too (so u, and h, stay zero there), one u element is +Inf."""
    from spatialvla_amd import kernels as Kn
    gen = torch.Generator(device="cpu").manual_seed(100 * M + I + r)
    R = Kn.lora_R(r)
    nb = I // 32
    mag = torch.tensor([2.0 ** (-10 + 20 * b / max(nb - 1, 1)) for b in range(nb)]).repeat_interleave(32)
    g = torch.randn(M, I, generator=gen)
    u = torch.randn(M, I, generator=gen) * mag
    u[:, 32:64] = 0.0
    u[M // 2, 70] = float("inf")
    buf = torch.zeros(M, 2 * I + 16, dtype=BF)
    buf[:, :I], buf[:, I:2 * I] = g.to(BF), u.to(BF)
    t = torch.zeros(M, 2 * R, dtype=BF)
    t[:, :r] = torch.randn(M, r, generator=gen).to(BF)
    t[:, R:R + r] = torch.randn(M, r, generator=gen).to(BF)
    Bg = (torch.randn(I, r, generator=gen) * 0.1).to(BF)
    Bu = (torch.randn(I, r, generator=gen) * 0.1 * mag[:, None]).to(BF)
    Bu[32:64] = 0
    return buf.to(dev), t.to(dev), [Bg.to(dev), Bu.to(dev)]


def _run(buf, t, mats, r, I, mx):
    from spatialvla_amd import kernels as Kn
    M = buf.shape[0]
    dev = buf.device
    c = buf.clone()
    hbuf = torch.full((M, I + 8), float("nan"), dtype=BF, device=dev)  # ldh > I
    out = None
    if mx:
        qbuf = torch.zeros(M, I + 16, dtype=torch.uint8, device=dev).view(FP8)  # mx_ldq > I
        sc = Kn.MXScales(M, I, dev)
        sc.buf.fill_(0x5a)
        out = (qbuf[:, :I], sc)
    Kn.lora_up(c[:, :2 * I], t, mats, r, alpha=0.5, geglu_h=hbuf[:, :I], mx_out=out)
    torch.cuda.synchronize()
    return c, hbuf, out


@pytest.mark.parametrize("r", [8, 32])
@pytest.mark.parametrize("I", [128, 384])
@pytest.mark.parametrize("M", [1, 33, 130])
def test_lora_up_geglu_mx_bitwise(cuda, M, I, r):
    from spatialvla_amd import kernels as Kn
    buf, t, mats = _case(M, I, r, cuda)
    c0, h0, _ = _run(buf, t, mats, r, I, False)
    c1, h1, (q1, s1) = _run(buf, t, mats, r, I, True)
    # g | u (and the pad columns beyond them) and h: the bits of the call without the copy; NaN == NaN bytewise
    assert torch.equal(c0.view(torch.int16), c1.view(torch.int16))
    assert torch.equal(h0.view(torch.int16), h1.view(torch.int16))
    assert not torch.equal(c1[:, :2 * I].view(torch.int16), buf[:, :2 * I].view(torch.int16))  # the adapters were added
    h = h1[:, :I]
    assert float(h[:, 32:64].float().abs().max()) == 0.0 and not bool(torch.isfinite(h[M // 2, 64:96].float()).all())
    qr, sr = Kn.quant_mx_rows(h)
    torch.cuda.synchronize()
    assert torch.equal(q1.view(torch.uint8), qr.view(torch.uint8))
    assert torch.equal(s1.exponents(), sr.exponents())
    # what the data was built to reach: the zero block's scale byte is 0, the +Inf block is a NaN block
    assert int(s1.exponents()[0, 1]) == -127 and int(s1.exponents()[M // 2, 2]) == 128
    assert bool((q1.view(torch.uint8)[M // 2, 64:96] == 0x7f).all())
    c2, h2, (q2, s2) = _run(buf, t, mats, r, I, True)
    assert torch.equal(c1.view(torch.int16), c2.view(torch.int16)) and torch.equal(h1.view(torch.int16), h2.view(torch.int16))
    assert torch.equal(q1.view(torch.uint8), q2.view(torch.uint8)) and torch.equal(s1.buf, s2.buf)


def test_lora_up_geglu_mx_refuses_other_widths(cuda):
    """I = 192 is no multiple of the 128-column scale tile: an error code, nothing launched (outputs untouched); the
    same call without the copy runs.  A ROPE / plain call with mx_q set is refused too."""
    from spatialvla_amd import _lib, kernels as Kn
    M, I, r = 33, 192, 8
    buf, t, mats = _case(M, I, r, cuda)
    before = buf.clone()
    with pytest.raises(_lib.SvlaError, match="lora_up"):
        _run(buf, t, mats, r, I, True)
    c = buf.clone()
    h = torch.full((M, I), float("nan"), dtype=BF, device=cuda)
    q = torch.zeros(M, I, dtype=torch.uint8, device=cuda).view(FP8)
    with pytest.raises(_lib.SvlaError, match="lora_up"):
        Kn.lora_up(c[:, :2 * I], t, mats, r, alpha=0.5, geglu_h=h, mx_out=(q, Kn.MXScales(M, I, cuda)))
    torch.cuda.synchronize()
    assert torch.equal(c.view(torch.int16), before.view(torch.int16)) and bool(torch.isnan(h.float()).all())
    assert int(q.view(torch.uint8).max()) == 0
    _run(buf, t, mats, r, I, False)
    I = 128
    buf, t, mats = _case(M, I, r, cuda)
    q = torch.zeros(M, I, dtype=torch.uint8, device=cuda).view(FP8)
    with pytest.raises(_lib.SvlaError, match="GEGLU output"):
        Kn.lora_up(buf[:, :2 * I].clone(), t, mats, r, mx_out=(q, Kn.MXScales(M, I, cuda)))


def test_lora_up_geglu_mx_refuses_aliased_outputs(cuda):
    """The copy or its scales sharing bytes with g | u or h (the kernel's pointers are restrict-qualified): an error
    code, nothing launched."""
    from spatialvla_amd import _lib, kernels as Kn
    M, I, r = 33, 128, 8
    buf, t, mats = _case(M, I, r, cuda)
    c = buf[:, :2 * I].clone()
    before = c.clone()
    h = torch.full((M, I), float("nan"), dtype=BF, device=cuda)
    sc = Kn.MXScales(M, I, cuda)
    q_in_h = h.view(torch.uint8)[:, :I].view(FP8)   # the first half of every row of h
    q_in_c = c.view(torch.uint8)[:, :I].view(FP8)
    sc_in_h = Kn.MXScales(M, I, cuda, buf=h.view(torch.uint8).reshape(-1)[:sc.buf.numel()])
    q = torch.zeros(M, I, dtype=torch.uint8, device=cuda).view(FP8)
    for out in ((q_in_h, sc), (q_in_c, sc), (q, sc_in_h)):
        with pytest.raises(_lib.SvlaError, match="overlap"):
            Kn.lora_up(c, t, mats, r, alpha=0.5, geglu_h=h, mx_out=out)
    torch.cuda.synchronize()
    assert torch.equal(c.view(torch.int16), before.view(torch.int16)) and bool(torch.isnan(h.float()).all())
