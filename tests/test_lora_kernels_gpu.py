"""svla_lora_down / svla_lora_up / svla_lora_wgrad (csrc/lora.hip) against torch fp32 references of the same products
with the bf16 rounding points of include/svla.h.  Bounds: rel-L2 < 5e-3 for products, 1e-2 through GELU (the
per-kernel bounds of test_kernels_gpu.py)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from harness import rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _r(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).to(BF)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=BF, device="cuda")


def _bf(x):
    return x.to(BF).float()


def _split(n, parts):
    """Column starts of `parts` segments of n columns, multiples of 16, not all equal."""
    if parts == 1:
        return [n]
    base = (n // parts) // 16 * 16
    sizes = [base + 16] + [base] * (parts - 2)
    return sizes + [n - sum(sizes)]


# ------------------------------------------------------------------------------------------ lora_down
@pytest.mark.parametrize("M,K,r", [(200, 320, 8), (1000, 2304, 32), (130, 9216, 64)])
@pytest.mark.parametrize("nseg", [1, 3])
def test_lora_down_shared(cuda, M, K, r, nseg):
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(1)
    R = Kn.lora_R(r)
    x = _r(M, K)
    mats = [_r(r, K, scale=0.05) for _ in range(nseg)]
    t = _nan(M, nseg * R)
    Kn.lora_down(x, mats, r, t, alpha=0.75)
    torch.cuda.synchronize()
    for s, a in enumerate(mats):
        ref = 0.75 * (x.float() @ a.float().T)
        assert rel_l2(t[:, s * R:s * R + r], ref) < 5e-3, s
        assert (t[:, s * R + r:(s + 1) * R] == 0).all(), "pad columns r..R-1 must be written as zero"


@pytest.mark.parametrize("M,K,r", [(200, 320, 8), (1000, 2304, 32), (130, 9216, 64)])
def test_lora_down_sliced(cuda, M, K, r):
    """Two segments whose boundary is no multiple of 256 (320 = 192 | 128)."""
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(2)
    R = Kn.lora_R(r)
    n0 = 192 if K == 320 else (K // 2 + 72)
    sizes = [n0, K - n0]
    x = _r(M, K)
    mats = [_r(n, r, scale=0.05) for n in sizes]
    t = _nan(M, 2 * R)
    Kn.lora_down(x, mats, r, t, sliced=True, alpha=2.0)
    torch.cuda.synchronize()
    off = 0
    for s, b in enumerate(mats):
        ref = 2.0 * (x[:, off:off + sizes[s]].float() @ b.float())
        assert rel_l2(t[:, s * R:s * R + r], ref) < 5e-3, s
        assert (t[:, s * R + r:(s + 1) * R] == 0).all()
        off += sizes[s]


# ------------------------------------------------------------------------------------------ lora_up
def _t_slices(M, r, nseg, Kn):
    """T [M, nseg R] with NaN in the pad columns: the kernel may not read them."""
    R = Kn.lora_R(r)
    t = _nan(M, nseg * R)
    for s in range(nseg):
        t[:, s * R:s * R + r] = _r(M, r)
    return t


def _up_ref_sliced(c, t, mats, r, R, alpha):
    out, off = [], 0
    for s, b in enumerate(mats):
        u = _bf(alpha * (t[:, s * R:s * R + r].float() @ b.float().T))
        out.append(_bf(c[:, off:off + b.shape[0]].float() + u))
        off += b.shape[0]
    return torch.cat(out, 1)


@pytest.mark.parametrize("r", [8, 32, 64])
def test_lora_up_none(cuda, r):
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(3)
    M, N = 200, 320
    R = Kn.lora_R(r)
    # sliced, 3 segments
    sizes = _split(N, 3)
    mats = [_r(n, r, scale=0.1) for n in sizes]
    t = _t_slices(M, r, 3, Kn)
    c0 = _r(M, N)
    c = c0.clone()
    Kn.lora_up(c, t, mats, r, alpha=0.5)
    torch.cuda.synchronize()
    assert rel_l2(c, _up_ref_sliced(c0, t, mats, r, R, 0.5)) < 5e-3
    # summed, 2 segments
    mats = [_r(r, N, scale=0.1) for _ in range(2)]
    t = _t_slices(M, r, 2, Kn)
    c = c0.clone()
    Kn.lora_up(c, t, mats, r, summed=True, alpha=0.5)
    torch.cuda.synchronize()
    u = sum(t[:, s * R:s * R + r].float() @ a.float() for s, a in enumerate(mats))
    assert rel_l2(c, _bf(c0.float() + _bf(0.5 * u))) < 5e-3
    # zero T leaves C bitwise unchanged
    c = c0.clone()
    Kn.lora_up(c, torch.zeros(M, 2 * R, dtype=BF, device=cuda), mats, r, summed=True, alpha=0.5)
    torch.cuda.synchronize()
    assert torch.equal(c, c0)


def test_lora_up_merge_form(cuda):
    """The merge W += s B A: T = B with ldt = r = 8 < R; everything behind T is NaN, so an over-read shows."""
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(4)
    n_out, n_in, r = 200, 320, 8
    buf = _nan(n_out * r + 4096)
    b = buf[:n_out * r].view(n_out, r)
    b.copy_(_r(n_out, r, scale=0.1))
    a = _r(r, n_in, scale=0.1)
    w0 = _r(n_out, n_in, scale=0.02)
    w = w0.clone()
    Kn.lora_up(w, b, [a], r, summed=True, alpha=2.0)
    torch.cuda.synchronize()
    assert torch.isfinite(w.float()).all()
    assert rel_l2(w, _bf(w0.float() + _bf(2.0 * (b.float() @ a.float())))) < 5e-3


def _rope_tables(L, D):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, device="cuda").float() / D))
    fr = (torch.arange(L, device="cuda").float() + 1)[:, None] * inv[None]
    return fr.cos().to(BF).contiguous(), fr.sin().to(BF).contiguous()


def _rope_ref(c, L, D, cols, cos, sin):
    """bf16(bf16(x cos) + bf16(rotate_half(x) sin)) on the heads of the first `cols` columns; row m at m % L."""
    M = c.shape[0]
    pos = torch.arange(M, device=c.device) % L
    cs, sn = cos.float()[pos][:, None, :], sin.float()[pos][:, None, :]
    x = c[:, :cols].float().view(M, cols // D, D)
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    lo = _bf(_bf(x1 * cs) + _bf(-x2 * sn))
    hi = _bf(_bf(x2 * cs) + _bf(x1 * sn))
    out = c.float().clone()
    out[:, :cols] = torch.cat([lo, hi], -1).view(M, cols)
    return out


def test_lora_up_rope(cuda):
    """ROPE: zero T on a plain q|k|v product is bitwise svla_qkv_rope_fill's in-place rotation; non-zero T follows
    the torch chain (update rounded to bf16, then the rotation's roundings)."""
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(5)
    B, L, Hq, Hkv, D, H, r = 2, 100, 2, 1, 256, 256, 8
    M, qd, kd = B * L, Hq * D, Hkv * D
    N = qd + 2 * kd
    R = Kn.lora_R(r)
    x = _r(M, H)
    ws = [_r(qd, H, scale=0.06), _r(kd, H, scale=0.06), _r(kd, H, scale=0.06)]
    cos, sin = _rope_tables(L, D)
    qkv = torch.empty(M, N, dtype=BF, device=cuda)
    Kn.linear_fwd(x, ws, qkv)
    mats = [_r(qd, r, scale=0.1), _r(kd, r, scale=0.1), _r(kd, r, scale=0.1)]
    rope = (cos, sin, L, D, qd + kd)
    # zero T
    a = qkv.clone()
    kc, vc = (torch.empty(B, L, kd, dtype=BF, device=cuda) for _ in range(2))
    Kn.qkv_rope_append(a, B, L, Hq, Hkv, D, cos.repeat(B, 1), sin.repeat(B, 1), kc, vc, 0, k_back=True)
    b = qkv.clone()
    Kn.lora_up(b, torch.zeros(M, 3 * R, dtype=BF, device=cuda), mats, r, alpha=1.0, rope=rope)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(b[:, qd + kd:], qkv[:, qd + kd:])
    # non-zero T
    t = _t_slices(M, r, 3, Kn)
    c = qkv.clone()
    Kn.lora_up(c, t, mats, r, alpha=0.5, rope=rope)
    torch.cuda.synchronize()
    ref = _rope_ref(_up_ref_sliced(qkv, t, mats, r, R, 0.5).to(BF), L, D, qd + kd, cos, sin)
    assert rel_l2(c, ref) < 5e-3


def test_lora_up_geglu(cuda):
    """GEGLU: zero T on a plain gate|up product gives bitwise the h, g, u of an SVLA_EPI_GEGLU call (both GEMMs on the
    same kernel variant, so the accumulators agree); non-zero T follows the torch chain."""
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(6)
    M, H, I, r = 200, 256, 384, 8
    R = Kn.lora_R(r)
    x = _r(M, H)
    wg, wu = _r(I, H, scale=0.06), _r(I, H, scale=0.06)
    h0, g0, u0 = (torch.empty(M, I, dtype=BF, device=cuda) for _ in range(3))
    gu = torch.empty(M, 2 * I, dtype=BF, device=cuda)
    try:
        Kn.gemm_variant = 2
        Kn.linear_geglu_fwd(x, wg, wu, h0, g0, u0)
        Kn.linear_fwd(x, [wg, wu], gu)
    finally:
        Kn.gemm_variant = 0
    mats = [_r(I, r, scale=0.1), _r(I, r, scale=0.1)]
    c = gu.clone()
    h = _nan(M, I)
    Kn.lora_up(c, torch.zeros(M, 2 * R, dtype=BF, device=cuda), mats, r, alpha=1.0, geglu_h=h)
    torch.cuda.synchronize()
    assert torch.equal(c[:, :I], g0) and torch.equal(c[:, I:], u0) and torch.equal(h, h0)
    t = _t_slices(M, r, 2, Kn)
    c = gu.clone()
    h = _nan(M, I)
    Kn.lora_up(c, t, mats, r, alpha=0.5, geglu_h=h)
    torch.cuda.synchronize()
    ref = _up_ref_sliced(gu, t, mats, r, R, 0.5)
    assert rel_l2(c, ref) < 5e-3
    g, u = c[:, :I].float(), c[:, I:].float()  # the kernel's own g | u: h is checked as a function of them
    assert rel_l2(h, _bf(F.gelu(g, approximate="tanh")) * u) < 1e-2


# ------------------------------------------------------------------------------------------ lora_wgrad
_WG = {}


def _wgrad_inputs(M, W, r):
    """Inputs and fp32 references of one (M, W, r) case, computed once and left unchanged."""
    key = (M, W, r)
    if key not in _WG:
        from spatialvla_amd import kernels as Kn
        torch.manual_seed(7)
        R = Kn.lora_R(r)
        y = _r(M, W)
        t = torch.zeros(M, 2 * R, dtype=BF, device="cuda")
        for s in range(2):
            t[:, s * R:s * R + r] = _r(M, r)
        sizes = _split(W, 2)
        ts = [t[:, s * R:s * R + r].float() for s in range(2)]
        ref_a = [0.5 * (ts[s].T @ y.float()) for s in range(2)]
        ref_b = [0.5 * (y[:, o:o + n].float().T @ ts[s]) for s, (o, n) in enumerate(zip([0, sizes[0]], sizes))]
        _WG[key] = (y, t, sizes, ref_a, ref_b)
    return _WG[key]


@pytest.mark.parametrize("M,W,r", [(200, 320, 8), (9984, 2304, 32), (1000, 1024, 64)])
@pytest.mark.parametrize("sliced", [False, True])
def test_lora_wgrad(cuda, M, W, r, sliced):
    from spatialvla_amd import kernels as Kn
    y, t, sizes, ref_a, ref_b = _wgrad_inputs(M, W, r)
    refs = ref_b if sliced else ref_a
    shapes = [(n, r) for n in sizes] if sliced else [(r, W)] * 2

    def run(acc_init=None):
        outs = [_nan(*s) if acc_init is None else acc_init[i].clone() for i, s in enumerate(shapes)]
        Kn.lora_wgrad(y, t, outs, r, sliced=sliced, alpha=0.5, accumulate=acc_init is not None)
        return outs

    o1 = run()
    o2 = run()  # same workspace: nothing is left behind by the first call
    torch.cuda.synchronize()
    for a, b, ref in zip(o1, o2, refs):
        assert rel_l2(a, ref) < 5e-3
        assert torch.equal(a, b)
    init = [_r(*s, scale=float(refs[0].std())) for s in shapes]
    o3 = run(init)
    torch.cuda.synchronize()
    for a, i0, ref in zip(o3, init, refs):
        assert rel_l2(a, i0.float() + ref) < 5e-3
    # beside a stream-K GEMM on a second stream (its own workspace): still the same bits
    s2 = torch.cuda.Stream()
    ga, gb = _r(2048, 2048), _r(2048, 2048)
    gc = torch.empty(2048, 2048, dtype=BF, device=cuda)
    torch.cuda.synchronize()
    try:
        Kn.gemm_variant = 4  # 8-phase + stream-K: the GEMM beside it really uses its workspace and counters
        with torch.cuda.stream(s2):
            for _ in range(3):
                Kn.linear_fwd(ga, [gb], gc)
    finally:
        Kn.gemm_variant = 0
    o4 = run()
    torch.cuda.synchronize()
    for a, b in zip(o1, o4):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ arguments
def test_lora_rejected_arguments(cuda):
    """A bad rank, a misaligned ld and more than 3 segments return SVLA_ERR_ARG with a message; nothing is launched
    (the NaN-filled output stays NaN)."""
    from spatialvla_amd import _lib as L
    lib = L.lib()
    M, K = 64, 128
    x = _r(M, K + 8)
    a = _r(32, K)
    t = _nan(M, 32)
    st = torch.cuda.current_stream().cuda_stream

    def segs(nseg, r, ld):
        s = L.LoraSegs()
        for i in range(min(nseg, 3)):
            s.ptr[i] = a.data_ptr()
        s.nseg, s.r, s.ld = nseg, r, ld
        return s

    def call(s, ldx):
        return lib.svla_lora_down(M, K, x.data_ptr(), ldx, ctypes.byref(s), L.LORA_SHARED, 1.0, t.data_ptr(), 32, st)

    assert call(segs(1, 32, K), K + 8) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(t.float()).all()
    t.fill_(float("nan"))
    for s, ldx, word in ((segs(1, 12, K), K + 8, b"rank"), (segs(1, 72, K), K + 8, b"rank"),
                         (segs(1, 32, K), K + 4, b"ldx"), (segs(4, 32, K), K + 8, b"segments")):
        assert call(s, ldx) == 1  # SVLA_ERR_ARG
        assert word in lib.svla_last_error()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=cuda)
    o = segs(4, 32, K)
    assert lib.svla_lora_wgrad(M, K, x.data_ptr(), K + 8, t.data_ptr(), 32, L.LORA_SHARED, ctypes.byref(o), 1.0, 0,
                               ws.data_ptr(), ws.numel(), st) == 1
    c = _r(M, K)
    assert lib.svla_lora_up(M, K, c.data_ptr(), K + 4, t.data_ptr(), 32, ctypes.byref(segs(1, 32, K)), L.LORA_SUMMED,
                            1.0, None, st) == 1
    torch.cuda.synchronize()
    assert torch.isnan(t.float()).all()
