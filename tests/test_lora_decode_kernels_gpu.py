"""The decode-step adapter kernels (csrc/lora_decode.hip): svla_lora_gemv_down and svla_lora_gemv against fp32 torch
restatements with the kernels' rounding points, against the training-path kernels on the same inputs, and bitwise
against the base GEMVs at B = 0.  Bound: rel-L2 < 5e-3, test_lora_kernels_gpu.py's bound for svla_lora_up /
svla_lora_down (bf16 outputs of fp32 sums: ~2^-9 relative per element).  A, B and s are scaled so the adapter term's rms
is 0.5-2x the base term's, and every segment has its own B, so a wrong slice or segment map is an O(1) error."""
import pytest
import torch

import harness as H

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TOL = 5e-3
DEV = "cuda:0"


def _rn(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(BF)


def _bf(x):
    return x.to(BF).float()


def _R(r):
    return (r + 31) // 32 * 32


def _operands(M, sizes, K, r, seed):
    """x, W_s, A_s, B_s and s with the adapter term's rms about the base term's: base ~ sqrt(K) * 0.02,
    t ~ sqrt(K) / r, adapter ~ s * sqrt(r) * t * b with b chosen per segment (segment i: 0.7 + 0.3 i of the target)."""
    torch.manual_seed(seed)
    x = _rn(M, K)
    Ws = [_rn(n, K, scale=0.02) for n in sizes]
    As = [_rn(r, K, scale=1.0 / r) for _ in sizes]
    s = 2.0
    b0 = 0.02 * r / (s * r ** 0.5)
    Bs = [_rn(n, r, scale=b0 * (0.7 + 0.3 * i)) for i, n in enumerate(sizes)]
    return x, Ws, As, Bs, s


def _t_ref(x, As, r):
    """T in svla_lora_down's SHARED layout: bf16(x A_s^T) in columns sR .. sR + r, zeros up to R."""
    R = _R(r)
    t = torch.zeros(x.shape[0], len(As) * R, device=x.device)
    for i, a in enumerate(As):
        t[:, i * R:i * R + r] = _bf(x.float() @ a.float().t())
    return t


def _y_ref(x, Ws, t, Bs, r, s):
    """bf16(bf16(x W^T) + bf16(s t_s B_s^T)) per segment, with the base and adapter terms (for the rms check)."""
    R = _R(r)
    base = torch.cat([_bf(x.float() @ w.float().t()) for w in Ws], 1)
    ad = torch.cat([_bf(s * (t[:, i * R:i * R + r].float() @ b.float().t())) for i, b in enumerate(Bs)], 1)
    return _bf(base + ad), base, ad


DOWN_SHAPES = [(2304, 3), (2048, 1), (9216, 1), (264, 2)]


@pytest.mark.parametrize("K,nseg", DOWN_SHAPES)
@pytest.mark.parametrize("r", [8, 24, 32, 64])
@pytest.mark.parametrize("M", [1, 5, 8])
def test_lora_gemv_down(cuda, M, K, nseg, r):
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(100 + r + M)
    R = _R(r)
    x = _rn(M, K)
    As = [_rn(r, K, scale=1.0 / r) for _ in range(nseg)]
    t = torch.full((M, nseg * R), float("nan"), dtype=BF, device=cuda)
    Kn.lora_gemv_down(x, As, r, t)
    ref = _t_ref(x, As, r)
    t2 = torch.full_like(t, float("nan"))
    Kn.lora_down(x, As, r, t2)
    t3 = torch.full_like(t, float("nan"))
    Kn.lora_gemv_down(x, As, r, t3)
    torch.cuda.synchronize()
    e_ref, e_train = H.rel_l2(t, ref), H.rel_l2(t, t2)
    print(f"lora_gemv_down M={M} K={K} nseg={nseg} r={r}: rel {e_ref:.2e}, vs svla_lora_down {e_train:.2e}")
    assert e_ref < TOL and e_train < TOL
    assert torch.equal(t, t3)  # two calls, the same bits
    for i in range(nseg):  # the pad columns r..R-1 of every slice are written as zero
        assert float(t[:, i * R + r:(i + 1) * R].float().abs().sum()) == 0.0
        assert bool(torch.isfinite(t.float()).all())


@pytest.mark.parametrize("K", [2304, 256])
@pytest.mark.parametrize("M", [1, 5, 8])
def test_lora_gemv_down_norm(cuda, M, K):
    """The norm-pair prologue: h_out and x are bitwise svla_add_rmsnorm2_fwd, T is the plain form's on that x."""
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(7 + M)
    r, nseg = 32, 2
    R = _R(r)
    res, y = _rn(M, K), _rn(M, K)
    w1, w2 = _rn(K, scale=0.1), _rn(K, scale=0.1)
    As = [_rn(r, K, scale=1.0 / r) for _ in range(nseg)]
    h, x = torch.empty_like(res), torch.empty_like(res)
    Kn.add_rmsnorm2_fwd(res, y, w1, w2, 1e-6, 1e-6, h, x)
    h2, x2 = torch.full_like(res, float("nan")), torch.full_like(res, float("nan"))
    t = torch.full((M, nseg * R), float("nan"), dtype=BF, device=cuda)
    Kn.lora_gemv_down(x2, As, r, t, norm=(res, y, w1, w2, 1e-6, 1e-6, h2))
    tp = torch.empty_like(t)
    Kn.lora_gemv_down(x, As, r, tp)
    torch.cuda.synchronize()
    assert torch.equal(h2, h) and torch.equal(x2, x)
    assert torch.equal(t, tp)
    assert H.rel_l2(t, _t_ref(x, As, r)) < TOL


STORE_SHAPES = [(1, [2048, 1024, 1024], 2304), (8, [2304], 2048), (3, [2304], 9216), (5, [16, 16, 16], 264)]


def _store_case(M, sizes, K, r=32, seed=5, zero_b=False):
    from spatialvla_amd import kernels as Kn
    x, Ws, As, Bs, s = _operands(M, sizes, K, r, seed)
    if zero_b:
        Bs = [torch.zeros_like(b) for b in Bs]
    t = torch.empty(M, len(sizes) * _R(r), dtype=BF, device=DEV)
    Kn.lora_gemv_down(x, As, r, t)
    out = torch.full((M, sum(sizes)), float("nan"), dtype=BF, device=DEV)
    Kn.lora_gemv(x, Ws, t, Bs, r, s, out)
    return x, Ws, As, Bs, s, t, out


@pytest.mark.parametrize("M,sizes,K", STORE_SHAPES)
def test_lora_gemv_store(cuda, M, sizes, K):
    from spatialvla_amd import kernels as Kn
    r = 32
    x, Ws, As, Bs, s, t, out = _store_case(M, sizes, K, r)
    ref, base, ad = _y_ref(x, Ws, t, Bs, r, s)
    ratio = float(ad.norm() / base.norm())
    out2 = torch.full_like(out, float("nan"))
    Kn.lora_gemv(x, Ws, t, Bs, r, s, out2)
    # the training path on the same operands: plain-store GEMM, then svla_lora_up SLICED
    comp = torch.empty_like(out)
    Kn.linear_fwd(x, Ws, comp)
    Kn.lora_up(comp, t, Bs, r, alpha=s)
    torch.cuda.synchronize()
    e, ec = H.rel_l2(out, ref), H.rel_l2(out, comp)
    print(f"lora_gemv STORE M={M} N={sizes} K={K}: rel {e:.2e}, vs gemm + lora_up {ec:.2e}, adapter/base rms {ratio:.2f}")
    assert 0.5 <= ratio <= 2.0
    assert e < TOL and ec < TOL
    assert torch.equal(out, out2)
    # other ranks through the same kernels (one lane per rank column: r = 8 and r = 64 are the edges)
    for r2 in (8, 24, 64):
        x, Ws, As, Bs, s, t, o = _store_case(M, sizes, K, r2, seed=6)
        assert H.rel_l2(o, _y_ref(x, Ws, t, Bs, r2, s)[0]) < TOL, r2


GEGLU_SHAPES = [(1, 1024, 2304), (5, 1024, 2304), (2, 48, 256)]


def _base_geglu(x, wg, wu):
    """linear_geglu_fwd on the same operands.  The library's GeGLU GEMM takes I % 64 == 0 only, so other I run with
    zero rows appended to both weights (a wave owns one row pair: the first I columns do not depend on the others)."""
    from spatialvla_amd import kernels as Kn
    M, K = x.shape
    I = wg.shape[0]
    Ip = (I + 63) // 64 * 64
    if Ip != I:
        pad = torch.zeros(Ip - I, K, dtype=BF, device=DEV)
        wg, wu = torch.cat([wg, pad]), torch.cat([wu, pad])
    h, g, u = (torch.empty(M, Ip, dtype=BF, device=DEV) for _ in range(3))
    Kn.linear_geglu_fwd(x, wg, wu, h, g, u)
    return h[:, :I], g[:, :I], u[:, :I]


@pytest.mark.parametrize("M,I,K", GEGLU_SHAPES)
def test_lora_gemv_geglu(cuda, M, I, K):
    from spatialvla_amd import kernels as Kn
    r = 32
    x, Ws, As, Bs, s = _operands(M, [I, I], K, r, seed=9)
    t = torch.empty(M, 2 * _R(r), dtype=BF, device=cuda)
    Kn.lora_gemv_down(x, As, r, t)
    h, g, u = (torch.full((M, I), float("nan"), dtype=BF, device=cuda) for _ in range(3))
    Kn.lora_gemv(x, Ws, t, Bs, r, s, h, geglu_out=(g, u))
    gu_ref, base, ad = _y_ref(x, Ws, t, Bs, r, s)
    g_ref, u_ref = gu_ref[:, :I], gu_ref[:, I:]
    h_ref = _bf(torch.nn.functional.gelu(g_ref, approximate="tanh")) * u_ref
    h2, g2, u2 = (torch.empty_like(h) for _ in range(3))
    Kn.lora_gemv(x, Ws, t, Bs, r, s, h2, geglu_out=(g2, u2))
    torch.cuda.synchronize()
    eg, eu, eh = H.rel_l2(g, g_ref), H.rel_l2(u, u_ref), H.rel_l2(h, h_ref)
    print(f"lora_gemv GEGLU M={M} I={I} K={K}: g {eg:.2e} u {eu:.2e} h {eh:.2e}")
    assert 0.5 <= float(ad.norm() / base.norm()) <= 2.0
    assert eg < TOL and eu < TOL and eh < TOL
    # h is the fused epilogue's rounding applied to the kernel's own g, u (as test_gemv_geglu checks)
    h_own = (torch.nn.functional.gelu(g.float(), approximate="tanh").to(BF).float() * u.float()).to(BF)
    assert (h.float() - h_own.float()).abs().max() <= 1e-2 * h_own.float().abs().max()
    assert torch.equal(h, h2) and torch.equal(g, g2) and torch.equal(u, u2)


@pytest.mark.parametrize("M,sizes,K", STORE_SHAPES)
def test_lora_gemv_store_zero_b_is_base_gemv(cuda, M, sizes, K):
    from spatialvla_amd import kernels as Kn
    x, Ws, As, Bs, s, t, out = _store_case(M, sizes, K, zero_b=True)
    base = torch.empty_like(out)
    Kn.linear_fwd(x, Ws, base)
    torch.cuda.synchronize()
    assert torch.equal(out, base)


@pytest.mark.parametrize("M,I,K", GEGLU_SHAPES)
def test_lora_gemv_geglu_zero_b_is_base_gemv(cuda, M, I, K):
    from spatialvla_amd import kernels as Kn
    r = 32
    x, Ws, As, Bs, s = _operands(M, [I, I], K, r, seed=9)
    Bs = [torch.zeros_like(b) for b in Bs]
    t = torch.empty(M, 2 * _R(r), dtype=BF, device=cuda)
    Kn.lora_gemv_down(x, As, r, t)
    h, g, u = (torch.empty(M, I, dtype=BF, device=cuda) for _ in range(3))
    Kn.lora_gemv(x, Ws, t, Bs, r, s, h, geglu_out=(g, u))
    hb, gb, ub = _base_geglu(x, Ws[0], Ws[1])
    torch.cuda.synchronize()
    assert torch.equal(g, gb) and torch.equal(u, ub) and torch.equal(h, hb)


@pytest.mark.parametrize("geglu", [False, True])
@pytest.mark.parametrize("M,K", [(1, 2304), (5, 2304), (2, 256)])
def test_lora_gemv_norm_zero_b_is_gemv_rmsnorm2(cuda, M, K, geglu):
    """lora_gemv_down's norm form + lora_gemv at B = 0 against svla_gemv_rmsnorm2: every output bitwise."""
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(21)
    r = 32
    sizes = [64, 64] if geglu else [128, 32, 32]
    res, y = _rn(M, K), _rn(M, K)
    w1, w2 = _rn(K, scale=0.1), _rn(K, scale=0.1)
    Ws = [_rn(n, K, scale=0.02) for n in sizes]
    As = [_rn(r, K, scale=1.0 / r) for _ in sizes]
    Bs = [torch.zeros(n, r, dtype=BF, device=cuda) for n in sizes]
    h_ref = torch.empty_like(res)
    N = sizes[0] if geglu else sum(sizes)
    o_ref = torch.empty(M, N, dtype=BF, device=cuda)
    gu_ref = tuple(torch.empty(M, N, dtype=BF, device=cuda) for _ in range(2)) if geglu else None
    Kn.gemv_rmsnorm2(res, y, w1, w2, 1e-6, 1e-6, h_ref, Ws, o_ref, geglu_out=gu_ref)
    h, x = torch.empty_like(res), torch.empty_like(res)
    t = torch.empty(M, len(sizes) * _R(r), dtype=BF, device=cuda)
    Kn.lora_gemv_down(x, As, r, t, norm=(res, y, w1, w2, 1e-6, 1e-6, h))
    o = torch.empty_like(o_ref)
    gu = tuple(torch.empty_like(o_ref) for _ in range(2)) if geglu else None
    Kn.lora_gemv(x, Ws, t, Bs, r, 2.0, o, geglu_out=gu)
    torch.cuda.synchronize()
    assert torch.equal(h, h_ref) and torch.equal(o, o_ref)
    if geglu:
        assert torch.equal(gu[0], gu_ref[0]) and torch.equal(gu[1], gu_ref[1])


def test_lora_gemv_bad_arguments(cuda):
    """Bad arguments come back as errors from the library (svla_last_error set) and the outputs stay untouched."""
    from spatialvla_amd import kernels as Kn, _lib as L_
    torch.manual_seed(2)
    K, N, r = 256, 64, 16
    sent = 1.5

    def down(M=2, r=r, x=None, a=None):
        x = _rn(M, K) if x is None else x
        a = _rn(r, K) if a is None else a
        t = torch.full((x.shape[0], _R(r)), sent, dtype=BF, device=cuda)
        with pytest.raises(L_.SvlaError) as ei:
            Kn.lora_gemv_down(x, [a], r, t)
        torch.cuda.synchronize()
        assert bool((t == sent).all()) and "lora_gemv_down" in str(ei.value)

    down(r=12)                                      # r not a multiple of 8
    down(r=72)                                      # r above 64
    down(M=9)                                       # more than 8 rows
    flat = _rn(2 * K + 8)
    down(x=flat[4:4 + 2 * K].view(2, K))            # x 8 bytes off a 16-B boundary
    down(a=_rn(r * K + 8)[4:4 + r * K].view(r, K))  # A misaligned

    def up(M=2, r=r, sizes=(32, 32), x=None):
        x = _rn(M, K) if x is None else x
        Ws = [_rn(n, K) for n in sizes]
        Bs = [_rn(n, r) for n in sizes]
        t = _rn(x.shape[0], len(sizes) * _R(r))
        out = torch.full((x.shape[0], sum(sizes)), sent, dtype=BF, device=cuda)
        with pytest.raises(L_.SvlaError) as ei:
            Kn.lora_gemv(x, Ws, t, Bs, r, 1.0, out)
        torch.cuda.synchronize()
        assert bool((out == sent).all()) and "lora_gemv" in str(ei.value)

    up(r=12)
    up(M=9)
    up(sizes=(24, 40))                              # a segment start that is no multiple of 16
    up(x=flat[4:4 + 2 * K].view(2, K))
    # the norm prologue holds rows of at most 2560 features
    M, Kb = 1, 4096
    res, y, h, x = (_rn(M, Kb) for _ in range(4))
    w = _rn(Kb)
    t = torch.full((M, 32), sent, dtype=BF, device=cuda)
    x0 = x.clone()
    with pytest.raises(L_.SvlaError):
        Kn.lora_gemv_down(x, [_rn(16, Kb)], 16, t, norm=(res, y, w, w, 1e-6, 1e-6, h))
    torch.cuda.synchronize()
    assert bool((t == sent).all()) and torch.equal(x, x0)
