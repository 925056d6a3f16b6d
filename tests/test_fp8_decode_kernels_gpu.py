"""The weight-only MX fp8 decode kernels (csrc/fp8_decode.hip): svla_mx_scales_rowmajor, svla_gemv_mxfp8 and
svla_head_gemv_mxfp8.

The reference is never the kernel: it is W' = the exact bf16 dequantisation of K.quant_mx_rows(W) (e4m3 x 2^X is exactly
representable in bf16 for the exponents used), multiplied in float64 on the CPU.  The product bound per element is
    |y - y64| <= 2^-8 |y64| + K 2^-23 sum_k |x_k w'_k|
-- one bf16 rounding plus the worst-case fp32 accumulation error of K terms (derived, not measured) -- and every case
first shows that the existing bf16 GEMV on W' meets the same bound, so the bound is not what fails."""
import pytest
import torch

import harness as H
from spatialvla_amd import _lib as L
from spatialvla_amd import kernels as K

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CAP = 30.0


def _dequant_mx(q, sc):
    X = sc.exponents()
    rows, k = q.shape
    return (q.float().view(rows, k // 32, 32) * torch.exp2(X.float())[..., None]).view(rows, k)


def _w_data(n, k, g, scale=1.0):
    """Rows whose 32-k blocks span 2^-20 .. 2^10 in magnitude (the exponents differ within a row), one all-zero block
    and one all-zero row.  Generated on the CPU so the data do not depend on the device's generator."""
    w = torch.randn(n, k, generator=g)
    mag = torch.exp2(torch.randint(-20, 11, (n, k // 32), generator=g).float())
    w = (w.view(n, k // 32, 32) * mag[..., None]).view(n, k) * scale
    w[min(2, n - 1), :32] = 0
    w[0, :] = 0
    return w.to(BF)


def _quant(w):
    """(q, MXScales, row-major exponents, W' bf16) of a bf16 device matrix; W' is checked to be exact in bf16."""
    q, sc = K.quant_mx_rows(w)
    s = K.mx_scales_rowmajor(sc)
    wd = _dequant_mx(q, sc)
    wb = wd.to(BF)
    assert torch.equal(wb.float(), wd), "the dequantised weights must be exact in bf16"
    return q, sc, s, wb


def _bound(y, x, wb):
    """(error, tolerance) of y [M, N] against the float64 product of x [M, K] and W' [N, K], on the CPU."""
    x64, w64 = x.double().cpu(), wb.double().cpu()
    y64 = x64 @ w64.T
    tol = 2.0 ** -8 * y64.abs() + x.shape[1] * 2.0 ** -23 * (x64.abs() @ w64.abs().T)
    return (y.double().cpu() - y64).abs(), tol, y64


def _assert_bound(y, x, wb, what):
    err, tol, _ = _bound(y, x, wb)
    bad = err > tol
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert not bool(bad.any()), (what, int(bad.sum()), worst)


def _out(M, N, dev):
    return torch.full((M, K.round_up(N, 8)), 7.0, dtype=BF, device=dev)[:, :N]


def _bf16_gemv(x, wb):
    out = _out(x.shape[0], wb.shape[0], x.device)
    K.linear_fwd(x, [wb], out)
    return out


@pytest.mark.parametrize("n,k", [(24, 128), (130, 256), (1000, 2304), (520, 9216)])
def test_scales_rowmajor_bitwise(cuda, n, k):
    g = torch.Generator().manual_seed(n + k)
    q, sc, s, _ = _quant(_w_data(n, k, g).to(cuda))
    assert s.dtype == torch.uint8 and tuple(s.shape) == (n, k // 32)
    assert torch.equal(s.to(torch.int32) - 127, sc.exponents())
    assert int(s.min()) == 0 and int(s.max()) > 100  # the zero blocks (X = -127) and the 2^10 blocks


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("n,k", [(24, 128), (130, 256), (1000, 2304), (520, 9216)])  # the last: the split-K form
def test_gemv_store(cuda, M, n, k):
    g = torch.Generator().manual_seed(1000 * M + n + k)
    w = _w_data(n, k, g).to(cuda)
    x = torch.randn(M, k, generator=g).to(BF).to(cuda)
    q, sc, s, wb = _quant(w)
    assert len(torch.unique(sc.exponents()[1])) > 1  # exponents differ within a row
    _assert_bound(_bf16_gemv(x, wb), x, wb, "bf16 GEMV on W'")
    y = _out(M, n, cuda)
    K.gemv_mxfp8(x, [q], [s], y)
    _assert_bound(y, x, wb, "svla_gemv_mxfp8")
    assert bool((y[:, 0] == 0).all())  # an all-zero row: every block contributes exactly 0
    y2 = _out(M, n, cuda)
    K.gemv_mxfp8(x, [q], [s], y2)
    assert torch.equal(y, y2)  # bitwise stable run to run


def test_gemv_three_segments(cuda):
    g = torch.Generator().manual_seed(11)
    k, sizes, M = 256, (256, 128, 128), 3
    ws = [_w_data(n, k, g).to(cuda) for n in sizes]
    x = torch.randn(M, k, generator=g).to(BF).to(cuda)
    qs, ss, wbs = [], [], []
    for w in ws:
        q, _, s, wb = _quant(w)
        qs.append(q), ss.append(s), wbs.append(wb)
    wb = torch.cat(wbs, 0)
    _assert_bound(_bf16_gemv(x, wb), x, wb, "bf16 GEMV on W'")
    y = _out(M, sum(sizes), cuda)
    K.gemv_mxfp8(x, qs, ss, y)
    _assert_bound(y, x, wb, "three segments")
    # the segments of one quantised matrix give the bits of the whole matrix
    q, _, s, _ = _quant(torch.cat(ws, 0))
    y1 = _out(M, sum(sizes), cuda)
    K.gemv_mxfp8(x, [q], [s], y1)
    assert torch.equal(y, y1)


def test_nan_block(cuda):
    g = torch.Generator().manual_seed(5)
    n, k, M = 24, 256, 3
    w = _w_data(n, k, g)
    w[5, 32:64] = float("nan")
    w = w.to(cuda)
    x = torch.randn(M, k, generator=g).to(BF).to(cuda)
    q, sc = K.quant_mx_rows(w)
    s = K.mx_scales_rowmajor(sc)
    assert int(s[5, 1]) == 0xFF
    y = _out(M, n, cuda)
    K.gemv_mxfp8(x, [q], [s], y)
    assert bool(y[:, 5].isnan().all())
    keep = [i for i in range(n) if i != 5]
    assert bool(torch.isfinite(y[:, keep].float()).all())


def _geglu_formula(g, u):
    """SVLA_EPI_GEGLU's element formula on stored bf16 g, u: bf16(bf16(gelu_tanh(g)) u), gelu from the library's table."""
    M, n = g.shape
    gp = torch.zeros(M, K.round_up(n, 8), dtype=BF, device=g.device)  # svla_gelu_rows takes widths that are multiples of 8
    gp[:, :n] = g
    hg = torch.empty_like(gp)
    K.gelu_rows(0, gp, hg)
    return (hg[:, :n].float() * u.float()).to(BF)


@pytest.mark.parametrize("M", [1, 3, 8])
def test_gemv_geglu(cuda, M):
    g_ = torch.Generator().manual_seed(20 + M)
    k, I = 256, 192
    wg, wu = _w_data(I, k, g_, 0.05).to(cuda), _w_data(I, k, g_, 0.05).to(cuda)
    x = torch.randn(M, k, generator=g_).to(BF).to(cuda)
    q, _, s, wb = _quant(torch.cat([wg, wu], 0))
    _assert_bound(_bf16_gemv(x, wb), x, wb, "bf16 GEMV on W'")
    c, g, u = (_out(M, I, cuda) for _ in range(3))
    K.gemv_mxfp8(x, [q[:I], q[I:]], [s[:I], s[I:]], c, geglu_out=(g, u))
    _assert_bound(g, x, wb[:I], "g")
    _assert_bound(u, x, wb[I:], "u")
    assert torch.equal(c, _geglu_formula(g, u))
    # c against the formula applied to the reference's g, u (bf16 of the float64 products)
    _, _, g64 = _bound(g, x, wb[:I])
    _, _, u64 = _bound(u, x, wb[I:])
    c_ref = _geglu_formula(g64.to(BF).to(cuda), u64.to(BF).to(cuda)).float().cpu()
    assert H.rel_l2(c, c_ref) < 2.0 ** -6  # a few bf16 roundings of g and u carried through gelu(g) u


@pytest.mark.parametrize("geglu", [False, True])
@pytest.mark.parametrize("M,n,k", [(3, 130, 256), (1, 1000, 2304), (8, 384, 2304)])
def test_norm_prologue(cuda, M, n, k, geglu):
    g_ = torch.Generator().manual_seed(M + n + k)
    if geglu:
        n -= n % 2
    w = _w_data(n, k, g_, 0.05).to(cuda)
    res, yin = (torch.randn(M, k, generator=g_).to(BF).to(cuda) for _ in range(2))
    w1, w2 = ((0.1 * torch.randn(k, generator=g_)).to(BF).to(cuda) for _ in range(2))
    e1, e2 = 1e-6, 1e-5
    h_ref, x_ref = torch.empty_like(res), torch.empty_like(res)
    K.add_rmsnorm2_fwd(res, yin, w1, w2, e1, e2, h_ref, x_ref)
    q, _, s, wb = _quant(w)
    _assert_bound(_bf16_gemv(x_ref, wb), x_ref, wb, "bf16 GEMV on W'")
    h = torch.zeros_like(res)
    if geglu:
        I = n // 2
        c, g, u = (_out(M, I, cuda) for _ in range(3))
        K.gemv_mxfp8(None, [q[:I], q[I:]], [s[:I], s[I:]], c, geglu_out=(g, u), norm=(res, yin, w1, w2, e1, e2, h))
        _assert_bound(g, x_ref, wb[:I], "g")
        _assert_bound(u, x_ref, wb[I:], "u")
        assert torch.equal(c, _geglu_formula(g, u))
    else:
        y = _out(M, n, cuda)
        K.gemv_mxfp8(None, [q], [s], y, norm=(res, yin, w1, w2, e1, e2, h))
        _assert_bound(y, x_ref, wb, "product")
        # the same bits as the plain kernel on the stored x of svla_add_rmsnorm2_fwd (same chunk map for the same K)
        y0 = _out(M, n, cuda)
        K.gemv_mxfp8(x_ref, [q], [s], y0)
        assert torch.equal(y, y0)
    assert torch.equal(h, h_ref)


HEAD_CASES = [(8, 1000, 256, 23), (8, 2050, 2304, 14), (1, 2050, 2304, 33)]  # seeds: see test_fp8_decode_cpu.py


def _head_data(M, n, k, seed):
    """CPU data whose logits have a standard deviation of about 1: the top logits sit near 4, where a bf16 ulp (2^-6 ..
    2^-5) is below H.MARGIN, so a row the float64 reference calls confident cannot flip on the roundings of the
    logit chain alone."""
    g = torch.Generator().manual_seed(seed)
    w = _w_data(n, k, g)
    x = torch.randn(M, k, generator=g).to(BF)
    sd = float((x.double() @ w.double().T).std())
    return (w.float() * (1.0 / sd)).to(BF), x


@pytest.mark.parametrize("M,n,k,seed", HEAD_CASES)
def test_head(cuda, M, n, k, seed):
    w, x = _head_data(M, n, k, seed)
    w, x = w.to(cuda), x.to(cuda)
    q, _, s, wb = _quant(w)
    ld = K.round_up(n, 64)
    ntn = K.ceil_div(n, 128)
    # the raw product of the STORE kernel, then svla_softcap_ce_rows on it
    raw = torch.zeros(M, ld, dtype=BF, device=cuda)
    K.gemv_mxfp8(x, [q], [s], raw[:, :n])
    _assert_bound(_bf16_gemv(x, wb), x, wb, "bf16 GEMV on W'")
    _assert_bound(raw[:, :n], x, wb, "raw product")
    st_ref = torch.zeros(M, ntn, 3, device=cuda)
    K.softcap_ce_rows(raw, n, st_ref, CAP)
    logits = torch.zeros(M, ld, dtype=BF, device=cuda)
    st = torch.zeros(M, ntn, 3, device=cuda)
    K.head_gemv_mxfp8(x, q, s, logits, n, st, CAP)
    assert torch.equal(logits[:, :n], raw[:, :n])
    assert bool((logits[:, n:] == 0).all())  # columns >= N are not written
    assert torch.equal(st.view(torch.int32), st_ref.view(torch.int32))
    # finalize -> argmax against the float64 reference wherever it is confident
    lse, loss_rows = (torch.empty(M, device=cuda) for _ in range(2))
    am = torch.empty(M, dtype=torch.int64, device=cuda)
    loss2 = torch.empty(2, device=cuda)
    tgt = torch.full((M,), -1, dtype=torch.int64, device=cuda)
    K.ce_finalize(n, ntn, st, logits[:, :n], tgt, lse, am, loss_rows, loss2)
    ref = CAP * torch.tanh(x.double().cpu() @ wb.double().cpu().T / CAP)
    top2 = ref.topk(2, -1).values
    conf = (top2[:, 0] - top2[:, 1]) > H.MARGIN
    print(f"head [{M}, {n}, {k}]: {int(conf.sum())}/{M} rows confident, margins {[round(float(v), 3) for v in top2[:, 0] - top2[:, 1]]}")
    assert int(conf.sum()) * 4 >= 3 * M
    assert torch.equal(am.cpu()[conf], ref.argmax(-1)[conf])
    # twice: the same bits
    logits2 = torch.zeros_like(logits)
    st2 = torch.zeros_like(st)
    K.head_gemv_mxfp8(x, q, s, logits2, n, st2, CAP)
    assert torch.equal(logits, logits2) and torch.equal(st.view(torch.int32), st2.view(torch.int32))


def test_bad_arguments_launch_nothing(cuda):
    n = 24
    for M, k, msg in ((1, 136, "multiple of 128"), (9, 128, r"M in \[1, 8\]")):
        x = torch.ones(M, k, dtype=BF, device=cuda)
        q = torch.zeros(n, k, dtype=torch.float8_e4m3fn, device=cuda)
        s = torch.full((n, k // 32), 127, dtype=torch.uint8, device=cuda)
        y = _out(M, n, cuda)
        with pytest.raises(L.SvlaError, match=msg) as e:
            K.gemv_mxfp8(x, [q], [s], y)
        assert "code 1" in str(e.value)  # SVLA_ERR_ARG
        logits = torch.full((M, 64), 7.0, dtype=BF, device=cuda)
        st = torch.full((M, 1, 3), 7.0, device=cuda)
        with pytest.raises(L.SvlaError, match=msg):
            K.head_gemv_mxfp8(x, q, s, logits, n, st, CAP)
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()) and bool((logits == 7.0).all()) and bool((st == 7.0).all())
