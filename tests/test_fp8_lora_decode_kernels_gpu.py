"""The e4m3 adapter GEMVs of the decode step (csrc/fp8_decode.hip): svla_lora_gemv_mxfp8 and svla_lora_head_gemv_mxfp8.

Most checks are bitwise and need no tolerance: the output must equal bf16(float(Y0) + float(Yad)) with Y0 =
svla_gemv_mxfp8 on the same operands (the base sum, bit for bit) and Yad = svla_lora_gemv on an all-zero W, which is
exactly bf16(s l) (the adapter term and its rounding); with B = 0 it must equal Y0.  The float64 restatement applies
test_fp8_decode_kernels_gpu.py's derived product bound to the base part and test_lora_decode_kernels_gpu.py's rel-L2 <
5e-3 (bf16 outputs of fp32 sums) to the sum with the adapter term taken in float64 from the kernel's T.  The scaling is
chosen per case so the adapter term's rms equals the base term's: a wrong slice or segment map is an O(1) error."""
import pytest
import torch

import harness as H
from spatialvla_amd import _lib as L
from spatialvla_amd import kernels as K
from test_fp8_decode_kernels_gpu import CAP, _assert_bound, _geglu_formula, _out, _quant, _w_data

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TOL = 5e-3  # test_lora_decode_kernels_gpu.py


def _R(r):
    return (r + 31) // 32 * 32


def _case(M, sizes, k, r, seed, dev, w_scale=1.0):
    """x, the quantised segments, A_s / B_s per segment (each its own values), T from svla_lora_gemv_down, Y0 and the
    scaling that makes rms(adapter term) = rms(Y0).  Generated on the CPU."""
    g = torch.Generator().manual_seed(seed)
    ws = [_w_data(n, k, g, w_scale).to(dev) for n in sizes]
    x = torch.randn(M, k, generator=g).to(BF).to(dev)
    As = [(torch.randn(r, k, generator=g) / r).to(BF).to(dev) for _ in sizes]
    Bs = [(torch.randn(n, r, generator=g) * (0.7 + 0.3 * i)).to(BF).to(dev) for i, n in enumerate(sizes)]
    qs, ss, wbs = [], [], []
    for w in ws:
        q, _, s, wb = _quant(w)
        qs.append(q), ss.append(s), wbs.append(wb)
    R = _R(r)
    t = torch.full((M, len(sizes) * R), float("nan"), dtype=BF, device=dev)
    K.lora_gemv_down(x, As, r, t)
    y0 = _out(M, sum(sizes), dev)
    K.gemv_mxfp8(x, qs, ss, y0)
    raw = torch.cat([t[:, i * R:i * R + r].double() @ b.double().T for i, b in enumerate(Bs)], 1)
    finite = torch.isfinite(y0.double())
    s = float(y0.double()[finite].pow(2).mean().sqrt() / raw.pow(2).mean().sqrt())
    return dict(x=x, qs=qs, ss=ss, wb=torch.cat(wbs, 0), As=As, Bs=Bs, t=t, y0=y0, s=s, raw=raw, r=r, sizes=sizes)


def _yad(c):
    """svla_lora_gemv on an all-zero W: bf16(bf16(0) + bf16(s l)) = bf16(s l), the adapter term with its rounding."""
    x = c["x"]
    zs = [torch.zeros(n, x.shape[1], dtype=BF, device=x.device) for n in c["sizes"]]
    out = _out(x.shape[0], sum(c["sizes"]), x.device)
    K.lora_gemv(x, zs, c["t"], c["Bs"], c["r"], c["s"], out)
    return out


def _sum_bf16(a, b):
    return (a.float() + b.float()).to(BF)


STORE_CASES = ([(48, 128, r) for r in (8, 64)] + [(144, 256, r) for r in (8, 64)]
               + [(1008, 2304, 32), (528, 9216, 32)]  # KCH = 3; the split-K form
               + [(49, 128, 8)])  # the kernel pairs rows: the last wave owns a single row


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("n,k,r", STORE_CASES)
def test_store(cuda, M, n, k, r):
    c = _case(M, [n], k, r, 1000 * M + n + k + r, cuda)
    x, y0 = c["x"], c["y0"]
    y = _out(M, n, cuda)
    K.lora_gemv_mxfp8(x, c["qs"], c["ss"], c["t"], c["Bs"], r, c["s"], y)
    yad = _yad(c)
    assert float(yad.float().abs().max()) > 0
    assert torch.equal(y, _sum_bf16(y0, yad))
    assert not torch.equal(y, y0)
    # B = 0, T != 0: the base kernel's bits
    yz = _out(M, n, cuda)
    K.lora_gemv_mxfp8(x, c["qs"], c["ss"], c["t"], [torch.zeros_like(b) for b in c["Bs"]], r, c["s"], yz)
    assert torch.equal(yz, y0)
    # twice: the same bits
    y2 = _out(M, n, cuda)
    K.lora_gemv_mxfp8(x, c["qs"], c["ss"], c["t"], c["Bs"], r, c["s"], y2)
    assert torch.equal(y, y2)
    # float64: the derived bound on the base part, rel-L2 on the sum
    _assert_bound(yz, x, c["wb"], "base part")
    ref = x.double().cpu() @ c["wb"].double().cpu().T + c["s"] * c["raw"].cpu()
    rel = H.rel_l2(y, ref.float())
    print(f"lora_gemv_mxfp8 M={M} N={n} K={k} r={r}: rel-L2 against float64 {rel:.2e}")
    assert rel < TOL


def test_three_segments(cuda):
    M, k, r, sizes = 3, 256, 32, [64, 32, 32]  # q|k|v, unequal, a different B per segment
    c = _case(M, sizes, k, r, 77, cuda)
    y = _out(M, sum(sizes), cuda)
    K.lora_gemv_mxfp8(c["x"], c["qs"], c["ss"], c["t"], c["Bs"], r, c["s"], y)
    assert torch.equal(y, _sum_bf16(c["y0"], _yad(c)))
    ref = c["x"].double().cpu() @ c["wb"].double().cpu().T + c["s"] * c["raw"].cpu()
    assert H.rel_l2(y, ref.float()) < TOL
    # a swapped pair of B segments is seen
    sw = dict(c, Bs=[c["Bs"][0], c["Bs"][2], c["Bs"][1]])
    assert not torch.equal(y, _sum_bf16(c["y0"], _yad(sw)))


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("I,k", [(144, 256), (144, 2304), (528, 256), (528, 2304)])
def test_geglu(cuda, M, I, k):
    r = 32
    c = _case(M, [I, I], k, r, 31 * M + I + k, cuda, w_scale=0.05)
    h, g, u = (_out(M, I, cuda) for _ in range(3))
    K.lora_gemv_mxfp8(c["x"], c["qs"], c["ss"], c["t"], c["Bs"], r, c["s"], h, geglu_out=(g, u))
    want = _sum_bf16(c["y0"], _yad(c))  # g | u through the STORE forms of both parents
    assert torch.equal(g, want[:, :I]) and torch.equal(u, want[:, I:])
    assert torch.equal(h, _geglu_formula(g, u))
    # the STORE form on the same two segments gives the same g | u
    y = _out(M, 2 * I, cuda)
    K.lora_gemv_mxfp8(c["x"], c["qs"], c["ss"], c["t"], c["Bs"], r, c["s"], y)
    assert torch.equal(y, want)


def test_nan_block(cuda):
    g = torch.Generator().manual_seed(5)
    n, k, M, r = 48, 256, 3, 8
    w = _w_data(n, k, g)
    w[5, 32:64] = float("nan")
    w = w.to(cuda)
    x = torch.randn(M, k, generator=g).to(BF).to(cuda)
    q, sc = K.quant_mx_rows(w)
    s = K.mx_scales_rowmajor(sc)
    assert int(s[5, 1]) == 0xFF
    A = (torch.randn(r, k, generator=g) / r).to(BF).to(cuda)
    B = torch.randn(n, r, generator=g).to(BF).to(cuda)
    t = torch.empty(M, _R(r), dtype=BF, device=cuda)
    K.lora_gemv_down(x, [A], r, t)
    y = _out(M, n, cuda)
    K.lora_gemv_mxfp8(x, [q], [s], t, [B], r, 2.0, y)
    assert bool(y[:, 5].isnan().all())
    keep = [i for i in range(n) if i != 5]
    assert bool(torch.isfinite(y[:, keep].float()).all())


def _head_case(M, n, k, r, seed, dev="cpu"):
    """test_fp8_decode_kernels_gpu._head_data's logits (standard deviation about 1) with an adapter term of half that:
    w, x, A, B on the CPU and the scaling; T is bf16(x A^T)."""
    from test_fp8_decode_kernels_gpu import _head_data
    w, x = _head_data(M, n, k, seed)
    g = torch.Generator().manual_seed(seed + 1)
    A = (torch.randn(r, k, generator=g) / r).to(BF)
    B = torch.randn(n, r, generator=g).to(BF)
    t = (x.double() @ A.double().T).to(BF)
    s = 0.5 / float((t.double() @ B.double().T).std())
    return w, x, A, B, s


def _head_run(x, q, s8, t, B, r, s, n, dev):
    M = x.shape[0]
    logits = torch.zeros(M, K.round_up(n, 64), dtype=BF, device=dev)
    st = torch.zeros(M, K.ceil_div(n, 128), 3, device=dev)
    K.lora_head_gemv_mxfp8(x, q, s8, t, B, r, s, logits, n, st, CAP)
    return logits, st


@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("n,k", [(1008, 256), (2064, 256), (1008, 2304), (2064, 2304)])
def test_head_bitwise(cuda, M, n, k):
    r = 32
    w, x, A, B, s = (v.to(cuda) if torch.is_tensor(v) else v for v in _head_case(M, n, k, r, 3 * n + k + M))
    q, _, s8, _ = _quant(w)
    t = torch.empty(M, _R(r), dtype=BF, device=cuda)
    K.lora_gemv_down(x, [A], r, t)
    ld, ntn = K.round_up(n, 64), K.ceil_div(n, 128)
    # B = 0: the head of enable_fp8_decode, logits and statistics
    l0 = torch.zeros(M, ld, dtype=BF, device=cuda)
    st0 = torch.zeros(M, ntn, 3, device=cuda)
    K.head_gemv_mxfp8(x, q, s8, l0, n, st0, CAP)
    lz, stz = _head_run(x, q, s8, t, torch.zeros_like(B), r, s, n, cuda)
    assert torch.equal(lz, l0) and torch.equal(stz.view(torch.int32), st0.view(torch.int32))
    # B != 0: svla_softcap_ce_rows applied to the STORE kernel's output on the same operands
    raw = torch.zeros(M, ld, dtype=BF, device=cuda)
    K.lora_gemv_mxfp8(x, [q], [s8], t, [B], r, s, raw[:, :n])
    st_ref = torch.zeros(M, ntn, 3, device=cuda)
    K.softcap_ce_rows(raw, n, st_ref, CAP)
    lg, st = _head_run(x, q, s8, t, B, r, s, n, cuda)
    assert torch.equal(lg[:, :n], raw[:, :n]) and not torch.equal(lg, l0)
    assert bool((lg[:, n:] == 0).all())  # columns >= N are not written
    assert torch.equal(st.view(torch.int32), st_ref.view(torch.int32))
    lg2, st2 = _head_run(x, q, s8, t, B, r, s, n, cuda)
    assert torch.equal(lg, lg2) and torch.equal(st.view(torch.int32), st2.view(torch.int32))


HEAD_CASES = [(8, 2050, 2304, 32, 10), (1, 2050, 256, 8, 3)]  # (M, N, K, r, seed); seeds: test_fp8_lora_decode_cpu.py


def head_reference(x, wd, t, B, s):
    """The float64 logits of the adapted head on dequantised weights wd and a given T."""
    return CAP * torch.tanh((x.double() @ wd.double().T + s * (t.double() @ B.double().T)) / CAP)


@pytest.mark.parametrize("M,n,k,r,seed", HEAD_CASES)
def test_head_ragged_n(cuda, M, n, k, r, seed):
    """An N that is no multiple of 16 (the STORE form refuses it): the argmax after svla_ce_finalize against the
    float64 reference wherever that is confident."""
    w, x, A, B, s = (v.to(cuda) if torch.is_tensor(v) else v for v in _head_case(M, n, k, r, seed))
    q, _, s8, wb = _quant(w)
    t = torch.empty(M, _R(r), dtype=BF, device=cuda)
    K.lora_gemv_down(x, [A], r, t)
    lg, st = _head_run(x, q, s8, t, B, r, s, n, cuda)
    lse, loss_rows = (torch.empty(M, device=cuda) for _ in range(2))
    am = torch.empty(M, dtype=torch.int64, device=cuda)
    loss2 = torch.empty(2, device=cuda)
    tgt = torch.full((M,), -1, dtype=torch.int64, device=cuda)
    K.ce_finalize(n, K.ceil_div(n, 128), st, lg[:, :n], tgt, lse, am, loss_rows, loss2)
    ref = head_reference(x.cpu(), wb.cpu(), t[:, :r].cpu(), B.cpu(), s)
    top2 = ref.topk(2, -1).values
    mg = top2[:, 0] - top2[:, 1]
    conf = mg > H.MARGIN
    print(f"adapter head [{M}, {n}, {k}]: {int(conf.sum())}/{M} rows confident, margins {[round(float(v), 3) for v in mg]}")
    assert int(conf.sum()) * 4 >= 3 * M
    assert torch.equal(am.cpu()[conf], ref.argmax(-1)[conf])
    assert bool((lg[:, n:] == 0).all())


def test_bad_arguments_launch_nothing(cuda):
    n = 48

    def operands(M, k, r, ldb=None):
        x = torch.ones(M, k, dtype=BF, device=cuda)
        q = torch.zeros(n * k + 16, dtype=torch.float8_e4m3fn, device=cuda)
        s = torch.full((n, k // 32), 127, dtype=torch.uint8, device=cuda)
        t = torch.ones(M, 96, dtype=BF, device=cuda)
        B = torch.ones(n, ldb or r, dtype=BF, device=cuda)[:, :r]
        return x, q, s, t, B

    cases = [(9, 128, 8, 0, None, r"M in \[1, 8\]"), (1, 136, 8, 0, None, "multiple of 128"),
             (1, 128, 65, 0, 72, r"rank must be a multiple of 8 in \[8, 64\]"), (1, 128, 8, 1, None, "16-B aligned")]
    for M, k, r, off, ldb, msg in cases:
        x, qf, s, t, B = operands(M, k, r, ldb)
        q = qf[off:off + n * k].view(n, k)
        y = _out(M, n, cuda)
        with pytest.raises(L.SvlaError, match=msg) as e:
            K.lora_gemv_mxfp8(x, [q], [s], t, [B], r, 1.0, y)
        assert "code 1" in str(e.value)  # SVLA_ERR_ARG
        logits = torch.full((M, 64), 7.0, dtype=BF, device=cuda)
        st = torch.full((M, 1, 3), 7.0, device=cuda)
        with pytest.raises(L.SvlaError, match=msg) as e:
            K.lora_head_gemv_mxfp8(x, q, s, t, B, r, 1.0, logits, n, st, CAP)
        assert "code 1" in str(e.value)
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()) and bool((logits == 7.0).all()) and bool((st == 7.0).all())
