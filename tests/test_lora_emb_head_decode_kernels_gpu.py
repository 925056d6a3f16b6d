"""The two decode-step kernels of enable_lora_decode(emb_head=True) against the launches they replace, bit for bit
(no tolerance anywhere in this file):

svla_lora_head_gemv  against svla_lora_gemv (STORE) + svla_softcap_ce_rows on the same inputs -- logits[:, :N], the
                     three statistics of every 128-column group and the argmax / lse after svla_ce_finalize -- and,
                     with B = 0, against the base decode head (the plain-store projection + svla_softcap_ce_rows).
                     M in {1, 5, 8}, K in {256, 2304}, r in {8, 32, 64}, N in {72, 131, 577} (less than one 128-row
                     block, a 3-column tail as at the 4B vocabulary, the tiny model's odd vocabulary), the 4B width
                     N = 265347 once, a NaN column and an all-zero row (softcap.hip's separate paths).
svla_lora_embed_decode against svla_embed_merge + svla_lora_embed_fwd: rows in {1, 5, 8}, H in {256, 2304}, na in
                     {64, 8194}, ids mixing text ids with a0, a0 + na - 1, a0 - 1 and a0 + na.
Refused arguments report through svla_last_error() and launch nothing; columns [N, ld) of the logits keep their bits."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CAP, SCALE = 30.0, 2.0
SENTINEL = 3.0  # bf16 0x4040: the pre-filled logits buffer


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _inputs(M, N, K, r, seed, zero_B=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s, scale: (torch.randn(*s, generator=g, device="cuda") * scale).to(BF)
    x = rn(M, K, scale=1.0)
    w = rn(N, K, scale=K ** -0.5 * 8.0)  # raw logits of a few units: inside the tanh table and beyond it
    A = rn(r, K, scale=K ** -0.5)
    B = torch.zeros(N, r, dtype=BF, device="cuda") if zero_B else rn(N, r, scale=0.5)
    return x, w, A, B


def _finalize(Kn, N, stats, logits):
    M = logits.shape[0]
    tgt = torch.full((M,), -1, dtype=torch.int64, device="cuda")
    lse = torch.empty(M, dtype=torch.float32, device="cuda")
    am = torch.empty(M, dtype=torch.int64, device="cuda")
    rows = torch.empty(M, dtype=torch.float32, device="cuda")
    loss2 = torch.empty(2, dtype=torch.float32, device="cuda")
    Kn.ce_finalize(N, stats.shape[1], stats, logits[:, :N], tgt, lse, am, rows, loss2)
    return am, lse


def _head_pair(x, w, A, B, r, base=False):
    """(new kernel, composition): each (logits buffer [M, ld] pre-filled, stats, argmax, lse)."""
    from spatialvla_amd import kernels as Kn
    M, N = x.shape[0], w.shape[0]
    ld, ntn = Kn.round_up(N, 64), Kn.ceil_div(N, 128)
    t = torch.empty(M, Kn.lora_R(r), dtype=BF, device="cuda")
    Kn.lora_gemv_down(x, [A], r, t)
    out = []
    for new in (True, False):
        buf = torch.full((M, ld), SENTINEL, dtype=BF, device="cuda")
        stats = torch.full((M, ntn, 3), -7.0, dtype=torch.float32, device="cuda")
        if new:
            Kn.lora_head_gemv(x, w, t, B, r, SCALE, buf, N, stats, CAP)
        else:
            if base:
                Kn.linear_fwd(x, [w], buf[:, :N])
            else:
                Kn.lora_gemv(x, [w], t, [B], r, SCALE, buf)
            Kn.softcap_ce_rows(buf, N, stats, CAP)
        out.append((buf, stats) + _finalize(Kn, N, stats, buf))
    torch.cuda.synchronize()
    return out


def _assert_head_equal(got, want, N, what):
    (lg, st, am, lse), (lg_w, st_w, am_w, lse_w) = got, want
    assert _same(lg[:, :N], lg_w[:, :N]), (what, "logits")
    for i, nm in enumerate(("max", "sum exp", "argmax")):
        assert _same(st[..., i], st_w[..., i]), (what, nm)
    assert torch.equal(am, am_w) and _same(lse, lse_w), (what, "finalize")
    pad = lg[:, N:]
    assert pad.numel() == 0 or bool((pad == SENTINEL).all()), (what, "columns [N, ld) were written")


@pytest.mark.parametrize("K", [256, 2304])
@pytest.mark.parametrize("M", [1, 5, 8])
def test_head_gemv_bitwise(cuda, M, K):
    for r in (8, 32, 64):
        for N in (72, 131, 577):
            seed = 1000 * M + K + 7 * r + N
            x, w, A, B = _inputs(M, N, K, r, seed)
            got, want = _head_pair(x, w, A, B, r)
            _assert_head_equal(got, want, N, f"M{M} K{K} r{r} N{N} vs lora_gemv + softcap_ce_rows")
            # the adapter term is in the logits (a dropped term would also pass an equality of two wrong results)
            x0, w0, A0, B0 = _inputs(M, N, K, r, seed, zero_B=True)
            assert torch.equal(x0, x) and torch.equal(w0, w)
            got0, base = _head_pair(x, w, A, B0, r, base=True)
            _assert_head_equal(got0, base, N, f"M{M} K{K} r{r} N{N} B = 0 vs the base head")
            assert not _same(got[0][:, :N], got0[0][:, :N])


def test_head_gemv_4b_width(cuda):
    M, N, K, r = 1, 265347, 2304, 32
    x, w, A, B = _inputs(M, N, K, r, 5)
    got, want = _head_pair(x, w, A, B, r)
    _assert_head_equal(got, want, N, "4B width")
    assert 0 <= int(got[2][0]) < N
    del got, want
    got0, base = _head_pair(x, w, A, torch.zeros_like(B), r, base=True)
    _assert_head_equal(got0, base, N, "4B width, B = 0 vs the base head")


@pytest.mark.parametrize("case", ["nan", "zeros"])
def test_head_gemv_special_rows(cuda, case):
    """A NaN logit (one weight row is NaN: the lane's chunk takes softcap.hip's per-element path, the NaN is skipped
    by the statistics) and an all-zero logits row (x row zero: the zero maximum, whose argmax is the first column)."""
    M, N, K, r = 5, 577, 256, 8
    x, w, A, B = _inputs(M, N, K, r, 11)
    if case == "nan":
        w[130] = float("nan")
        w[576] = float("nan")  # the ragged last chunk
    else:
        x[2] = 0
    got, want = _head_pair(x, w, A, B, r)
    _assert_head_equal(got, want, N, case)
    if case == "nan":
        assert bool(got[0][:, 130].isnan().all()) and bool(got[0][:, 576].isnan().all())
        assert int(got[0][:, :N].isnan().sum()) == 2 * M and bool(torch.isfinite(got[1][..., 0]).all())
    else:
        assert float(got[0][2, :N].abs().max()) == 0.0 and int(got[2][2]) == 0
    got0, base = _head_pair(x, w, A, torch.zeros_like(B), r, base=True)
    _assert_head_equal(got0, base, N, case + ", B = 0 vs the base head")


# ---------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("na", [64, 8194])
@pytest.mark.parametrize("H", [256, 2304])
@pytest.mark.parametrize("rows", [1, 5, 8])
def test_embed_decode_bitwise(cuda, rows, H, na):
    from spatialvla_amd import kernels as Kn
    a0, r = 300, 16
    vocab = a0 + na + 40
    g = torch.Generator(device="cuda").manual_seed(rows * 31 + H + na)
    rn = lambda *s, scale: (torch.randn(*s, generator=g, device="cuda") * scale).to(BF)
    embed, spatial = rn(vocab, H, scale=0.05), rn(na, H, scale=0.05)
    A, B = rn(r, na, scale=0.05), rn(H, r, scale=0.5)
    norm = float(torch.tensor(H ** 0.5, dtype=BF))
    pool = [a0, 5, a0 + na - 1, a0 - 1, a0 + na, a0 + na // 2, 0, vocab - 1]
    for start in range(len(pool) if rows == 1 else 1):  # a single row: every kind of id in turn
        ids = torch.tensor([pool[(start + i) % len(pool)] for i in range(rows)], dtype=torch.int64, device="cuda")
        want = torch.full((rows, H), SENTINEL, dtype=BF, device="cuda")
        Kn.embed_merge(ids, None, embed, spatial, a0, na, None, norm, want)
        plain = want.clone()
        Kn.lora_embed_fwd(ids, None, embed, spatial, a0, A, B, r, SCALE, norm, want)
        got = torch.full((rows, H), SENTINEL, dtype=BF, device="cuda")
        Kn.lora_embed_decode(ids, embed, spatial, a0, A, B, r, SCALE, norm, got)
        torch.cuda.synchronize()
        assert _same(got, want), ids.tolist()
        inside = (ids >= a0) & (ids < a0 + na)
        assert _same(got[~inside], plain[~inside])
        if bool(inside.any()):  # the adapter moved the action rows
            assert not _same(got[inside], plain[inside])


# ---------------------------------------------------------------------------------------- refusals
def _head_args(M=1, N=131, K=256, r=8, x_off=0, ld=None):
    x, w, A, B = _inputs(max(M, 1), N, K if K % 8 == 0 else K + 8 - K % 8, 8 if r % 8 else r, 3)
    M_alloc = max(M, 1)
    t = torch.zeros(M_alloc, 64, dtype=BF, device="cuda")
    ld = ld or (N + 63) // 64 * 64
    buf = torch.full((M_alloc, ld), SENTINEL, dtype=BF, device="cuda")
    stats = torch.full((M_alloc, (N + 127) // 128, 3), -7.0, dtype=torch.float32, device="cuda")
    keep = (x, w, A, B, t)
    args = [M, N, K, x.data_ptr() + x_off, x.stride(0), w.data_ptr(), w.stride(0), t.data_ptr(), t.stride(0),
            B.data_ptr(), B.stride(0), r, SCALE, CAP, buf.data_ptr(), ld, stats.data_ptr(), None]
    return args, buf, stats, keep


@pytest.mark.parametrize("what,kw", [("M = 9", dict(M=9)), ("M = 0", dict(M=0)), ("misaligned x", dict(x_off=2)),
                                     ("r = 12", dict(r=12)), ("r = 72", dict(r=72)), ("K % 8", dict(K=260)),
                                     ("K above 4096", dict(K=4104)), ("ld below N", dict(ld=128))])
def test_head_gemv_refuses(cuda, what, kw):
    from spatialvla_amd import _lib as L
    args, buf, stats, keep = _head_args(**kw)
    if what == "K above 4096":
        args[4] = args[6] = 4104  # row strides that would admit the K
    if what == "ld below N":
        args[15] = 128
    rc = L.lib().svla_lora_head_gemv(*args)
    torch.cuda.synchronize()
    assert rc != 0, what
    assert b"lora_head_gemv" in L.lib().svla_last_error()
    assert bool((buf == SENTINEL).all()) and bool((stats == -7.0).all()), "a refused call launched"


def test_head_gemv_wrapper_refuses(cuda):
    from spatialvla_amd import kernels as Kn
    x, w, A, B = _inputs(2, 131, 256, 8, 3)
    t = torch.zeros(2, 32, dtype=BF, device="cuda")
    buf = torch.zeros(2, 192, dtype=BF, device="cuda")
    stats = torch.zeros(2, 2, 3, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        Kn.lora_head_gemv(x, w, t, B[:100], 8, SCALE, buf, 131, stats, CAP)
    with pytest.raises(ValueError):
        Kn.lora_head_gemv(x, w, t, B, 8, SCALE, buf, 131, stats[:, :1], CAP)


@pytest.mark.parametrize("what,kw", [("rows = 9", dict(rows=9)), ("r = 12", dict(r=12)), ("H % 8", dict(H=260)),
                                     ("misaligned out", dict(out_off=2))])
def test_embed_decode_refuses(cuda, what, kw):
    from spatialvla_amd import _lib as L
    rows, r, H, out_off = kw.get("rows", 2), kw.get("r", 8), kw.get("H", 256), kw.get("out_off", 0)
    a0, na = 100, 64
    embed = torch.zeros(200, 264, dtype=BF, device="cuda")
    spatial = torch.zeros(na, 264, dtype=BF, device="cuda")
    A = torch.zeros(16, na, dtype=BF, device="cuda")
    B = torch.zeros(264, 16, dtype=BF, device="cuda")
    ids = torch.full((16,), a0, dtype=torch.int64, device="cuda")
    out = torch.full((16, 264), SENTINEL, dtype=BF, device="cuda")
    rc = L.lib().svla_lora_embed_decode(rows, H, ids.data_ptr(), embed.data_ptr(), spatial.data_ptr(), a0, na,
                                        A.data_ptr(), B.data_ptr(), r, SCALE, 16.0, out.data_ptr() + out_off, None)
    torch.cuda.synchronize()
    assert rc != 0, what
    assert b"lora_embed_decode" in L.lib().svla_last_error()
    assert bool((out == SENTINEL).all()), "a refused call launched"
