"""svla_sample_rows (csrc/sample.hip) against the numpy restatement tests/sample_ref.py.

Shapes: N = 577 in a row stride of 640 whose pad columns hold +inf and NaN (they must not be read), M in {1, 8, 9, 64};
the full width N = 265 347 at M = 3.  Inputs bf16(30 tanh(x / 30)), x Gaussian of scale 3 (scale 4 at the full width).

Bounds, none taken from the kernel's output:
 * token: equal to the float64 restatement's wherever its two largest perturbed scores differ by more than 1e-3 (the
   kernel's fp32 score v / T + g carries ~1e-5 at |score| ~ 100); at most 1 % of rows may fall under that gate.
 * kept set (aux): exact for top-k (integer work); for top-p exact wherever the restatement's cumulative mass at the
   chosen threshold and at the one before it is more than 2e-5 away from top_p; at most 5 % of rows gated out.
 * log-probabilities: |kernel - float64| <= 4 e32 + 1e-6, e32 the error of the float32 restatement of the same
   formulas on the same inputs and tokens (the factor 4: another summation order).  Both errors are written to
   sample_rows.json in the parity directory the 4B parity tests use ($SVLA_PARITY_DIR or their default) before the
   assertion.
 * chi-square of 64 rows x 313 positions of one row of logits over the 31 most probable columns + rest: below the
   1 - 1e-6 quantile of chi-square(31), 83.6."""
import numpy as np
import pytest
import torch

import sample_ref as R
from spatialvla_amd import kernels as K

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SETTINGS = [(1.0, 0, 1.0), (1.0, 0, 0.9), (0.7, 50, 0.95), (2.0, 8, 0.5)]
SEED = 0x1234567890AB
_cache = {}
_parity = {}


def _logits(M, N, scale):
    """Shared inputs, seeded by the shape.  (The full-width seed is one on which the restatement's own gates leave no
    row out: three rows are too few for the gates' allowances to admit one.)"""
    key = (M, N, scale)
    if key not in _cache:
        _cache[key] = R.make_logits(np.random.default_rng(11 if N > 577 else 1000 + M + N), M, N, scale)
    return _cache[key]


def _dev(v, ld, cuda):
    """[M, N] float32 bf16 values -> bf16 device buffer [M, ld] whose pad columns alternate +inf / NaN."""
    M, N = v.shape
    buf = torch.empty(M, ld, dtype=BF)
    buf[:, :N] = torch.from_numpy(v).to(BF)
    if ld > N:
        buf[:, N:] = float("inf")
        buf[:, N + 1::2] = float("nan")
    return buf.to(cuda)


def _params(cuda, T, k, p, seed=SEED, draw=0, nranges=0):
    return K.pack_sample_params(T, p, k, seed, draw, nranges).to(cuda)


def _run(cuda, v, ld, T, k, p, position=7, rng=None, row_ids=None, seed=SEED, draw=0):
    M, N = v.shape
    ranges = step = None
    if rng is not None:
        # a table of capacity 4 with 3 entries in use; 4 % 3 == 1: the middle entry
        ranges = torch.tensor([[0, 1], list(rng), [2, 3], [5, 6]], dtype=torch.int32, device=cuda)
        step = torch.tensor([4], dtype=torch.int64, device=cuda)
    rid = None if row_ids is None else torch.tensor(row_ids, dtype=torch.int32, device=cuda)
    tok, lp, lpr, aux = K.sample_rows(_dev(v, ld, cuda), N, _params(cuda, T, k, p, seed, draw, 3), position, rid, ranges,
                                      step, aux=True)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), lp.cpu().numpy(), lpr.cpu().numpy(), aux.cpu().numpy()


def _write_parity():
    from test_full4b_gpu import _dump
    _dump("sample_rows.json", _parity)


def _check(cuda, name, v, ld, T, k, p, rng, positions=(7,)):
    """The kernel on every row of v at every position against the restatement.  The gates are pooled over the case's
    rows x positions; returns the kernel outputs of the first position."""
    M, N = v.shape
    lo, hi = rng if rng is not None else (0, N)
    gated_tok = gated_p = 0
    err = np.zeros((len(positions), M, 2))
    e32 = np.zeros((len(positions), M, 2))
    first = None
    for pi, pos in enumerate(positions):
        out = _run(cuda, v, ld, T, k, p, position=pos, rng=rng)
        first = first or out
        tok, lp, lpr, aux = out
        for m in range(M):
            kw = dict(temperature=T, top_k=k, top_p=p, seed=SEED, position=pos, row_id=m, lo=lo, hi=hi)
            r64 = R.sample_row(v[m], dtype=np.float64, **kw)
            r32 = R.sample_row(v[m], dtype=np.float32, **kw)
            t = int(tok[m])
            assert lo <= t < hi
            # the sampled token lies in the kernel's own kept set, whose size matches its threshold
            assert v[m, t] >= aux[m, 0]
            assert int(aux[m, 1]) == int((v[m, lo:hi] >= aux[m, 0]).sum())
            p_ok = p >= 1 or r64["p_gap"] > 2e-5
            if p_ok:
                assert aux[m, 0] == np.float32(r64["thr"]) and int(aux[m, 1]) == r64["kept"], (
                    name, m, aux[m], r64["thr"], r64["kept"])
            else:
                gated_p += 1
            if r64["gap"] > 1e-3 and p_ok:
                assert t == r64["token"], (name, pos, m, t, r64["token"], r64["gap"])
            else:
                gated_tok += 1
            if p_ok:  # the same kept set: the log-probabilities of the kernel's token are comparable
                ref, ref32 = R.logprobs(r64, v[m], t), R.logprobs(r32, v[m], t)
                err[pi, m] = abs(float(lp[m]) - ref[0]), abs(float(lpr[m]) - ref[1])
                e32[pi, m] = abs(ref32[0] - ref[0]), abs(ref32[1] - ref[1])
    rows = M * len(positions)
    _parity[name] = {"rows": rows, "gated_token_rows": gated_tok, "gated_top_p_rows": gated_p,
                     "logprob_err_kernel": float(err[..., 0].max()), "logprob_err_f32": float(e32[..., 0].max()),
                     "logprob_raw_err_kernel": float(err[..., 1].max()),
                     "logprob_raw_err_f32": float(e32[..., 1].max())}
    print(name, _parity[name])
    _write_parity()
    assert gated_tok <= 0.01 * rows, (name, gated_tok)
    assert gated_p <= 0.05 * rows, (name, gated_p)
    assert err[..., 0].max() <= 4 * e32[..., 0].max() + 1e-6
    assert err[..., 1].max() <= 4 * e32[..., 1].max() + 1e-6
    return first


@pytest.mark.parametrize("ranged", [False, True])
@pytest.mark.parametrize("T,k,p", SETTINGS)
def test_small(cuda, T, k, p, ranged):
    """M = 64 at four positions (256 rows share the gates' allowances) against the restatement; M = 1, 8, 9 are the
    same rows with the same row ids, so they must reproduce the 64-row run's bits."""
    v = _logits(64, 577, 3.0)
    rng = (101, 409) if ranged else None
    big = _check(cuda, f"N577_M64_T{T}_k{k}_p{p}_{'range' if ranged else 'all'}", v, 640, T, k, p, rng,
                 positions=(7, 8, 9, 10))
    for M in (1, 8, 9):
        for a, b in zip(big, _run(cuda, v[:M], 640, T, k, p, rng=rng)):
            assert a[:M].tobytes() == b.tobytes(), (M, T, k, p)


@pytest.mark.parametrize("ranged", [False, True])
@pytest.mark.parametrize("T,k,p", SETTINGS)
def test_full_width(cuda, T, k, p, ranged):
    N = 265347
    v = _logits(3, N, 4.0)
    _check(cuda, f"N{N}_M3_T{T}_k{k}_p{p}_{'range' if ranged else 'all'}", v, K.round_up(N, 64), T, k, p,
           (257153, 261249) if ranged else None)


def test_top_k_1_is_the_row_maximum(cuda):
    v = _logits(64, 577, 3.0)
    tok, lp, _, aux = _run(cuda, v, 640, 1.3, 1, 1.0)
    assert (v[np.arange(64), tok] == v.max(1)).all()
    assert (aux[:, 0] == v.max(1)).all()
    ties = (v == v.max(1, keepdims=True)).sum(1)
    assert (aux[:, 1] == ties).all()
    assert np.allclose(lp, -np.log(ties), atol=1e-6)


@pytest.mark.parametrize("rng", [None, (101, 409)])
def test_greedy_is_the_first_argmax(cuda, rng):
    v = _logits(64, 577, 3.0).copy()
    v[5, 300] = v[5, 200] = 31.0  # an exact tie above every other value: the first column wins
    tok, lp, lpr, _ = _run(cuda, v, 640, 0.0, 50, 0.5, rng=rng)
    lo, hi = rng if rng is not None else (0, 577)
    assert (tok == lo + v[:, lo:hi].argmax(1)).all()
    v64 = v.astype(np.float64)
    vt = v64[np.arange(64), tok]
    lse = lambda x: x.max(1) + np.log(np.exp(x - x.max(1, keepdims=True)).sum(1))
    assert np.abs(lp - (vt - lse(v64[:, lo:hi]))).max() < 2e-6
    assert np.abs(lpr - (vt - lse(v64))).max() < 2e-6


def test_row_invariance(cuda):
    """A row alone at M = 1 and the same row as row 37 of 64 with its row id: the same bits."""
    v = _logits(64, 577, 3.0)
    for (T, k, p) in SETTINGS:
        big = _run(cuda, v, 640, T, k, p, row_ids=list(range(100, 164)))
        one = _run(cuda, v[37:38], 640, T, k, p, row_ids=[137])
        for a, b in zip(big, one):
            assert a[37].tobytes() == b[0].tobytes()
    vf = _logits(3, 265347, 4.0)
    big = _run(cuda, vf, K.round_up(265347, 64), 0.7, 50, 0.95, row_ids=[5, 6, 7])
    one = _run(cuda, vf[2:3], K.round_up(265347, 64), 0.7, 50, 0.95, row_ids=[7])
    for a, b in zip(big, one):
        assert a[2].tobytes() == b[0].tobytes()


def test_draw_and_seed_change_the_noise(cuda):
    v = _logits(64, 577, 3.0)
    base = _run(cuda, v, 640, 1.0, 0, 1.0)[0]
    assert (base == _run(cuda, v, 640, 1.0, 0, 1.0)[0]).all()
    assert (base != _run(cuda, v, 640, 1.0, 0, 1.0, draw=1)[0]).any()
    assert (base != _run(cuda, v, 640, 1.0, 0, 1.0, seed=SEED + (1 << 32))[0]).any()
    assert (base != _run(cuda, v, 640, 1.0, 0, 1.0, position=8)[0]).any()


def test_chi_square(cuda):
    row = R.make_logits(np.random.default_rng(5), 1, 577, 2.0)
    buf = _dev(np.repeat(row, 64, 0), 640, cuda)
    params = _params(cuda, 1.0, 0, 1.0, seed=99)
    toks = torch.empty(313, 64, dtype=torch.int64, device=cuda)
    lp = torch.empty(64, dtype=torch.float32, device=cuda)
    lpr = torch.empty(64, dtype=torch.float32, device=cuda)
    for pos in range(313):
        K.sample_rows(buf, 577, params, pos, out=(toks[pos], lp, lpr))
    chi = R.chi_square_top31(row[0], toks.cpu().numpy().ravel())
    print(f"chi-square(31) over {toks.numel()} kernel draws: {chi:.1f} (bound {R.CHI2_31_Q})")
    assert chi < R.CHI2_31_Q


def test_special_values(cuda):
    v = _logits(8, 577, 3.0).copy()
    # rule 6: a NaN among the allowed columns -> the first such column, NaN log-probabilities
    v[0, 300] = v[0, 200] = np.nan
    # a NaN outside the allowed range is not a NaN of the draw
    tok, lp, lpr, aux = _run(cuda, v, 640, 1.0, 0, 0.9, rng=(250, 400))
    assert tok[0] == 300 and np.isnan(lp[0]) and np.isnan(lpr[0]) and np.isnan(aux[0, 0]) and aux[0, 1] == 0
    assert not np.isnan(lp[1:]).any() and ((tok >= 250) & (tok < 400)).all()
    tok, lp, lpr, _ = _run(cuda, v, 640, 1.0, 0, 0.9, rng=(301, 400))
    assert 301 <= tok[0] < 400 and np.isfinite(lp[0]) and np.isnan(lpr[0])
    # a single finite allowed column
    w = np.full((2, 577), -np.inf, dtype=np.float32)
    w[:, 123] = -4.5
    for (T, k, p) in SETTINGS:
        tok, lp, lpr, aux = _run(cuda, w, 640, T, k, p)
        assert (tok == 123).all() and (lp == 0).all() and (lpr == 0).all()
        assert (aux[:, 0] == -4.5).all() or k == 0 and p >= 1
    # a range of width 1
    tok, lp, lpr, aux = _run(cuda, v, 640, 2.0, 8, 0.5, rng=(411, 412))
    assert (tok == 411).all() and (lp == 0).all() and (aux[:, 1] == 1).all()
    assert (lpr[1:] < 0).all()


def test_refusals(cuda):
    buf = torch.zeros(2, 640, dtype=BF, device=cuda)
    with pytest.raises(ValueError):
        K.sample_rows(buf, 577, torch.zeros(8, dtype=torch.uint8, device=cuda), 0)
    with pytest.raises(ValueError):
        K.sample_rows(buf, 577, _params(cuda, 1.0, 0, 1.0), 0, row_ids=torch.zeros(2, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError):
        K.sample_rows(buf.float(), 577, _params(cuda, 1.0, 0, 1.0), 0)
