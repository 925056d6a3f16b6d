"""numpy restatement of svla_sample_rows (include/svla.h): allowed range, top-k, top-p, Gumbel-max over Philox4x32-10,
and the two log-probabilities.  `dtype` selects the arithmetic of the weights and sums: float64 is the reference the
kernel is compared with, float32 the yardstick of what fp32 arithmetic costs on the same formulas.  The noise is
always float64."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on broadcastable counter words; returns the four output words (uint64
    arrays holding 32-bit values)."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in (c0, c1, c2, c3)]
    c = [np.array(x) for x in np.broadcast_arrays(*c)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> _S32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> _S32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def gumbel(cols, position, row_id, seed, draw=0):
    """g = -log(-log u) for the given columns (broadcasts over position / row_id arrays), float64."""
    cols = np.asarray(cols, dtype=np.uint64)
    seed = int(seed)
    w = philox4x32_10(cols >> np.uint64(2), position, row_id, int(draw) & 0xFFFFFFFF, seed & 0xFFFFFFFF,
                      (seed >> 32) & 0xFFFFFFFF)
    sel = np.broadcast_to(cols & np.uint64(3), w[0].shape)
    word = np.choose(sel.astype(np.int64), w)
    u = ((word >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u))


def _lse(x):
    m = x.max()
    if not np.isfinite(m):
        return m
    return m + np.log(np.exp(x - m).sum(dtype=x.dtype))


def sample_row(v, temperature, top_k=0, top_p=1.0, seed=0, draw=0, position=0, row_id=0, lo=None, hi=None,
               dtype=np.float64):
    """One row.  v: the N logits (bf16 values in any float array).  Returns a dict: token, thr (smallest kept value),
    kept (count), gap (difference of the two largest perturbed scores, inf when one column is kept), p_gap (distance of
    top_p from the cumulative mass at the chosen top-p threshold and at the one before it, inf without top-p), and what
    `logprobs` needs."""
    v64 = np.asarray(v, dtype=np.float64)
    N = v64.shape[0]
    a, b = (0, N) if lo is None else (max(int(lo), 0), min(int(hi), N))
    if a >= b:
        a, b = 0, N
    va = v64[a:b].astype(dtype)
    vall = v64.astype(dtype)
    n = b - a
    if np.isnan(va).any():
        return {"token": a + int(np.argmax(np.isnan(va))), "nan": True, "thr": np.nan, "kept": 0, "gap": np.inf,
                "p_gap": np.inf}
    T = dtype(np.float32(temperature))
    greedy = not (T > 0)
    invT = dtype(1.0) if greedy else dtype(1.0) / T
    vmax = va.max()
    w = np.where(va == vmax, dtype(1.0), np.exp((va - vmax) * invT))
    keep = np.ones(n, dtype=bool)
    p_gap = np.inf
    if not greedy:
        kk = int(top_k) if 0 < int(top_k) < n else n
        kth = np.partition(va, n - kk)[n - kk]
        keep = va >= kth
        p = dtype(np.float32(top_p))
        if p < 1:
            order = np.argsort(-va[keep], kind="stable")
            vs, ws = va[keep][order], w[keep][order]
            Z = ws.sum(dtype=dtype)
            cw = np.cumsum(ws, dtype=dtype)
            last = np.r_[vs[1:] != vs[:-1], True]  # cumulative mass at the end of each value class
            cum, cls = cw[last], vs[last]
            i = min(int(np.argmax(cum >= p * Z)) if (cum >= p * Z).any() else len(cum) - 1, len(cum) - 1)
            p_gap = min(abs(cum[i] / Z - p), abs(cum[i - 1] / Z - p) if i > 0 else np.inf)
            keep = va >= cls[i]
    zk = w[keep].sum(dtype=dtype)
    if greedy:
        tok = int(np.argmax(va))
        gap = np.inf
    else:
        s = va.astype(np.float64) / np.float64(np.float32(temperature)) + gumbel(np.arange(a, b), position, row_id,
                                                                                seed, draw)
        s = np.where(keep, s, -np.inf)
        tok = int(np.argmax(s))
        top2 = np.partition(s, n - 2)[n - 2:] if n > 1 else np.array([-np.inf, s[0]])
        gap = float(top2[1] - top2[0])
    return {"token": a + tok, "nan": False, "thr": float(va[keep].min()), "kept": int(keep.sum()), "gap": gap,
            "p_gap": float(p_gap), "keep": keep, "lo": a, "vmax": vmax, "invT": invT, "logz": np.log(zk),
            "lse_raw": _lse(vall), "dtype": dtype}


def logprobs(res, v, token):
    """(logprob, logprob_raw) of `token` under the row result `res` of sample_row(v, ...)."""
    if res["nan"]:
        return np.nan, np.nan
    dt = res["dtype"]
    vt = dt(np.asarray(v, dtype=np.float64)[token])
    return float((vt - res["vmax"]) * res["invT"] - res["logz"]), float(vt - res["lse_raw"])


def make_logits(rng, M, N, scale, cap=30.0):
    """bf16(cap tanh(x / cap)), x Gaussian of the given scale; returns a float32 array [M, N] of bf16 values."""
    import torch
    x = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32) * np.float32(scale))
    return (cap * torch.tanh(x / cap)).bfloat16().float().numpy()


def chi_square_top31(v, tokens, temperature=1.0):
    """Pearson statistic of `tokens` (draws from softmax(v / T)) over the 31 most probable columns plus "rest"
    (31 degrees of freedom)."""
    v = np.asarray(v, dtype=np.float64) / temperature
    p = np.exp(v - v.max())
    p /= p.sum()
    top = np.argsort(-p)[:31]
    cnt = np.bincount(np.asarray(tokens), minlength=v.shape[0]).astype(np.float64)
    n = float(len(tokens))
    obs = np.append(cnt[top], n - cnt[top].sum())
    exp = np.append(p[top], 1 - p[top].sum()) * n
    assert exp.min() >= 5.0
    return float(((obs - exp) ** 2 / exp).sum())


CHI2_31_Q = 83.6  # the 1 - 1e-6 quantile of chi-square with 31 degrees of freedom
