"""Attention forward and backward at the mask edges (sliding window, key classes, fully masked rows) against the float64
reference of tests/attn_mask_ref.py, whose cases are built (and checked on the CPU, test_attention_masks_cpu.py) so
that an off-by-one on the window or the causal edge, a visible class-2 key or a window that skips the prefix keys moves
the reference by at least 3x the tolerances asserted here.  Also: the stored-dS workspace holding NaN patterns,
distinct leading dimensions with guard columns and rows, and the autograd plug-in."""
import ctypes
import math

import pytest
import torch

import attn_mask_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _flat(t):
    return t.reshape(t.shape[0] * t.shape[1], -1).contiguous()


def _kernel_inputs(case, d):
    """q / k reach the kernels rotated (RoPE is the QKV GEMM's epilogue, bf16)."""
    q, k = d["q"], d["k"]
    if case.rope:
        q, k = R.rope_bf16(q, d["cos"], d["sin"]), R.rope_bf16(k, d["cos"], d["sin"])
    return _flat(q), _flat(k), _flat(d["v"])


class _Run:
    """Forward once, then any number of backward calls (one per upstream gradient) through spatialvla_amd.kernels."""

    def __init__(self, Kn, case, d, q=None, k=None, v=None, out=None):
        self.Kn, self.c, self.d = Kn, case, d
        c = case
        if q is None:
            q, k, v = _kernel_inputs(c, d)
        self.q, self.k, self.v = q, k, v
        self.out = out if out is not None else torch.empty(c.B * c.L, c.Hq * c.D, dtype=BF, device=q.device)
        self.lse = torch.empty(c.B, c.Hq, c.L, device=q.device)
        Kn.attn_fwd(self.args(False), self.out, self.lse)

    def args(self, bwd):
        c, d = self.c, self.d
        return self.Kn.attn_args(c.B, c.L, c.Hq, c.Hkv, c.D, self.q, self.q.stride(0), self.k, self.k.stride(0), self.v,
                                 self.v.stride(0), c.scale, c.cap, d["cls"], c.window,
                                 d["cos"] if bwd else None, d["sin"] if bwd else None)

    def shaped(self, t, H):
        return t.reshape(self.c.B, self.c.L, H, self.c.D)

    def bwd(self, do, dq=None, dk=None, dv=None):
        c = self.c
        do = do if do.dim() == 2 else _flat(do)
        dq = dq if dq is not None else torch.empty(c.B * c.L, c.Hq * c.D, dtype=BF, device=do.device)
        dk = dk if dk is not None else torch.empty(c.B * c.L, c.Hkv * c.D, dtype=BF, device=do.device)
        dv = dv if dv is not None else torch.empty_like(dk)
        self.Kn.attn_bwd(self.args(True), self.out, do, self.lse, dq, dq.stride(0), dk, dk.stride(0), dv, dv.stride(0))
        torch.cuda.synchronize()
        return dict(dq=self.shaped(dq, c.Hq), dk=self.shaped(dk, c.Hkv), dv=self.shaped(dv, c.Hkv))


def _close(tag, got, ref, tol):
    e = R.rel(got, ref)
    print(f"  {tag}: rel_l2 {e:.3e} (< {tol:g})")
    assert math.isfinite(e) and e < tol, (tag, e, tol)


def _check_grads(tag, got, ref):
    for n in ("dq", "dk", "dv"):
        _close(f"{tag} {n}", got[n], ref[n], R.TOL_GRAD)


def _check_case(Kn, cuda, case):
    """The whole tensors against the reference, then every mutant the whole tensors cannot tell apart on the rows it
    changes (out on those rows; the gradients of dO zeroed outside them)."""
    d, ref, plan = R.prepared(case, cuda)
    run = _Run(Kn, case, d)
    print(f"{case!r}")
    out = run.shaped(run.out, case.Hq)
    _close("out", out, ref["out"], R.TOL_OUT)
    dead = R.dead_rows(case, d)
    live = ~dead[:, None, :].expand_as(ref["lse"])
    lse_ref = ref["lse"]
    if case.rope:  # the lse is the forward's, whose q / k are the bf16-rounded rotated rows: the exact lse of those
        q, k, v = _kernel_inputs(case, d)
        lse_ref = R.ref_attn(run.shaped(q, case.Hq), run.shaped(k, case.Hkv), d["v"], case.scale, case.cap,
                             case.vis(d))[1]
    _close("lse", run.lse[live], lse_ref[live], R.TOL_LSE)
    if case.cap and bool(dead.any()):  # the softcap path: L keys at 2^-120 each
        _close("lse of fully masked rows", run.lse[~live], torch.full_like(run.lse[~live], R.dead_lse_cap(case.L)),
               R.TOL_LSE)
    _check_grads("dO", run.bwd(d["do"]), ref)
    for m, (where, rows, _) in plan.items():
        if where != "rows":
            continue
        _close(f"[{m}] out on its rows", out[rows], ref["out"][rows], R.TOL_OUT)
        do = d["do"] * R.row_mask(rows, d["do"])
        _check_grads(f"[{m}] dO on its rows", run.bwd(do), case.reference(d, None, do))


def _paths(cases):
    """(case, stored-dS?) pairs: both backward paths at head_dim 256, the recomputing one (the only one) at 72."""
    return [pytest.param(c, ds, id=f"{c!r}-{'storedS' if ds else 'recompute'}")
            for c in cases for ds in ((True, False) if c.D == 256 else (False,))]


def _both_paths(Kn, ds, fn):
    Kn.ATTN_DS[0] = ds
    try:
        return fn()
    finally:
        Kn.ATTN_DS[0] = True


# ------------------------------------------------------------------------------------------------ A, C
@pytest.mark.parametrize("ds", [True, False], ids=["storedS", "recompute"])
@pytest.mark.parametrize("case", R.CASES_A, ids=repr)
def test_backward_window_d256(cuda, case, ds):
    """Case A: head_dim 256 forward and backward under a sliding window, through the stored-dS backward
    (svla_attn_bwd_ds) and the recomputing one (svla_attn_bwd): out, lse, dq, dk, dv."""
    from spatialvla_amd import kernels as Kn
    _both_paths(Kn, ds, lambda: _check_case(Kn, cuda, case))


@pytest.mark.parametrize("case", R.CASES_C, ids=repr)
def test_window_and_classes_d72(cuda, case):
    """Case C: the head_dim-72 kernels accept key classes and a window; they must then compute them."""
    from spatialvla_amd import kernels as Kn
    _check_case(Kn, cuda, case)


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("case,ds", _paths(R.CASES_B))
def test_fully_masked_rows(cuda, case, ds):
    """Case B: query rows with no visible key (left padding: the query's own key is class 2, nothing else in reach)
    are uniform over all L keys, forward and backward, compared on their own: 6 or 7 rows of 140 vanish in the norm of
    the whole tensor.  Forward: out on those rows is the mean of V over all keys.  Backward: dO zeroed everywhere
    else, so dq, dk and dv come from those rows alone.
    Without a softcap the backward used exp2(MASKVAL - lse2) for the row's p, with lse2 = MASKVAL + log2(L) rounded to
    MASKVAL in fp32 (or one ulp off it): 1, 0 or inf where the row's p is 1/L."""
    from spatialvla_amd import kernels as Kn
    d, ref, _ = R.prepared(case, cuda)
    dead = R.dead_rows(case, d)
    assert int(dead.sum()) == 13  # rows 0..6 of the first sequence, 0..5 of the second
    do = d["do"] * R.row_mask(dead, d["do"])
    want = case.reference(d, None, do)

    def go():
        print(f"{case!r}")
        run = _Run(Kn, case, d)
        out = run.shaped(run.out, case.Hq)
        meanv = d["v"].double().repeat_interleave(case.Hq // case.Hkv, 2).mean(1, keepdim=True).expand_as(ref["out"])
        _close("out of fully masked rows vs mean(V)", out[dead], meanv[dead], R.TOL_OUT)
        _close("out of fully masked rows", out[dead], ref["out"][dead], R.TOL_OUT)
        got = run.bwd(do)
        for n in ("dq", "dk", "dv"):
            print(f"  {n}: |kernel| / |reference| = {float(got[n].double().norm() / want[n].norm()):.4g}")
        _check_grads("dO on fully masked rows", got, want)
    _both_paths(Kn, ds, go)


# ------------------------------------------------------------------------------------------------ D
def _bwd_ds_direct(run, do, fill):
    """svla_attn_bwd_ds on a workspace of exactly svla_attn_bwd_ds_workspace_bytes, 256-B aligned, pre-filled (with
    a 4 KiB guard behind it) with the 16-bit pattern `fill`; returns the gradients and the guard."""
    from spatialvla_amd import _lib
    c = run.c
    lib = _lib.lib()
    n = int(lib.svla_attn_bwd_ds_workspace_bytes(c.B, c.L, c.Hq))
    assert n % 2 == 0
    guard = 4096
    buf = torch.empty((n + guard + 256) // 2, dtype=torch.int16, device=do.device)
    off = (-buf.data_ptr()) % 256
    assert off % 2 == 0
    buf.fill_(fill)
    do = _flat(do)
    dq = torch.empty(c.B * c.L, c.Hq * c.D, dtype=BF, device=do.device)
    dk = torch.empty(c.B * c.L, c.Hkv * c.D, dtype=BF, device=do.device)
    dv = torch.empty_like(dk)
    a = run.args(True)
    _lib.check(lib.svla_attn_bwd_ds(ctypes.byref(a), run.out.data_ptr(), run.out.stride(0), do.data_ptr(), do.stride(0),
                                    run.lse.data_ptr(), dq.data_ptr(), dq.stride(0), dk.data_ptr(), dk.stride(0),
                                    dv.data_ptr(), dv.stride(0), buf.data_ptr() + off, n,
                                    torch.cuda.current_stream().cuda_stream), "attn_bwd_ds")
    torch.cuda.synchronize()
    g = buf[(off + n) // 2:(off + n + guard) // 2]
    return dict(dq=run.shaped(dq, c.Hq), dk=run.shaped(dk, c.Hkv), dv=run.shaped(dv, c.Hkv)), g


@pytest.mark.parametrize("case", R.CASES_D, ids=repr)
def test_stored_ds_workspace_poisoned(cuda, case):
    """Case D: the dK/dV kernel leaves the dS^T columns round32(L)..round64(L)-1 unwritten when L % 64 is 1..32, and
    kernels.attn_bwd hands it torch.empty memory.  Whatever the workspace held (bf16 NaN, bytes 0xFF), the results
    are finite, bitwise those of a zeroed workspace and within tolerance of the reference; nothing is written past
    svla_attn_bwd_ds_workspace_bytes."""
    from spatialvla_amd import kernels as Kn
    d, ref, _ = R.prepared(case, cuda)
    run = _Run(Kn, case, d)
    zero, g0 = _bwd_ds_direct(run, d["do"], 0)
    assert bool((g0 == 0).all())
    print(f"{case!r}")
    _check_grads("zeroed workspace", zero, ref)
    for fill in (0x7FC0, -1):  # bf16 NaN; bytes 0xFF (a negative bf16 NaN)
        got, g = _bwd_ds_direct(run, d["do"], fill)
        assert bool((g == fill).all()), f"guard behind the workspace overwritten (fill {fill:#x})"
        for n in ("dq", "dk", "dv"):
            assert bool(torch.isfinite(got[n]).all()), (n, fill)
            assert torch.equal(got[n], zero[n]), (n, fill)


# ------------------------------------------------------------------------------------------------ E
def _wide(rows, cols, left, right, extra, fill, device):
    """A [rows + extra, left + cols + right] bf16 buffer of `fill` and its [rows, cols] window."""
    buf = torch.full((rows + extra, left + cols + right), fill, dtype=BF, device=device)
    return buf, buf[:rows, left:left + cols]


def _outside_is(buf, rows, left, cols, fill):
    m = torch.ones_like(buf, dtype=torch.bool)
    m[:rows, left:left + cols] = False
    return bool((buf[m] == fill).all())


@pytest.mark.parametrize("case,ds", _paths(R.CASES_E))
def test_leading_dimensions_and_stray_writes(cuda, case, ds):
    """Case E: q, k, v in three tensors of different row strides (NaN in their padding: nothing outside the head
    columns may be read into a result), out / dO / dq / dk / dv in wider buffers of 7.0 with 3 rows behind B*L: the
    results meet the reference and every element outside the [B*L, H*D] windows is still 7.0."""
    from spatialvla_amd import kernels as Kn
    d, ref, _ = R.prepared(case, cuda)
    c, n = case, case.B * case.L
    nq, nk = c.Hq * c.D, c.Hkv * c.D
    nan = float("nan")
    geo = dict(q=(nq, 8, 0), k=(nk, 16, 0), v=(nk, 0, 24), out=(nq, 8, 24), do=(nq, 16, 24), dq=(nq, 24, 24),
               dk=(nk, 24, 32), dv=(nk, 32, 32))  # (columns, padding left, padding right)
    bufs, win = {}, {}
    for name, (cols, left, right) in geo.items():
        bufs[name], win[name] = _wide(n, cols, left, right, 3, nan if name in "qkv" else 7.0, cuda)
    for name, t in zip("qkv", _kernel_inputs(case, d)):
        win[name].copy_(t)
    win["do"].copy_(_flat(d["do"]))
    assert len({win[x].stride(0) - geo[x][0] for x in geo}) == 8 and len({win[x].stride(0) for x in "qkv"}) == 3

    def go():
        run = _Run(Kn, case, d, win["q"], win["k"], win["v"], win["out"])
        got = run.bwd(win["do"], win["dq"], win["dk"], win["dv"])
        print(f"{case!r}")
        _close("out", run.shaped(run.out, c.Hq), ref["out"], R.TOL_OUT)
        _check_grads("dO", got, ref)
        for name in ("out", "do", "dq", "dk", "dv"):
            cols, left, _ = geo[name]
            assert _outside_is(bufs[name], n, left, cols, 7.0), f"{name}: written outside its [B*L, H*D] window"
    _both_paths(Kn, ds, go)


# ------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("case", R.CASES_F, ids=repr)
def test_plugin_window_and_softcap0(cuda, case):
    """Case F: functional.hip_attention through autograd: the window (and softcap 0 with fully masked rows) reach
    the forward and, through ctx.meta, the backward."""
    from spatialvla_amd.functional import hip_attention
    d, ref, _ = R.prepared(case, cuda)
    q, k, v = (d[n].transpose(1, 2).detach().clone().requires_grad_(True) for n in "qkv")
    out = hip_attention(q, k, v, case.scale, case.cap, d["cls"], case.window)
    assert out.shape == (case.B, case.L, case.Hq, case.D)
    out.backward(d["do"])
    torch.cuda.synchronize()
    print(f"{case!r}")
    _close("out", out, ref["out"], R.TOL_OUT)
    _check_grads("dO", dict(dq=q.grad.transpose(1, 2), dk=k.grad.transpose(1, 2), dv=v.grad.transpose(1, 2)), ref)
    dead = R.dead_rows(case, d)
    if bool(dead.any()):  # the fully masked rows on their own
        do = d["do"] * R.row_mask(dead, d["do"])
        q.grad = k.grad = v.grad = None
        hip_attention(q, k, v, case.scale, case.cap, d["cls"], case.window).backward(do)
        _check_grads("dO on fully masked rows",
                     dict(dq=q.grad.transpose(1, 2), dk=k.grad.transpose(1, 2), dv=v.grad.transpose(1, 2)),
                     case.reference(d, None, do))


# ------------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize("ragged", [False, True])
def test_tiny_vs_oracle_window16(cuda, ragged):
    """Training forward + backward of the tiny model with sliding_window 16 (the sliding layer's mask bites: which
    layers slide, how cfg.window reaches the attention arguments forward and backward, window x kv_class) against the
    CPU oracle; test_attention_masks_cpu.py asserts that window 16 moves the oracle by more than these tolerances."""
    import harness as H
    res = H.tiny_parity_run("cuda:0", batch=2, seed=R.MODEL_SEED, ragged=ragged, overrides=R.WINDOW16,
                            depth=R.model_depth())
    print({k: v for k, v in res.items() if k != "grad_rel"})
    assert not res["grads_missing"]
    assert abs(res["loss_hip"] - res["loss_ref"]) < 2e-2 * max(1.0, abs(res["loss_ref"]))
    assert res["logits_rel"] < H.LOGITS_TOL
    assert res["grad_rel_max"] < H.GRAD_TOL
    assert res["argmax_agree_confident"] == 1.0


def test_predict_action_cached_equals_uncached_window16(cuda):
    """Greedy tokens of the KV-cached decode equal those of full re-forwards with sliding_window 16 < Lk: the prefill
    and the decode attention kernels apply the window inside the model (eager steps and captured graphs)."""
    import os
    from safetensors.torch import load_file
    import harness as H
    g = load_file(os.path.join(os.path.dirname(__file__), "golden", "tiny_train.safetensors"))
    depth = g["out.depth"].to(cuda)
    inputs = {"input_ids": g["in.input_ids"][:, :-13], "pixel_values": g["in.pixel_values"],
              "intrinsic": g["in.intrinsic"]}
    toks = {}
    for w in (16, 4096):
        model = H.build_hip_model(H.apply_overrides(H.cfg_dict("tiny"), {"text_config": {"sliding_window": w}}), "cuda:0")
        model.predict_depth = lambda p: depth[:p.shape[0]]
        model.decode_graphs = False
        toks[w] = model.predict_action(inputs, max_new_tokens=8, eos_token_id=-1)
        if w == 16:
            full = model.predict_action_uncached(inputs, max_new_tokens=8, eos_token_id=-1)
            assert toks[w].shape == (2, 8)
            assert torch.equal(toks[w], full), (toks[w], full)
            model.decode_graphs = True
            g1 = model.predict_action(inputs, max_new_tokens=8, eos_token_id=-1)
            g2 = model.predict_action(inputs, max_new_tokens=8, eos_token_id=-1)
            assert torch.equal(g1, full) and torch.equal(g2, full)
    assert not torch.equal(toks[16], toks[4096]), "the window changed no greedy token: the run proves nothing"
