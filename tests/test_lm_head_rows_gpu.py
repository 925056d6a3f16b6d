"""The training step's lm_head over the rows that carry a label (LMHeadCEFn._forward_rows, TrainEngine.train_step).

Kernel level: svla_gather_rows_bf16 / svla_scatter_rows_bf16 against index_select / zeros + index_copy_, bit for bit
(R = 1 and an unsorted row list included), and the logits of gathered rows against the same rows of the full product
with both GEMMs forced onto the 4-wave kernel (variant 3) at [640, 1000 (ragged), 512], bit for bit: a row's k order
does not depend on which rows share its tile.

Model level (tiny preset, the model bound to a TrainEngine): forward + backward with the label-row head against the
full-logits head on the same weights and batch.  At 26 label rows against 624 the dispatcher may pick another tile
kernel for the projection, so the yardstick is the project's noise floor (tests/test_dp4b_gpu.py): the distance
between the full path under the default dispatch and under GEMM variant 2, x 2, per quantity; where the label-row
logits statistics come out bitwise equal (same kernel arithmetic), every gradient must be bitwise equal instead.
argmax on the label rows: identical wherever the full logits' top-1 / top-2 margin exceeds harness.MARGIN (the
suite's criterion for bf16 logits).  Off the label rows argmax is -1 and lse NaN; forward() called directly still
returns full logits."""
import pytest
import torch

import harness as H

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _r(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).to(BF)


@pytest.mark.parametrize("rows", [[5], [7, 0, 639, 3, 200, 201, 8], list(range(0, 640, 5))],
                         ids=["one", "unsorted", "sorted128"])
def test_gather_scatter_rows_bitwise(cuda, rows):
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(201)
    M, C = 640, 2304
    src = _r(M, C + 8)[:, :C]  # a row stride beyond the columns
    idx = torch.tensor(rows, dtype=torch.int64, device=cuda)
    got = torch.empty(len(rows), C, dtype=BF, device=cuda)
    Kn.gather_rows(idx, src, got)
    assert torch.equal(got, src.index_select(0, idx))
    back = torch.full((M, C), 7.0, dtype=BF, device=cuda)  # every row must be written
    Kn.scatter_rows(idx, got, back)
    assert torch.equal(back, torch.zeros(M, C, dtype=BF, device=cuda).index_copy_(0, idx, got))


def test_gathered_rows_logits_bitwise(cuda):
    from spatialvla_amd import kernels as Kn
    torch.manual_seed(202)
    M, N, Kd = 640, 1000, 512
    h, w = _r(M, Kd), _r(N, Kd, scale=0.05)
    idx = torch.tensor([3, 17, 18, 19, 255, 256, 300, 511, 512, 638, 639], dtype=torch.int64, device=cuda)
    h_r = torch.empty(idx.numel(), Kd, dtype=BF, device=cuda)
    Kn.gather_rows(idx, h, h_r)
    full = torch.empty(M, N, dtype=BF, device=cuda)
    part = torch.empty(idx.numel(), N, dtype=BF, device=cuda)
    try:
        Kn.gemm_variant = 3
        Kn.linear_fwd(h, [w], full)
        Kn.linear_fwd(h_r, [w], part)
    finally:
        Kn.gemm_variant = 0
    assert torch.equal(part, full.index_select(0, idx))
    assert H.rel_l2(full, h.float() @ w.float().T) < 5e-3


def _fwd_bwd(model, eng, batch, rows_only, variant):
    """One forward + backward of the engine-bound model; (loss, lse, argmax, logits, {name: gradient})."""
    from spatialvla_amd import kernels as Kn
    eng.flat_grad.zero_()
    try:
        Kn.gemm_variant = variant
        model.head_label_rows = rows_only
        out = model(**batch, return_dict=True)
        out.loss.backward()
    finally:
        Kn.gemm_variant = 0
        model.head_label_rows = False
    torch.cuda.synchronize()
    grads = {n: p._svla_grad.detach().float().clone() for n, p in model.named_parameters()
             if p.requires_grad and getattr(p, "_svla_grad", None) is not None}
    st = model.last_stash
    return out.loss.detach().float().clone(), st["lse"].clone(), st["argmax"].clone(), out.logits, grads


def _dist(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def test_train_step_label_rows_vs_full_logits(cuda):
    from spatialvla_amd import presets
    from spatialvla_amd.engine import TrainEngine
    cfgd = H.cfg_dict("tiny")
    b = H.batch_tensors(presets.synthetic_batch(cfgd, batch=2, seed=6), cuda)
    depth = torch.rand(2, 1, 224, 224, generator=torch.Generator().manual_seed(4)).mul(3).add(0.5).to(cuda)
    model = H.build_hip_model(cfgd, "cuda:0")
    model.train()
    model.vision_zoe_model.eval()
    model.predict_depth = lambda pv, _d=depth: _d
    eng = TrainEngine(model, lr=1e-3, warmup_ratio=0.0, total_steps=10, max_grad_norm=1.0)
    B, Lq = b["labels"].shape
    lab = (model._targets(b["labels"], b["attention_mask"], B, Lq, cuda) >= 0)
    R = int(lab.sum())
    assert 0 < R < B * Lq

    loss_f, lse_f, am_f, logits_f, g_f = _fwd_bwd(model, eng, b, False, 0)
    loss_2, lse_2, am_2, logits_2, g_2 = _fwd_bwd(model, eng, b, False, 2)
    loss_r, lse_r, am_r, logits_r, g_r = _fwd_bwd(model, eng, b, True, 0)

    assert logits_f is not None and tuple(logits_f.shape[:2]) == (B, Lq)
    assert logits_r is None
    assert lse_r.shape == lse_f.shape and am_r.shape == am_f.shape
    assert bool((am_r[~lab] == -1).all()) and bool(torch.isnan(lse_r[~lab]).all())
    assert g_r.keys() == g_f.keys() and len(g_f) > 0

    same = torch.equal(lse_r[lab], lse_f[lab])
    print(f"label rows {R} of {B * Lq}; lse bitwise equal: {same}")
    print(f"loss full {float(loss_f):.8f} variant2 {float(loss_2):.8f} rows {float(loss_r):.8f}")
    fl_lse, d_lse = _dist(lse_2[lab], lse_f[lab]), _dist(lse_r[lab], lse_f[lab])
    print(f"lse: floor {fl_lse:.3e} rows {d_lse:.3e}")
    worst = max(g_f, key=lambda n: _dist(g_r[n], g_f[n]) - 2 * _dist(g_2[n], g_f[n]))
    print(f"gradients: worst {worst}: floor {_dist(g_2[worst], g_f[worst]):.3e} rows {_dist(g_r[worst], g_f[worst]):.3e}")

    # argmax: the suite's criterion for bf16 logits (harness.MARGIN)
    top2 = logits_f.view(B * Lq, -1)[lab].float().topk(2, -1).values
    conf = (top2[:, 0] - top2[:, 1]) > H.MARGIN
    assert torch.equal(am_r[lab][conf], am_f[lab][conf])
    if same:
        # same kernel arithmetic on the label rows: the loss re-associates an R-term fp32 sum, nothing else moves
        assert torch.equal(am_r[lab], am_f[lab])
        row_loss_sum = float(loss_f.abs()) * R  # every row loss is positive: sum |row loss| = R * mean
        assert abs(float(loss_r) - float(loss_f)) <= (R - 1) * 2.0 ** -24 * row_loss_sum / R
        for n in g_f:
            assert torch.equal(g_r[n], g_f[n]), n
    else:
        assert d_lse <= 2 * fl_lse
        assert abs(float(loss_r) - float(loss_f)) <= 2 * abs(float(loss_2) - float(loss_f))
        for n in g_f:
            assert _dist(g_r[n], g_f[n]) <= 2 * _dist(g_2[n], g_f[n]), n

    # the engine's own step takes the label-row head and restores the option; forward() itself is unchanged
    loss_e = eng.train_step(b)
    torch.cuda.synchronize()
    assert torch.equal(loss_e.float(), loss_r)
    assert model.head_label_rows is False
    assert bool((model.last_stash["argmax"][~lab] == -1).all())
    with torch.no_grad():
        out = model(**b, return_dict=True)
    assert out.logits is not None and tuple(out.logits.shape[:2]) == (B, Lq)
