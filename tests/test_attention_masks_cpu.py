"""Discriminating power of the attention mask cases (torch only): every mask mutation that changes a case's mask must
move the float64 reference by at least 3x the kernels' tolerance on out, dq, dk and dv, else the GPU comparison of
tests/test_attention_masks_gpu.py would pass with that slip in a kernel."""
import pytest
import torch

import attn_mask_ref as R


@pytest.mark.parametrize("case", R.ALL_CASES, ids=repr)
def test_mutants_are_told_apart(case):
    d, ref, plan = R.prepared(case)  # mutant_plan raises when a mutant is within 3x the tolerance everywhere
    for m, (where, rows, dist) in plan.items():
        print(f"{case!r} {m}: {where} " + " ".join(f"{n}={v:.3f}" for n, v in dist.items()))
        assert all(dist[n] >= 3 * R.TOLS[n] for n in R.QUANT)
    if case.window > 0 and case.window < case.L - 1:
        assert "w+1" in plan and "w-1" in plan
    if case.lay != "none":
        assert "strict" in plan
    dead = R.dead_rows(case, d)
    if case.lay == "left-pad":  # rows 0..5 see nothing: exactly uniform, the mean of V over all L keys
        assert bool(dead[:, :6].all())
        v = d["v"].double().repeat_interleave(case.Hq // case.Hkv, 2).mean(1, keepdim=True).expand_as(ref["out"])
        assert R.rel(ref["out"][dead], v[dead]) < 1e-12


def test_reference_gradient_passes_the_mask():
    """On a fully masked row the pass-through mask hands the scores a gradient (as the additive mask does) where a
    torch.where mask blocks it: dq of such a row is non-zero."""
    case = R.CASES_B[0]
    d, ref, _ = R.prepared(case)
    dead = R.dead_rows(case, d)
    assert float(ref["dq"][dead].norm()) > 0


@pytest.mark.parametrize("ragged", [False, True])
def test_oracle_window16_differs_from_4096(ragged):
    """The model-level window runs of test_attention_masks_gpu.py prove something only if the window changes the
    oracle's result by more than the parity tolerance: loss and logits at sliding_window 16 against 4096, same
    weights, batch and depth, differ by more than 3x LOGITS_TOL."""
    import harness as H
    import spatialvla_oracle as O
    from spatialvla_amd import presets
    out = {}
    for w in (16, 4096):
        cfgd = H.apply_overrides(H.cfg_dict("tiny"), {"text_config": {"sliding_window": w}})
        bc = H.batch_tensors(presets.synthetic_batch(cfgd, batch=2, seed=R.MODEL_SEED, ragged=ragged), "cpu")
        with torch.no_grad():
            out[w] = O.forward(O.build_params(cfgd, H.SEED), cfgd, bc, None, depth=R.model_depth(), cap={})
    (l16, g16), (l4k, g4k) = out[16], out[4096]
    print(f"ragged={ragged}: loss {float(l16):.4f} vs {float(l4k):.4f}, logits rel_l2 {H.rel_l2(g16, g4k):.3f}")
    assert H.rel_l2(g16, g4k) > 3 * H.LOGITS_TOL
    assert abs(float(l16) - float(l4k)) > 3 * H.LOGITS_TOL
