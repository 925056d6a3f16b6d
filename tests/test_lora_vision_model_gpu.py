"""LoRA on the reference's default target set ("spatialvla-linear": Gemma2 + SigLIP + projector + Ego3D, 29 modules on
the tiny model) end to end on the GPU: against the CPU oracle patched by tests/lora_vision_ref.py (same bf16 adapter
values on both sides, depth fed from the oracle), the kernel path against the unfused composition, the initial state,
TrainEngine steps, merge, and the KV-cached decode with unmerged adapters.  Measured figures go to
lora_vision_tiny.json in the parity directory before anything is asserted."""
import pytest
import torch

import harness as H
import lora_vision_ref as LV
from test_lora_vision_cpu import VISION_B_STD

pytestmark = pytest.mark.gpu
R, ALPHA, SEED, N_NEW = 8, 16.0, 7, 6
S = ALPHA / R
N_AD = 58
_RECORDED = {}


def _record(**kv):
    from test_full4b_gpu import _dump
    _RECORDED.update(kv)
    _dump("lora_vision_tiny.json", _RECORDED)


def _lora_model(ctx, adapters=None):
    m = H.build_hip_model(ctx["cfgd"], "cuda:0")
    m.predict_depth = lambda pv, _d=ctx["depth_dev"]: _d  # device tensor: no host copy inside a graph capture
    m.add_lora(R, ALPHA, target_modules="spatialvla-linear", seed=0)
    if adapters is not None:
        LV.set_model_adapters(m, adapters)
    return m


def _hip_names(by_path, which):
    """Module path -> the name harness.run_hip reports the adapter gradient under."""
    return {f"{p.replace('vision_tower.vision_model.', 'vision_tower.')}.lora.{which}": g for p, g in by_path.items()}


@pytest.fixture(scope="module")
def ctx(cuda):
    """Oracle and model runs shared by the tests below, computed once and left unchanged."""
    import spatialvla_oracle as O
    from spatialvla_amd import functional as Fn, presets
    cfgd = H.cfg_dict("tiny")
    bc = H.batch_tensors(presets.synthetic_batch(cfgd, batch=2, seed=SEED), "cpu")
    bd = {k: v.to(cuda) for k, v in bc.items()}
    P, zoe = H.build_oracle(cfgd)
    loss0, logits0, _, cap = H.run_oracle(P, zoe, cfgd, bc)
    depth = cap["depth"]
    ads = LV.make_adapters(P, cfgd, R, SEED, vision_b_std=VISION_B_STD)
    assert len(ads) == N_AD // 2
    with LV.oracle_lora(P, ads, S):
        loss_r, logits_r, grads_r, _ = H.run_oracle(P, zoe, cfgd, bc, depth=depth)
    assert all(".lora" not in n for n in grads_r)
    gA = {p: a.grad.float() for p, (a, b) in ads.items()}
    gB = {p: b.grad.float() for p, (a, b) in ads.items()}
    with torch.no_grad():
        _, logits_m = O.forward(LV.merged_params(P, ads, S), cfgd, bc, zoe, depth=depth)
    c = dict(cfgd=cfgd, bc=bc, bd=bd, depth=depth, depth_dev=depth.to(cuda), ads=ads, base=(loss0, logits0),
             ref=(loss_r, logits_r.detach()), ref_grads={**_hip_names(gA, "A"), **_hip_names(gB, "B")},
             oracle_merge_dist=H.rel_l2(logits_m, logits_r))
    base = H.build_hip_model(cfgd, "cuda:0")
    c["hip_base"] = H.run_hip(base, bd, depth=depth)
    del base
    m = _lora_model(c, ads)
    c["hip"] = H.run_hip(m, bd)
    try:
        Fn.LORA_KERNELS[0] = False
        c["hip_composed"] = H.run_hip(m, bd)
    finally:
        Fn.LORA_KERNELS[0] = True
    return c


def test_parity_vs_patched_oracle(ctx):
    """Non-zero A and B on all 29 modules.  Logits bound: the project's rule for adapters -- 1.5 x the no-adapter
    model's rel-L2 against the unpatched oracle on the same batch (the base path's own bf16 error; the margin covers
    the two extra bf16 roundings per adapted linear, t and u)."""
    loss_h, logits_h, grads_h, am = ctx["hip"]
    loss_r, logits_r = ctx["ref"]
    base_rel = H.rel_l2(ctx["hip_base"][1], ctx["base"][1])
    composed_rel = H.rel_l2(ctx["hip_composed"][1], logits_r)
    res = H.compare(loss_h, logits_h, grads_h, am, loss_r, logits_r, ctx["ref_grads"], labels=ctx["bc"]["labels"])
    _record(logits_rel=res["logits_rel"], base_logits_rel=base_rel, composed_logits_rel=composed_rel,
            loss_hip=res["loss_hip"], loss_ref=res["loss_ref"], grad_rel_max=res["grad_rel_max"],
            grad_rel=res["grad_rel"], adapters_vs_base_logits_rel=H.rel_l2(logits_r, ctx["base"][1]))
    print(f"lora vision parity: logits rel {res['logits_rel']:.3e} (base {base_rel:.3e}, composition "
          f"{composed_rel:.3e}), loss {res['loss_hip']:.5f} vs {res['loss_ref']:.5f}, grads max "
          f"{res['grad_rel_max']:.3e}")
    assert H.rel_l2(logits_r, ctx["base"][1]) > 0.1  # the adapters matter: dropping one cannot pass
    assert not res["grads_missing"] and len(res["grad_rel"]) == N_AD
    for n, v in res["grad_rel"].items():
        assert v <= H.GRAD_TOL, (n, v)
    assert len(grads_h) == N_AD and all(".lora." in n for n in grads_h), "no base parameter may have a gradient"
    assert abs(res["loss_hip"] - res["loss_ref"]) <= 1e-2
    assert res["argmax_agree_confident"] == 1.0
    assert res["logits_rel"] <= 1.5 * base_rel


def test_kernels_vs_composition(ctx):
    _, logits_k, grads_k, _ = ctx["hip"]
    _, logits_c, grads_c, _ = ctx["hip_composed"]
    rel = H.rel_l2(logits_k, logits_c)
    grel = {n: H.rel_l2(grads_k[n], grads_c[n]) for n in grads_k if n in grads_c}
    _record(kernels_vs_composed_logits_rel=rel, kernels_vs_composed_grad_rel_max=max(grel.values()))
    assert rel < 5e-3
    assert grads_k.keys() == grads_c.keys() and len(grads_k) == N_AD
    for n, v in grel.items():
        assert v < 2e-2, (n, v)


def test_initial_state(ctx):
    """add_lora's own initialisation (B = 0): the model computes the base function, every dA is exactly zero and every
    dB is not -- the gradient reaches SigLIP layer 0, the projector and both Ego3D linears."""
    m = _lora_model(ctx)
    loss, _, grads, _ = H.run_hip(m, ctx["bd"])
    assert abs(float(loss) - float(ctx["hip_base"][0])) <= 1e-2
    assert len(grads) == N_AD
    for n, g in grads.items():
        if n.endswith(".A"):
            assert float(g.abs().max()) == 0.0, n
        else:
            assert float(g.abs().max()) > 0.0, n
    for key in ("vision_tower.encoder.layers.0.self_attn.q_proj.lora.B", "multi_modal_projector.linear.lora.B",
                "position_embedding_3d.position_embedding_head.0.lora.B",
                "position_embedding_3d.position_embedding_head.3.lora.B"):
        assert key in grads, key


def _engine_run(ctx):
    from spatialvla_amd.engine import TrainEngine
    m = _lora_model(ctx)
    m.train()
    m.vision_zoe_model.eval()
    base0 = {n: p.detach().clone() for n, p in m.named_parameters() if ".lora." not in n}
    eng = TrainEngine(m, lr=2e-3, warmup_ratio=0.0, total_steps=10, max_grad_norm=1.0)
    losses = torch.stack([eng.train_step(ctx["bd"]).clone() for _ in range(3)]).cpu()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        if ".lora." not in n:
            assert torch.equal(p.detach(), base0[n]), n
    return m, eng, losses, eng.full_master().cpu()


def test_train_engine(ctx):
    m, eng, losses, master = _engine_run(ctx)
    adapters = [p for n, p in m.named_parameters() if ".lora." in n]
    assert len(adapters) == N_AD and len(eng.params) == N_AD and all(p.requires_grad for p in adapters)
    assert {id(p) for p in eng.params} == {id(p) for p in adapters}
    assert eng.flat_param.numel() == sum((p.numel() + 63) // 64 * 64 for p in adapters)
    assert eng.master.numel() == eng.flat_param.numel()
    print("lora vision engine losses", losses.tolist())
    _record(engine_losses=losses.tolist())
    assert float(losses[2]) < float(losses[0])
    _, _, losses2, master2 = _engine_run(ctx)
    assert torch.equal(losses, losses2) and torch.equal(master, master2)


def test_merge(ctx):
    """merge_lora() on the full set: logits within 2 x the CPU oracle's own merged-versus-adapter distance, recomputed
    for the full set (the existing merge test's yardstick)."""
    m = _lora_model(ctx, ctx["ads"])
    with torch.no_grad():
        before = m(**ctx["bd"], return_dict=True).logits.float().cpu()
    h0 = m.position_embedding_3d.position_embedding_head[0]
    w0, wp0 = h0.weight.detach().clone(), m.multi_modal_projector.linear.weight.detach().clone()
    m.merge_lora()
    assert not m.has_lora and m.lora_targets is None
    assert not any(".lora." in n for n, _ in m.named_parameters())
    assert not any(hasattr(lin, "lora") for _, lin in m._lora_all_linears(True))
    assert h0.weight.shape == (144, 204) and not torch.equal(w0, h0.weight)
    assert not torch.equal(wp0, m.multi_modal_projector.linear.weight)
    with torch.no_grad():
        after = m(**ctx["bd"], return_dict=True).logits.float().cpu()
    dist = H.rel_l2(after, before)
    _record(merge_logits_rel=dist, oracle_merge_logits_rel=ctx["oracle_merge_dist"])
    print(f"lora vision merge: logits rel {dist:.3e}, oracle merged-vs-adapter {ctx['oracle_merge_dist']:.3e}")
    assert dist <= 2.0 * ctx["oracle_merge_dist"]


def test_lora_decode_full_set(ctx):
    """enable_lora_decode() with the full set: the prefill graph runs SigLIP / Ego3D / the projector through the LoRA
    Functions; cached greedy tokens against the uncached forward of the same unmerged model under the margin rule and
    the cap of test_lora_decode_model_gpu.py (harness.greedy_tokens_agree, >= 8 of 12 steps)."""
    from test_lora_decode_model_gpu import _uncached_step_logits
    m = _lora_model(ctx, ctx["ads"])
    bd = ctx["bd"]
    inputs = {"input_ids": bd["input_ids"][:, :-13], "pixel_values": bd["pixel_values"], "intrinsic": bd["intrinsic"]}
    with pytest.raises(RuntimeError, match=r"call merge_lora\(\) first"):
        m.predict_action(inputs, max_new_tokens=2, eos_token_id=-1)
    unc = m.predict_action_uncached(inputs, max_new_tokens=N_NEW, eos_token_id=-1)
    top2 = _uncached_step_logits(m, inputs, unc).topk(2, -1).values
    margins = top2[..., 0] - top2[..., 1]
    m.enable_lora_decode()
    m.decode_graphs = True
    first = m.predict_action(inputs, max_new_tokens=N_NEW, eos_token_id=-1)
    st = next(iter(m._svla_decode_states.values()))
    n_graphs, n_prefill = len(st["graphs"]), len(st["prefill"])
    assert n_graphs == N_NEW - 1 and all(g is not None for g in st["prefill"].values()), "the prefill was captured"
    assert st["wptr"][2][4] == m.multi_modal_projector.linear.lora.A.data_ptr()
    second = m.predict_action(inputs, max_new_tokens=N_NEW, eos_token_id=-1)
    assert next(iter(m._svla_decode_states.values())) is st
    assert len(st["graphs"]) == n_graphs and len(st["prefill"]) == n_prefill  # replayed, not re-captured
    m.decode_graphs = False
    eager = m.predict_action(inputs, max_new_tokens=N_NEW, eos_token_id=-1)
    n_cmp, n_ok = H.greedy_tokens_agree(first, unc, margins)
    _record(decode_tokens_uncached=unc.tolist(), decode_tokens_cached=first.tolist(), decode_tokens_ok=[n_ok, n_cmp],
            decode_margins=[[round(float(v), 3) for v in r] for r in margins])
    print(f"lora vision decode: cached {first.tolist()} vs uncached {unc.tolist()}: {n_ok}/{n_cmp}")
    assert first.shape == (2, N_NEW) and n_ok >= 8
    assert torch.equal(second, first) and torch.equal(eager, first)
    m.clear_decode_cache()
