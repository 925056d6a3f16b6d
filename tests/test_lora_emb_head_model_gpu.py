"""The three new fine-tuning recipes end to end on the GPU (tiny preset, batch 2), in the pattern of
test_lora_vision_model_gpu.py: "spatialvla-linear" + modules_to_save (the spatial table trained in full), "spatialvla-
linear+emb" (the Embedding adapter on spatial_embed_tokens) and "spatialvla-linear+emb+h" (also lm_head), against the
CPU oracle patched by tests/lora_emb_head_ref.py (same bf16 adapter values on both sides, depth fed from the oracle):
parity with every adapter non-zero, the gradient set, the initial state, label-rows against full-rows loss,
TrainEngine steps, merge, and predict_action after the merge.  Measured figures go to lora_emb_head_tiny.json in the
parity directory before anything is asserted."""
import pytest
import torch

import harness as H
import lora_emb_head_ref as LE
from test_lora_vision_cpu import VISION_B_STD

pytestmark = pytest.mark.gpu
R, ALPHA, SEED, N_NEW = 8, 16.0, 7, 6
S = ALPHA / R
TABLE = "spatial_embed_tokens.weight"
# case -> (target set, modules_to_save, Embedding adapter, lm_head adapter, gradients: 58 + the table / + 2 (+ 2))
CASES = {"mts": ("spatialvla-linear", True, False, False, 59),
         "emb": ("spatialvla-linear+emb", False, True, False, 60),
         "emb_h": ("spatialvla-linear+emb+h", False, True, True, 62)}
_RECORDED = {}


def _record(case, **kv):
    from test_full4b_gpu import _dump
    _RECORDED.setdefault(case, {}).update(kv)
    _dump("lora_emb_head_tiny.json", _RECORDED)


def _hip_names(by_path, which):
    return {f"{p.replace('vision_tower.vision_model.', 'vision_tower.')}.lora.{which}": g for p, g in by_path.items()}


@pytest.fixture(scope="module")
def base(cuda):
    """The oracle, the batch and the no-adapter runs shared by every case, computed once and left unchanged."""
    from spatialvla_amd import presets
    cfgd = H.cfg_dict("tiny")
    bc = H.batch_tensors(presets.synthetic_batch(cfgd, batch=2, seed=SEED), "cpu")
    bd = {k: v.to(cuda) for k, v in bc.items()}
    P, zoe = H.build_oracle(cfgd)
    loss0, logits0, _, cap = H.run_oracle(P, zoe, cfgd, bc)
    depth = cap["depth"]
    b = dict(cfgd=cfgd, bc=bc, bd=bd, P=P, zoe=zoe, depth=depth, depth_dev=depth.to(cuda), base=(loss0, logits0))
    m = H.build_hip_model(cfgd, "cuda:0")
    b["hip_base"] = H.run_hip(m, bd, depth=depth)
    del m
    return b


def _model(base, case, adapters=None):
    name, mts = CASES[case][:2]
    m = H.build_hip_model(base["cfgd"], "cuda:0")
    m.predict_depth = lambda pv, _d=base["depth_dev"]: _d
    m.add_lora(R, ALPHA, target_modules=name, seed=0, modules_to_save=["spatial_embed_tokens"] if mts else None)
    if adapters is not None:
        LE.set_model_adapters(m, adapters)
    return m


@pytest.fixture(scope="module", params=list(CASES))
def ctx(request, base, cuda):
    import spatialvla_oracle as O
    case = request.param
    name, mts, emb, head, n_grads = CASES[case]
    P, zoe, cfgd, bc = base["P"], base["zoe"], base["cfgd"], base["bc"]
    ads = LE.make_adapters(P, cfgd, R, SEED, emb=emb, head=head, vision_b_std=VISION_B_STD)
    assert len(ads) == 29 + emb + head
    with LE.oracle_lora(P, ads, S, modules_to_save=mts):
        loss_r, logits_r, grads_r, _ = H.run_oracle(P, zoe, cfgd, bc, depth=base["depth"])
    ref_grads = {**_hip_names({p: a.grad.float() for p, (a, _) in ads.items()}, "A"),
                 **_hip_names({p: b.grad.float() for p, (_, b) in ads.items()}, "B")}
    if mts:
        ref_grads[TABLE] = grads_r[TABLE]
    assert len(ref_grads) == n_grads
    with torch.no_grad():
        _, logits_m = O.forward(LE.merged_params(P, ads, S), cfgd, bc, zoe, depth=base["depth"])
    c = dict(base, case=case, ads=ads, n_grads=n_grads, ref=(loss_r, logits_r.detach()), ref_grads=ref_grads,
             oracle_merge_dist=H.rel_l2(logits_m, logits_r))
    c["hip"] = H.run_hip(_model(base, case, ads), base["bd"])
    return c


def _trainable_name(n):
    return ".lora." in n or n == TABLE


def test_parity_vs_patched_oracle(ctx):
    """All adapters non-zero.  The project's rules for adapters: logits within 1.5 x the no-adapter model's rel-L2
    against the unpatched oracle in the same run, every gradient within harness.GRAD_TOL, loss within 1e-2; the
    adapters move the oracle's logits by more than 0.1 rel-L2, so a dropped term cannot pass."""
    case = ctx["case"]
    loss_h, logits_h, grads_h, am = ctx["hip"]
    loss_r, logits_r = ctx["ref"]
    base_rel = H.rel_l2(ctx["hip_base"][1], ctx["base"][1])
    res = H.compare(loss_h, logits_h, grads_h, am, loss_r, logits_r, ctx["ref_grads"], labels=ctx["bc"]["labels"])
    moved = H.rel_l2(logits_r, ctx["base"][1])
    new = {n: v for n, v in res["grad_rel"].items() if "spatial_embed" in n or "lm_head" in n}
    _record(case, logits_rel=res["logits_rel"], base_logits_rel=base_rel, loss_hip=res["loss_hip"],
            loss_ref=res["loss_ref"], grad_rel_max=res["grad_rel_max"], grad_rel=res["grad_rel"],
            adapters_vs_base_logits_rel=moved)
    print(f"lora emb/head parity [{case}]: logits rel {res['logits_rel']:.3e} (base {base_rel:.3e}), loss "
          f"{res['loss_hip']:.5f} vs {res['loss_ref']:.5f}, grads max {res['grad_rel_max']:.3e}, new sites {new}, "
          f"adapters vs base {moved:.3e}")
    assert moved > 0.1
    assert not res["grads_missing"] and len(res["grad_rel"]) == ctx["n_grads"]
    for n, v in res["grad_rel"].items():
        assert v <= H.GRAD_TOL, (n, v)
    assert len(grads_h) == ctx["n_grads"] and all(_trainable_name(n) for n in grads_h), \
        "no frozen parameter may have a gradient"
    assert abs(res["loss_hip"] - res["loss_ref"]) <= 1e-2
    assert res["logits_rel"] <= 1.5 * base_rel


def test_initial_state(ctx):
    """add_lora's own initialisation: the base function; the Embedding adapter's dA is not zero and its dB is (A = 0),
    the lm_head adapter's dB is not zero and its dA is (B = 0); under modules_to_save the table has a gradient."""
    case = ctx["case"]
    _, mts, emb, head, n_grads = CASES[case]
    m = _model(ctx, case)
    loss, _, grads, _ = H.run_hip(m, ctx["bd"])
    assert abs(float(loss) - float(ctx["hip_base"][0])) <= 1e-2
    assert len(grads) == n_grads and all(_trainable_name(n) for n in grads)
    if emb:
        assert float(grads["spatial_embed_tokens.lora.A"].abs().max()) > 0.0
        assert float(grads["spatial_embed_tokens.lora.B"].abs().max()) == 0.0
    if head:
        assert float(grads["language_model.lm_head.lora.B"].abs().max()) > 0.0
        assert float(grads["language_model.lm_head.lora.A"].abs().max()) == 0.0
    if mts:
        assert float(grads[TABLE].abs().max()) > 0.0
    # the training step's label-rows head: bitwise the full-rows loss
    m.zero_grad(set_to_none=True)
    m.head_label_rows = True
    try:
        out = m(**ctx["bd"], return_dict=True)
    finally:
        m.head_label_rows = False
    assert out.logits is None
    _record(case, loss_full_rows=float(loss), loss_label_rows=float(out.loss.detach()))
    assert torch.equal(out.loss.detach().float().cpu(), loss)


def test_label_rows_with_adapters(ctx):
    """The label-rows head with every adapter non-zero.  test_initial_state holds the two forms of the loss to the same
    bits.  Here too every label row's logits are the full product's bits (the adapter term of a row does not depend on
    which rows share its block), but the loss is an fp32 sum over 26 rows instead of 624 mostly-zero ones and the
    order of that sum differs -- measured on the MI355X: one fp32 ulp (4.8e-7 at a loss of 7.03) in the
    modules_to_save case, whose head runs no adapter code at all, and in the "+emb+h" case; identical bits in the
    "+emb" case.  Bound: a reordered fp32 sum of n terms is off by at most n 2^-24 relative, n = the label rows (a
    different tile kernel for the 26-row projection, tests/test_lm_head_rows_gpu.py, would show as ~1e-4 and fail).
    The gradients of the new sites: harness.GRAD_TOL against the full-rows run."""
    case = ctx["case"]
    m = _model(ctx, case, ctx["ads"])
    m.head_label_rows = True
    out = m(**ctx["bd"], return_dict=True)
    out.loss.backward()
    torch.cuda.synchronize()
    full = float(ctx["hip"][0])
    _record(case, loss_full_rows_adapters=full, loss_label_rows_adapters=float(out.loss.detach()))
    n_rows = int((ctx["bc"]["labels"][:, 1:] != -100).sum())
    assert out.logits is None and n_rows == 26
    assert abs(float(out.loss.detach()) - full) <= n_rows * 2.0 ** -24 * abs(full)
    grads = {n.replace("vision_tower.vision_model.", "vision_tower."): p.grad.float().cpu()
             for n, p in m.named_parameters() if p.grad is not None}
    assert grads.keys() == ctx["hip"][2].keys()
    for n in grads:
        if "lm_head" in n or "spatial_embed" in n:
            assert H.rel_l2(grads[n], ctx["hip"][2][n]) <= H.GRAD_TOL, n


def _engine_run(ctx):
    from spatialvla_amd.engine import TrainEngine
    m = _model(ctx, ctx["case"])
    m.train()
    m.vision_zoe_model.eval()
    base0 = {n: p.detach().clone() for n, p in m.named_parameters() if ".lora." not in n}
    eng = TrainEngine(m, lr=2e-3, warmup_ratio=0.0, total_steps=10, max_grad_norm=1.0)
    losses = torch.stack([eng.train_step(ctx["bd"]).clone() for _ in range(3)]).cpu()
    torch.cuda.synchronize()
    mts = CASES[ctx["case"]][1]
    for n, p in m.named_parameters():
        if ".lora." in n:
            continue
        if n == TABLE and mts:
            assert not torch.equal(p.detach(), base0[n]), "the table trains under modules_to_save"
        else:
            assert torch.equal(p.detach(), base0[n]), n
    return m, eng, losses, eng.full_master().cpu()


def test_train_engine(ctx):
    case = ctx["case"]
    m, eng, losses, master = _engine_run(ctx)
    trained = [p for n, p in m.named_parameters() if _trainable_name(n) and p.requires_grad]
    assert len(trained) == ctx["n_grads"] and len(eng.params) == ctx["n_grads"]
    assert {id(p) for p in eng.params} == {id(p) for p in trained}, "the flat buffers hold exactly the adapters " \
        "(plus the table under modules_to_save)"
    assert eng.flat_param.numel() == sum((p.numel() + 63) // 64 * 64 for p in trained)
    assert eng.master.numel() == eng.flat_param.numel()
    print(f"lora emb/head engine losses [{case}]", losses.tolist())
    _record(case, engine_losses=losses.tolist())
    assert float(losses[2]) < float(losses[0])
    _, _, losses2, master2 = _engine_run(ctx)
    assert torch.equal(losses, losses2) and torch.equal(master, master2)


def test_merge_and_predict(ctx):
    """merge_lora(): logits within 2 x the CPU oracle's own merged-versus-adapter distance (test_merge's yardstick),
    and predict_action of the merged model gives the tokens predict_action_uncached gave before the merge, under
    the suite's margin rule for greedy tokens (harness.greedy_tokens_agree, >= 8 of 12 steps)."""
    from test_lora_decode_model_gpu import _uncached_step_logits
    case = ctx["case"]
    name, mts, emb, head, _ = CASES[case]
    m = _model(ctx, case, ctx["ads"])
    bd = ctx["bd"]
    inputs = {"input_ids": bd["input_ids"][:, :-13], "pixel_values": bd["pixel_values"], "intrinsic": bd["intrinsic"]}
    with torch.no_grad():
        before = m(**bd, return_dict=True).logits.float().cpu()
    if emb:
        with pytest.raises(NotImplementedError, match=r"merge_lora\(\)"):
            m.predict_action(inputs, max_new_tokens=2, eos_token_id=-1)
        with pytest.raises(NotImplementedError, match=r"merge_lora\(\)"):
            m.enable_lora_decode()
    unc = m.predict_action_uncached(inputs, max_new_tokens=N_NEW, eos_token_id=-1)
    top2 = _uncached_step_logits(m, inputs, unc).topk(2, -1).values
    margins = top2[..., 0] - top2[..., 1]
    table0, head0 = m.spatial_embed_tokens.weight.detach().clone(), m.language_model.lm_head.weight.detach().clone()
    if mts:  # the unmerged decode of the "spatialvla-linear" set reads the trainable table in place
        m.enable_lora_decode()
        dec = m.predict_action(inputs, max_new_tokens=N_NEW, eos_token_id=-1)
        n_cmp, n_ok = H.greedy_tokens_agree(dec, unc, margins)
        _record(case, lora_decode_tokens_ok=[n_ok, n_cmp])
        assert n_ok >= 8
        m.enable_lora_decode(False)
    m.merge_lora()
    assert not m.has_lora and m.lora_targets is None and m.lora_modules_to_save == []
    assert not any(".lora." in n for n, _ in m.named_parameters())
    assert not any(p.requires_grad for p in m.parameters())
    assert torch.equal(table0, m.spatial_embed_tokens.weight) != emb  # folded exactly when it carried an adapter
    assert torch.equal(head0, m.language_model.lm_head.weight) != head
    with torch.no_grad():
        after = m(**bd, return_dict=True).logits.float().cpu()
    dist = H.rel_l2(after, before)
    tok = m.predict_action(inputs, max_new_tokens=N_NEW, eos_token_id=-1)
    n_cmp, n_ok = H.greedy_tokens_agree(tok, unc, margins)
    _record(case, merge_logits_rel=dist, oracle_merge_logits_rel=ctx["oracle_merge_dist"],
            tokens_uncached_before_merge=unc.tolist(), tokens_cached_after_merge=tok.tolist(), tokens_ok=[n_ok, n_cmp],
            margins=[[round(float(v), 3) for v in r] for r in margins])
    print(f"lora emb/head merge [{case}]: logits rel {dist:.3e}, oracle merged-vs-adapter "
          f"{ctx['oracle_merge_dist']:.3e}; tokens {tok.tolist()} vs {unc.tolist()}: {n_ok}/{n_cmp}")
    assert dist <= 2.0 * ctx["oracle_merge_dist"]
    assert tok.shape == (2, N_NEW) and n_ok >= 8
    m.clear_decode_cache()
