"""LoRA fine-tuning end to end on the GPU: the tiny model with adapters on the seven Gemma2 projections against the CPU
oracle patched by tests/lora_ref.py (same bf16 adapter values on both sides, depth fed from the oracle as
harness.tiny_parity_run does), the kernel path against the unfused composition, TrainEngine steps, merge, adapter
files and guards, and one decoder layer at the 4B widths."""
import json

import pytest
import torch

import harness as H
import lora_ref as LR

pytestmark = pytest.mark.gpu
R, ALPHA, SEED = 8, 16.0, 7
S = ALPHA / R
_RECORDED = {}


def _record(**kv):
    """The measured figures, written before anything is asserted, to lora_tiny.json in the parity directory the 4B
    parity tests use ($SVLA_PARITY_DIR or their default)."""
    from test_full4b_gpu import _dump
    _RECORDED.update(kv)
    _dump("lora_tiny.json", _RECORDED)


def _lora_model(ctx, adapters=None):
    m = H.build_hip_model(ctx["cfgd"], "cuda:0")
    m.predict_depth = lambda pv, _d=ctx["depth_dev"]: _d  # device tensor: no host copy inside a graph capture
    m.add_lora(R, ALPHA, seed=0)
    if adapters is not None:
        LR.set_model_adapters(m, adapters)
    return m


def _hip_names(grads_by_path, which):
    return {f"{p}.lora.{which}": g for p, g in grads_by_path.items()}


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
    ads = LR.make_adapters(P, cfgd, R, SEED)
    with LR.oracle_lora(P, ads, S):
        loss_r, logits_r, grads_r, _ = H.run_oracle(P, zoe, cfgd, bc, depth=depth)
    gA = {p: a.grad.float() for p, (a, b) in ads.items()}
    gB = {p: b.grad.float() for p, (a, b) in ads.items()}
    with torch.no_grad():
        _, logits_m = O.forward(LR.merged_params(P, ads, S), cfgd, bc, zoe, depth=depth)
    c = dict(cfgd=cfgd, bc=bc, bd=bd, depth=depth, depth_dev=depth.to(cuda), ads=ads, base=(loss0, logits0),
             ref=(loss_r, logits_r.detach()),
             ref_grads={**_hip_names(gA, "A"), **_hip_names(gB, "B")},
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


def test_lora_parity_vs_patched_oracle(ctx):
    """Non-zero A and B.  Logits bound: 1.5 x the no-adapter model's rel-L2 against the unpatched oracle on the same
    batch (the base path's own bf16 error; the margin covers the two extra bf16 roundings per projection, t and u)."""
    loss_h, logits_h, grads_h, am = ctx["hip"]
    loss_r, logits_r = ctx["ref"]
    base_rel = H.rel_l2(ctx["hip_base"][1], ctx["base"][1])
    res = H.compare(loss_h, logits_h, grads_h, am, loss_r, logits_r, ctx["ref_grads"], labels=ctx["bc"]["labels"])
    _record(logits_rel=res["logits_rel"], base_logits_rel=base_rel, loss_hip=res["loss_hip"], loss_ref=res["loss_ref"],
            grad_rel_max=res["grad_rel_max"], grad_rel=res["grad_rel"])
    print(f"lora parity: logits rel {res['logits_rel']:.3e} (base {base_rel:.3e}), loss {res['loss_hip']:.5f} vs "
          f"{res['loss_ref']:.5f}, grads max {res['grad_rel_max']:.3e}")
    assert H.rel_l2(logits_r, ctx["base"][1]) > 0.1  # the adapters matter: dropping one cannot pass
    assert abs(res["loss_hip"] - res["loss_ref"]) <= 1e-2
    assert res["logits_rel"] <= 1.5 * base_rel
    assert not res["grads_missing"] and len(res["grad_rel"]) == 28
    for n, v in res["grad_rel"].items():
        assert v <= H.GRAD_TOL, (n, v)
    assert all(".lora." in n for n in grads_h), "no base parameter may have a gradient"
    assert res["argmax_agree_confident"] == 1.0


def test_lora_kernels_vs_composition(ctx):
    _, logits_k, grads_k, _ = ctx["hip"]
    _, logits_c, grads_c, _ = ctx["hip_composed"]
    assert H.rel_l2(logits_k, logits_c) < 5e-3
    assert grads_k.keys() == grads_c.keys() and len(grads_k) == 28
    for n in grads_k:
        assert H.rel_l2(grads_k[n], grads_c[n]) < 2e-2, n


def test_lora_initial_state(ctx):
    """add_lora's own initialisation (B = 0): the model computes the base function, every dA is exactly zero and
    every dB is not."""
    m = _lora_model(ctx)
    loss, _, grads, _ = H.run_hip(m, ctx["bd"])
    assert abs(float(loss) - float(ctx["hip_base"][0])) <= 1e-2
    assert len(grads) == 28
    for n, g in grads.items():
        if n.endswith(".A"):
            assert float(g.abs().max()) == 0.0, n
        else:
            assert float(g.abs().max()) > 0.0, n


def _engine_run(ctx, ckpt):
    from spatialvla_amd.engine import TrainEngine
    m = _lora_model(ctx)
    m.train()
    m.vision_zoe_model.eval()
    if ckpt:
        m.language_model._set_gradient_checkpointing()
    base0 = {n: p.detach().clone() for n, p in m.named_parameters() if ".lora." not in n}
    eng = TrainEngine(m, lr=2e-3, warmup_ratio=0.0, total_steps=10, max_grad_norm=1.0)
    losses = torch.stack([eng.train_step(ctx["bd"]).clone() for _ in range(3)]).cpu()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        if ".lora." not in n:
            assert torch.equal(p.detach(), base0[n]), n
    return m, eng, losses, eng.full_master().cpu()


def test_lora_train_engine(ctx):
    m, eng, losses, master = _engine_run(ctx, False)
    adapters = [p for n, p in m.named_parameters() if ".lora." in n]
    assert len(eng.params) == 28 and all(p.requires_grad for p in adapters)
    assert eng.flat_param.numel() == sum((p.numel() + 63) // 64 * 64 for p in adapters)
    assert eng.master.numel() == eng.flat_param.numel()
    print("lora engine losses", losses.tolist())
    assert float(losses[2]) < float(losses[0])
    _, _, losses2, master2 = _engine_run(ctx, False)
    assert torch.equal(losses, losses2) and torch.equal(master, master2)
    _, _, losses3, master3 = _engine_run(ctx, True)
    assert torch.equal(losses, losses3) and torch.equal(master, master3)


def _prompt_inputs(ctx):
    bd = ctx["bd"]
    return {"input_ids": bd["input_ids"][:, :-13], "pixel_values": bd["pixel_values"], "intrinsic": bd["intrinsic"]}


def test_lora_merge(ctx):
    """merge_lora(): logits within 2 x the CPU oracle's own merged-versus-adapter distance (both sides carry
    independent bf16 noise: sqrt(2) plus headroom); afterwards the cached decode runs and agrees with the uncached."""
    m = _lora_model(ctx, ctx["ads"])
    inputs = _prompt_inputs(ctx)
    with torch.no_grad():
        before = m(**ctx["bd"], return_dict=True).logits.float().cpu()
    with pytest.raises(RuntimeError, match=r"call merge_lora\(\) first"):
        m.predict_action(inputs, max_new_tokens=2, eos_token_id=-1)
    unc_adapters = m.predict_action_uncached(inputs, max_new_tokens=2, eos_token_id=-1)
    assert unc_adapters.shape == (2, 2)
    w0 = m.language_model.model.layers[0].mlp.down_proj.weight.detach().clone()
    m.merge_lora()
    assert not m.has_lora and not any(".lora." in n for n, _ in m.named_parameters())
    assert not torch.equal(w0, m.language_model.model.layers[0].mlp.down_proj.weight)
    with torch.no_grad():
        after = m(**ctx["bd"], return_dict=True).logits.float().cpu()
    dist = H.rel_l2(after, before)
    _record(merge_logits_rel=dist, oracle_merge_logits_rel=ctx["oracle_merge_dist"])
    print(f"lora merge: logits rel {dist:.3e}, oracle merged-vs-adapter {ctx['oracle_merge_dist']:.3e}")
    assert dist <= 2.0 * ctx["oracle_merge_dist"]
    cached = m.predict_action(inputs, max_new_tokens=3, eos_token_id=-1)
    uncached = m.predict_action_uncached(inputs, max_new_tokens=3, eos_token_id=-1)
    assert torch.equal(cached, uncached)


def test_lora_io_and_guards(ctx, tmp_path):
    m = _lora_model(ctx, ctx["ads"])
    with torch.no_grad():
        a = m(**ctx["bd"], return_dict=True).logits.clone()
    m.save_lora(str(tmp_path))
    m2 = H.build_hip_model(ctx["cfgd"], "cuda:0")
    m2.predict_depth = m.predict_depth
    m2.load_lora(str(tmp_path))
    with torch.no_grad():
        b = m2(**ctx["bd"], return_dict=True).logits
    assert torch.equal(a, b)
    with pytest.raises(NotImplementedError):
        m2.enable_fp8_projections(True)
    m3 = H.build_hip_model(ctx["cfgd"], "cuda:0")
    m3.enable_fp8_projections(True)
    with pytest.raises(NotImplementedError):
        m3.add_lora(R, ALPHA)
    with pytest.raises(RuntimeError, match=r"call merge_lora\(\) first"):
        m2.generate(input_ids=ctx["bd"]["input_ids"][:, :-13], max_new_tokens=1)
    with pytest.raises(RuntimeError, match=r"call merge_lora\(\) first"):
        with torch.no_grad():
            m2(input_ids=ctx["bd"]["input_ids"], past_key_values=m2.new_cache(2, 400))


def test_lora_layer_4b_width_kernels_vs_composition(cuda):
    """One Gemma2 layer at hidden 2304 / I 9216 / D 256 with 2 x 312 rows and r = 32: the only place the real column
    counts run (4096, 18432 and the 2048 | 1024 | 1024 slices); kernel path against the composition path."""
    from spatialvla_amd import SpatialVLAConfig, functional as Fn, presets
    from spatialvla_amd.modeling_gemma2 import Gemma2DecoderLayer, KVMask, LoRAAdapter
    torch.manual_seed(11)
    cfg = SpatialVLAConfig(**json.loads(json.dumps(presets.spatialvla_4b(use_vision_zoe=False))))
    layer = Gemma2DecoderLayer(cfg.text_config, 1).to(torch.bfloat16).to(cuda)
    r, B, L = 32, 2, 312
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if p.dim() == 2:
                p.normal_(0, 0.02)
            else:
                p.normal_(0, 0.1)
            p.requires_grad_(False)
        for sub, names in ((layer.self_attn, ("q_proj", "k_proj", "v_proj", "o_proj")),
                           (layer.mlp, ("gate_proj", "up_proj", "down_proj"))):
            for n in names:
                lin = getattr(sub, n)
                A = (torch.randn(r, lin.in_features, device=cuda) / r).to(torch.bfloat16)
                Bm = (torch.randn(lin.out_features, r, device=cuda) * 0.02).to(torch.bfloat16)
                lin.lora = LoRAAdapter(A, Bm, r, 32.0)
    h0 = torch.randn(B, L, 2304, device=cuda).to(torch.bfloat16)
    gout = torch.randn(B, L, 2304, device=cuda).to(torch.bfloat16)
    cls = torch.ones(B, L, dtype=torch.uint8, device=cuda)
    cls[:, :299] = 0
    rope = layer.self_attn.rotary_emb.tables((torch.arange(L, device=cuda) + 1)[None], torch.bfloat16)

    def run():
        layer.zero_grad(set_to_none=True)
        h = h0.clone().requires_grad_(True)
        y = layer(h, KVMask(cls), rope)
        (y.float() * gout.float()).sum().backward()
        torch.cuda.synchronize()
        return y.detach(), h.grad.detach(), {n: p.grad.detach().clone() for n, p in layer.named_parameters()
                                             if p.grad is not None}

    yk, dxk, gk = run()
    try:
        Fn.LORA_KERNELS[0] = False
        yc, dxc, gc = run()
    finally:
        Fn.LORA_KERNELS[0] = True
    assert H.rel_l2(yk, yc) < 5e-3
    assert H.rel_l2(dxk, dxc) < 2e-2
    assert len(gk) == 14 and gk.keys() == gc.keys()
    for n in gk:
        assert H.rel_l2(gk[n], gc[n]) < 2e-2, n


def test_lora_single_adapter_dispatch(cuda):
    """What ships for the products of a single adapter (functional._LoraKernelOps): t = x A^T on the library GEMM, dA
    on the GEMM from 8192 columns on and on svla_lora_wgrad below -- each bitwise the kernel it names and within the
    product bound of the fp32 reference; several adapters always take the rank-r kernels."""
    from spatialvla_amd import functional as Fn, kernels as Kn
    torch.manual_seed(3)
    ops, r, M = Fn._LoraKernelOps, 32, 200
    bf = torch.bfloat16
    x = torch.randn(M, 320, device=cuda).to(bf)
    As = [(torch.randn(r, 320, device=cuda) / r).to(bf) for _ in range(3)]
    t1 = ops.down(x, As[:1], r)
    ref = torch.empty(M, r, dtype=bf, device=cuda)
    Kn.linear_fwd(x, As[:1], ref)
    assert torch.equal(t1, ref) and H.rel_l2(t1, x.float() @ As[0].float().T) < 5e-3
    t3 = ops.down(x, As, r)
    ref3 = torch.empty(M, 3 * r, dtype=bf, device=cuda)
    Kn.lora_down(x, As, r, ref3)
    assert torch.equal(t3, ref3)
    dt = torch.randn(M, r, device=cuda).to(bf)
    for W, gemm in ((ops.WGRAD_GEMM_MIN_COLS, True), (ops.WGRAD_GEMM_MIN_COLS - 128, False)):
        y = torch.randn(M, W, device=cuda).to(bf)
        g = torch.full((r, W), float("nan"), dtype=bf, device=cuda)
        ops.wgrad(y, dt, [(g, False, None)], r, False, 1.0, [0, W])
        ref = torch.empty(r, W, dtype=bf, device=cuda)
        if gemm:
            Kn.linear_wgrad(dt, y, [ref])
        else:
            Kn.lora_wgrad(y, dt, [ref], r)
        torch.cuda.synchronize()
        assert torch.equal(g, ref), W
        assert H.rel_l2(g, dt.float().T @ y.float()) < 5e-3
