"""enable_fp8_lora() end to end on the GPU: the tiny model (hidden 256, I 512: the MX path runs) with LoRA adapters and
its frozen base projections in fp8, against the same model in bf16 and against the plain fp8 model -- every bound is
a multiple of an fp8-versus-bf16 distance measured on the same batch without adapters -- TrainEngine steps, the e4m3
weight copies built once, FP8_SITES, the bf16 cached decode, and one decoder layer at the 4B widths."""
import json

import pytest
import torch

import harness as H
import lora_ref as LR

pytestmark = pytest.mark.gpu
R, ALPHA, SEED = 8, 16.0, 7
S = ALPHA / R
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
_RECORDED = {}


def _record(**kv):
    """The measured figures, written before anything is asserted, to lora_fp8_tiny.json in the parity directory the
    4B parity tests use ($SVLA_PARITY_DIR or their default)."""
    from test_full4b_gpu import _dump
    _RECORDED.update(kv)
    _dump("lora_fp8_tiny.json", _RECORDED)


def _model(ctx, lora=True, adapters=None, fp8=False):
    m = H.build_hip_model(ctx["cfgd"], "cuda:0")
    m.predict_depth = lambda pv, _d=ctx["depth_dev"]: _d  # device tensor: no host copy inside a graph capture
    if lora:
        m.add_lora(R, ALPHA, seed=0)
        if adapters is not None:
            LR.set_model_adapters(m, adapters)
        if fp8:
            m.enable_fp8_lora()
    elif fp8:
        m.enable_fp8_projections(True)
    return m


@pytest.fixture(scope="module")
def ctx(cuda):
    """The runs the tests below share, computed once and left unchanged: the base model in bf16 and in fp8 (full
    fine-tune: logits and projection weight gradients, the two baselines), the adapted model in bf16 and in fp8, and
    the CPU oracle's merged-versus-adapter distance (test_lora_merge's yardstick)."""
    import spatialvla_oracle as O
    from spatialvla_amd import presets
    cfgd = H.cfg_dict("tiny")
    bc = H.batch_tensors(presets.synthetic_batch(cfgd, batch=2, seed=SEED), "cpu")
    bd = {k: v.to(cuda) for k, v in bc.items()}
    P, zoe = H.build_oracle(cfgd)
    cap = {}
    with torch.no_grad():
        O.forward(P, cfgd, bc, zoe, cap=cap)
        depth = cap["depth"]
        ads = LR.make_adapters(P, cfgd, R, SEED)
        with LR.oracle_lora(P, ads, S):
            _, logits_a = O.forward(P, cfgd, bc, zoe, depth=depth)
        _, logits_m = O.forward(LR.merged_params(P, ads, S), cfgd, bc, zoe, depth=depth)
    c = dict(cfgd=cfgd, bd=bd, depth_dev=depth.to(cuda), ads=ads, oracle_merge_dist=H.rel_l2(logits_m, logits_a))
    c["base_bf16"] = H.run_hip(_model(c, lora=False), bd)
    c["base_fp8"] = H.run_hip(_model(c, lora=False, fp8=True), bd)
    c["lora_bf16"] = H.run_hip(_model(c, adapters=ads), bd)
    c["lora_fp8"] = H.run_hip(_model(c, adapters=ads, fp8=True), bd)
    c["fp8_base_logits_rel"] = H.rel_l2(c["base_fp8"][1], c["base_bf16"][1])
    gb, gf = c["base_bf16"][2], c["base_fp8"][2]
    proj = [n for n in gb if n.startswith("language_model.model.layers.") and n.endswith(tuple(p + ".weight" for p in PROJ))]
    assert len(proj) == 7 * cfgd["text_config"]["num_hidden_layers"]
    c["fp8_base_grad_rel"] = {n: H.rel_l2(gf[n], gb[n]) for n in proj}
    return c


def test_fp8_lora_zero_B_equals_plain_fp8(ctx):
    """add_lora's own initialisation (B = 0) on the fp8 base: the logits of the plain fp8 model, bit for bit (measured:
    the RoPE and GeGLU epilogues of the fp8 GEMM round q | k and g | u to bf16 before applying them, which is what the
    rank-r pass reads back; a zero B adds exact zeros).  The issue's fallback bound was 5e-3."""
    with torch.no_grad():
        a = _model(ctx, fp8=True)(**ctx["bd"], return_dict=True).logits.float().cpu()
    d = H.rel_l2(a, ctx["base_fp8"][1])
    _record(zero_B_vs_plain_fp8_logits_rel=d, zero_B_bit_identical=bool(torch.equal(a, ctx["base_fp8"][1])))
    print(f"fp8 lora zero B vs plain fp8: rel {d:.3e}, identical {torch.equal(a, ctx['base_fp8'][1])}")
    assert torch.equal(a, ctx["base_fp8"][1])


def test_fp8_lora_logits_and_loss(ctx):
    """Non-zero adapters.  Bound on the fp8-LoRA logits against the bf16-LoRA logits: 1.5 x the plain fp8 base model's
    distance from the bf16 base model on the same batch (the adapters add two bf16 roundings per projection on top of
    the same operand noise)."""
    from test_full4b_gpu import FP8_TOL
    loss_f, logits_f = ctx["lora_fp8"][:2]
    loss_b, logits_b = ctx["lora_bf16"][:2]
    base = ctx["fp8_base_logits_rel"]
    d = H.rel_l2(logits_f, logits_b)
    moved = H.rel_l2(logits_f, ctx["base_fp8"][1])
    _record(fp8_base_logits_rel=base, fp8_lora_logits_rel=d, loss_fp8_lora=float(loss_f), loss_bf16_lora=float(loss_b),
            fp8_lora_vs_fp8_base_logits_rel=moved)
    print(f"fp8 lora: logits rel {d:.3e} (fp8 base vs bf16 base {base:.3e}), loss {float(loss_f):.5f} vs "
          f"{float(loss_b):.5f}, adapters move the logits by {moved:.3e}")
    assert moved > 0.1  # the adapters matter: dropping them cannot pass
    assert d <= 1.5 * base
    assert abs(float(loss_f) - float(loss_b)) < FP8_TOL["loss"]


def test_fp8_lora_gradients(ctx):
    """Bound on every adapter gradient against the bf16-LoRA gradient: 2 x the largest fp8-versus-bf16 rel-L2 error
    over the seven projection weight gradients of the full fine-tune on the same batch (dA and dB are built from the
    same fp8-noised dy)."""
    gf, gb = ctx["lora_fp8"][2], ctx["lora_bf16"][2]
    base = max(ctx["fp8_base_grad_rel"].values())
    rel = {n: H.rel_l2(gf[n], gb[n]) for n in gb if n in gf}
    _record(fp8_base_grad_rel=ctx["fp8_base_grad_rel"], fp8_base_grad_rel_max=base, fp8_lora_grad_rel=rel,
            fp8_lora_grad_rel_max=max(rel.values()))
    print(f"fp8 lora grads: max rel {max(rel.values()):.3e} (full fine-tune fp8 vs bf16 max {base:.3e})")
    assert len(gf) == 28 and gf.keys() == gb.keys()
    assert all(".lora." in n for n in gf), "no base parameter may have a gradient"
    for n, v in rel.items():
        assert v <= 2.0 * base, (n, v, base)


def _quant_counters(monkeypatch):
    """Wrap the three MX quantisers with a log of the shapes they were given."""
    from spatialvla_amd import kernels as Kn
    log = []
    for name in ("quant_mx_both", "quant_mx_rows", "quant_mx_cols"):
        orig = getattr(Kn, name)

        def wrapped(x, *a, _orig=orig, _name=name, **kw):
            log.append((_name, tuple(x.shape)))
            return _orig(x, *a, **kw)
        monkeypatch.setattr(Kn, name, wrapped)
    return log


def _weight_shapes(m):
    out = set()
    for l in m.language_model.model.layers:
        a, p = l.self_attn, l.mlp
        out.add((a.q_proj.out_features + a.k_proj.out_features + a.v_proj.out_features, a.q_proj.in_features))
        out.add(tuple(a.o_proj.weight.shape))
        out.add((2 * p.gate_proj.out_features, p.gate_proj.in_features))
        out.add(tuple(p.down_proj.weight.shape))
    return out


def _engine_run(ctx, ckpt, log=None):
    from spatialvla_amd.engine import TrainEngine
    m = _model(ctx, fp8=True)
    m.train()
    m.vision_zoe_model.eval()
    if ckpt:
        m.language_model._set_gradient_checkpointing()
    base0 = {n: p.detach().clone() for n, p in m.named_parameters() if ".lora." not in n}
    eng = TrainEngine(m, lr=2e-3, warmup_ratio=0.0, total_steps=10, max_grad_norm=1.0)
    assert m.fp8_lora
    losses, marks = [], []
    for _ in range(3):
        losses.append(eng.train_step(ctx["bd"]).clone())
        marks.append(len(log) if log is not None else 0)
    losses = torch.stack(losses).cpu()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        if ".lora." not in n:
            assert torch.equal(p.detach(), base0[n]), n
    return m, eng, losses, eng.full_master().cpu(), marks


def test_fp8_lora_train_engine_and_copies_built_once(ctx, monkeypatch):
    log = _quant_counters(monkeypatch)
    m, eng, losses, master, marks = _engine_run(ctx, False, log)
    ws = _weight_shapes(m)
    rows = ctx["bd"]["input_ids"].numel()
    assert all(s[0] != rows for s in ws), "an activation shape would be mistaken for a weight"
    n_layers = len(m.language_model.model.layers)
    step1 = [e for e in log[:marks[0]] if e[1] in ws]
    later = [e for e in log[marks[0]:marks[2]] if e[1] in ws]
    act_later = [e for e in log[marks[0]:marks[2]] if e[1] not in ws]
    print(f"fp8 lora engine losses {losses.tolist()}; weight quantisations: step 1 {len(step1)}, steps 2-3 {len(later)}; "
          f"activation quantisation passes in steps 2-3: {len(act_later)}")
    assert len(eng.params) == 28
    assert len(step1) == 4 * n_layers and all(e[0] == "quant_mx_both" for e in step1)
    assert later == []
    assert float(losses[2]) < float(losses[0])
    _, _, losses2, master2, _ = _engine_run(ctx, False)
    assert torch.equal(losses, losses2) and torch.equal(master, master2)
    _, _, losses3, master3, _ = _engine_run(ctx, True)
    _record(engine_losses=losses.tolist(), engine_losses_checkpointing=losses3.tolist(),
            checkpointing_bitwise=bool(torch.equal(losses, losses3) and torch.equal(master, master3)))
    # every MX copy a slot hands over is bitwise the quantisation pass it replaces, so the recompute changes no bit
    assert torch.equal(losses, losses3) and torch.equal(master, master3)

    # merge_lora() turns the switch off and leaves a plain bf16 model; enable_fp8_projections(True) then quantises the
    # merged weights on its next forward
    m2 = _model(ctx, adapters=ctx["ads"], fp8=True)
    with torch.no_grad():
        before = m2(**ctx["bd"], return_dict=True).logits.float().cpu()
    assert torch.equal(before, ctx["lora_fp8"][1])
    m2.merge_lora()
    assert not m2.has_lora and not m2.fp8_lora
    m2.enable_fp8_projections(True)
    n0 = len(log)
    with torch.no_grad():
        after = m2(**ctx["bd"], return_dict=True).logits.float().cpu()
    rebuilt = [e for e in log[n0:] if e[1] in ws]
    dist = H.rel_l2(after, before)
    # test_lora_merge's bound (2 x the CPU oracle's merged-versus-adapter distance: the re-rounding of the weights) plus
    # 1.5 x the fp8 baseline, the allowance test_fp8_lora_logits_and_loss gives one fp8 model against its bf16 partner:
    # the merged weights quantise to other e4m3 values than W, and the adapter term, bf16 before the merge, now passes
    # through the e4m3 operands as well
    bound = 2.0 * ctx["oracle_merge_dist"] + 1.5 * ctx["fp8_base_logits_rel"]
    _record(merge_then_fp8_logits_rel=dist, oracle_merge_logits_rel=ctx["oracle_merge_dist"], merge_then_fp8_bound=bound)
    print(f"fp8 lora merge -> fp8: logits rel {dist:.3e}, bound {bound:.3e}")
    assert len(rebuilt) == 4 * n_layers
    assert dist <= bound


def test_fp8_lora_copies_follow_base_weight_changes(ctx, monkeypatch):
    """What really rewrites a base weight still rebuilds its copy: an in-place change, a move, and an optimizer epoch
    once the weight sits in an engine's flat buffers; the epoch alone does not."""
    from spatialvla_amd import functional as Fn
    log = _quant_counters(monkeypatch)
    m = _model(ctx, adapters=ctx["ads"], fp8=True)
    ws = _weight_shapes(m)
    w = m.language_model.model.layers[0].mlp.down_proj.weight

    def rebuilt():
        n0 = len(log)
        with torch.no_grad():
            out = m(**ctx["bd"], return_dict=True).logits
        return len([e for e in log[n0:] if e[1] in ws]), out

    assert rebuilt()[0] == 4 * len(m.language_model.model.layers)
    n, ref = rebuilt()
    assert n == 0
    e0 = Fn.WEIGHT_EPOCH[0]
    try:
        Fn.WEIGHT_EPOCH[0] += 1
        assert rebuilt()[0] == 0
        with torch.no_grad():
            w.mul_(2.0)
        n, out = rebuilt()
        assert n == 1 and not torch.equal(out, ref)
        w.data = (w.data * 0.5).clone()  # the old values at a new address
        n, out = rebuilt()
        assert n == 1 and torch.equal(out, ref)
        Fn.register_flat_param(w)  # as TrainEngine does for what its flat buffers hold: the epoch enters the key
        assert rebuilt()[0] == 1
        assert rebuilt()[0] == 0
        Fn.WEIGHT_EPOCH[0] += 1
        assert rebuilt()[0] == 1
    finally:
        Fn.WEIGHT_EPOCH[0] = e0


def test_fp8_lora_sites(ctx, monkeypatch):
    """FP8_SITES = {"qkv"}: only the q|k|v projection (forward and input gradient) leaves the bf16 GEMM -- one
    svla_gemm_mxfp8 call per layer and pass, on that layer's q|k|v copy, and no other copy is ever built."""
    from spatialvla_amd import functional as Fn, kernels as Kn
    calls = []
    orig = Kn.gemm_mxfp8

    def wrapped(xq, xs, wq, ws, out, *a, **kw):
        calls.append(wq.data_ptr())
        return orig(xq, xs, wq, ws, out, *a, **kw)
    monkeypatch.setattr(Kn, "gemm_mxfp8", wrapped)
    m = _model(ctx, adapters=ctx["ads"], fp8=True)
    layers = m.language_model.model.layers
    with monkeypatch.context() as mp:
        mp.setattr(Fn, "FP8_SITES", [{"qkv"}])
        with torch.no_grad():
            m(**ctx["bd"], return_dict=True)
        copies = [l.mlp._svla_fp8_lora.mats for l in layers]
        assert all(set(c) == {"qkv"} for c in copies)
        assert calls == [c["qkv"]["q"].data_ptr() for c in copies]
        del calls[:]
        H.run_hip(m, ctx["bd"])
        assert all(set(c) == {"qkv"} for c in copies)
        n = len(layers)
        assert calls[:n] == [c["qkv"]["q"].data_ptr() for c in copies]
        # backward, last layer first: the q|k|v input gradient on W^T wherever the layer input needs a gradient
        back = calls[n:]
        assert 1 <= len(back) <= n and back == [c["qkv"]["qt"].data_ptr() for c in copies[::-1]][:len(back)]
    del calls[:]
    with torch.no_grad():
        m(**ctx["bd"], return_dict=True)
    assert len(calls) == 4 * len(layers)  # all four sites by default


def test_fp8_lora_decode_stays_bf16(ctx, monkeypatch):
    """The KV-cached forward under enable_lora_decode() never sees the switch: no svla_gemm_mxfp8 launch and no
    quantisation during predict_action or a cached prefill (fused decode steps, and the unfused loop the prefill and
    DECODE_NORM_FUSED = 0 take), prefill logits and KV cache bitwise those with the switch off, tokens equal."""
    from spatialvla_amd import functional as Fn, kernels as Kn
    m = _model(ctx, adapters=ctx["ads"])
    m.enable_lora_decode()
    bd = ctx["bd"]
    inputs = {"input_ids": bd["input_ids"][:, :-13], "pixel_values": bd["pixel_values"], "intrinsic": bd["intrinsic"]}

    def cached_prefill():
        cache = m.new_cache(2, 400)
        with torch.no_grad():
            logits = m(**inputs, past_key_values=cache).logits
        n = cache.seen_tokens
        return logits.clone(), cache.key_cache[:, :, :n].clone(), cache.value_cache[:, :, :n].clone()

    off = m.predict_action(inputs, max_new_tokens=4, eos_token_id=-1).clone()
    pre_off = cached_prefill()
    m.enable_fp8_lora()
    assert m.fp8_lora and m.lora_decode
    calls = []
    orig = Kn.gemm_mxfp8
    monkeypatch.setattr(Kn, "gemm_mxfp8", lambda *a, **kw: (calls.append("gemm_mxfp8"), orig(*a, **kw))[1])
    log = _quant_counters(monkeypatch)
    on = m.predict_action(inputs, max_new_tokens=4, eos_token_id=-1).clone()
    pre_on = cached_prefill()
    monkeypatch.setattr(Fn, "DECODE_NORM_FUSED", [False])
    m.clear_decode_cache()
    unfused = m.predict_action(inputs, max_new_tokens=4, eos_token_id=-1)
    assert calls == [] and log == []
    assert torch.equal(on, off) and torch.equal(unfused, off)
    for x, y in zip(pre_on, pre_off):
        assert torch.equal(x, y)
    with torch.no_grad():  # the uncached forward of the same model does run in fp8
        m(**bd, return_dict=True)
    assert len(calls) == 4 * len(m.language_model.model.layers)


def test_fp8_lora_layer_4b_width(cuda):
    """One Gemma2 layer at hidden 2304 / I 9216 / D 256 with 2 x 312 rows and r = 32 (as
    test_lora_layer_4b_width_kernels_vs_composition builds it): the fp8-LoRA layer against the bf16-LoRA layer within
    0.12, the project's bound for the fp8 layer against the bf16 layer (test_gemma2_layer_fp8_vs_bf16).  The only place
    the 18432-column GeGLU pass with the MX output runs at its real width."""
    from spatialvla_amd import SpatialVLAConfig, presets
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
        for sub, names in ((layer.self_attn, PROJ[:4]), (layer.mlp, PROJ[4:])):
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

    yb, dxb, gb = run()
    layer.set_fp8_lora(True)
    yf, dxf, gf = run()
    e_y, e_dx = H.rel_l2(yf - h0, yb - h0), H.rel_l2(dxf, dxb)
    print(f"fp8 lora layer at 4B widths: y rel {H.rel_l2(yf, yb):.3e} (branch output {e_y:.3e}), dx rel {e_dx:.3e}")
    assert H.rel_l2(yf, yb) < 0.12 and e_dx < 0.12
    assert len(gf) == 14 and gf.keys() == gb.keys()
    assert not torch.equal(yf, yb)  # the fp8 GEMMs ran
