"""KV-cached decode with unmerged LoRA adapters (enable_lora_decode) on the tiny model: greedy tokens against the CPU
oracle patched by tests/lora_ref.py, teacher-forced cached logits against the uncached adapter forward, the adapter
GEMVs against their composition from the training-path kernels, padded prompts, graph staleness, merge, mid-training
evaluation and the switch.  The measured figures go to lora_decode_tiny.json before anything is asserted."""
import os

import pytest
import torch
from safetensors.torch import load_file

import harness as H
import lora_ref as LR

pytestmark = pytest.mark.gpu
R, ALPHA, SEED, AD_SEED, N_NEW = 8, 16.0, 7, 8, 6
S = ALPHA / R
_RECORDED = {}


def _record(**kv):
    from test_full4b_gpu import _dump
    _RECORDED.update(kv)
    _dump("lora_decode_tiny.json", _RECORDED)


def _lora_model(ctx, switch=True):
    m = H.build_hip_model(ctx["cfgd"], "cuda:0")
    m.predict_depth = lambda pv, _d=ctx["depth_dev"]: _d  # device tensor: no host copy inside a graph capture
    m.add_lora(R, ALPHA, seed=0)
    LR.set_model_adapters(m, ctx["ads"])
    if switch:
        m.enable_lora_decode()
    return m


@pytest.fixture(scope="module")
def ctx(cuda):
    """The oracle's greedy decode with adapters (and without, to show they matter), computed once on the CPU."""
    import spatialvla_oracle as O
    from spatialvla_amd import presets
    cfgd = H.cfg_dict("tiny")
    bc = H.batch_tensors(presets.synthetic_batch(cfgd, batch=2, seed=SEED), "cpu")
    bd = {k: v.to(cuda) for k, v in bc.items()}
    P, zoe = H.build_oracle(cfgd)
    prompt_c = {"input_ids": bc["input_ids"][:, :-13], "pixel_values": bc["pixel_values"], "intrinsic": bc["intrinsic"]}
    with torch.no_grad():
        cap = {}
        O.forward(P, cfgd, bc, zoe, cap=cap)
        depth = cap["depth"]
        ads = LR.make_adapters(P, cfgd, R, AD_SEED)
        with LR.oracle_lora(P, ads, S):
            toks, margins = O.greedy_decode(P, cfgd, prompt_c, zoe, n_new=N_NEW, depth=depth)
        toks0, _ = O.greedy_decode(P, cfgd, prompt_c, zoe, n_new=N_NEW, depth=depth)
    c = dict(cfgd=cfgd, bc=bc, bd=bd, depth_dev=depth.to(cuda), ads=ads, toks=toks, margins=margins, toks_base=toks0,
             prompt={k: v.to(cuda) for k, v in prompt_c.items()})
    c["model"] = _lora_model(c)
    return c


def _teacher_forced(model, bd):
    """Prefill with use_cache=True, then steps of 1 and 2 tokens through past_key_values; the uncached forward over
    the same P + 3 tokens with the matching KVMask; the prompt alone, uncached."""
    from spatialvla_amd.modeling_gemma2 import KVMask
    ids = bd["input_ids"]
    B, L = ids.shape
    P = L - 13
    pv, intr = bd["pixel_values"], bd["intrinsic"]
    with torch.no_grad():
        o1 = model(input_ids=ids[:, :P], pixel_values=pv, intrinsic=intr, use_cache=True)
        cache = o1.past_key_values
        assert cache.get_seq_length() == P
        l1 = o1.logits.clone()
        l2 = model(input_ids=ids[:, P:P + 1], past_key_values=cache).logits.clone()
        l3 = model(input_ids=ids[:, P + 1:P + 3], past_key_values=cache).logits.clone()
        assert cache.get_seq_length() == P + 3
        cls = torch.ones(B, P + 3, dtype=torch.uint8, device=ids.device)
        cls[:, :P] = 0
        ref = model(input_ids=ids[:, :P + 3], pixel_values=pv, intrinsic=intr, kv_mask=KVMask(cls)).logits.clone()
        prompt = model(input_ids=ids[:, :P], pixel_values=pv, intrinsic=intr).logits.clone()
    return dict(P=P, prefill=l1, step1=l2, step2=l3, ref=ref, prompt=prompt)


def _gated_argmax_equal(a, ref, what):
    """argmax(a) == argmax(ref) wherever ref's top-1 / top-2 margin exceeds the harness margin."""
    top2 = ref.float().topk(2, -1).values
    conf = (top2[..., 0] - top2[..., 1]) > H.MARGIN
    agree = a.float().argmax(-1) == ref.float().argmax(-1)
    assert bool(agree[conf].all()), what
    return int(conf.sum()), int(conf.numel())


def test_tokens_against_oracle(ctx):
    m = ctx["model"]
    toks, margins = ctx["toks"], ctx["margins"]
    n_diff = int((toks != ctx["toks_base"]).sum())
    runs = {}
    m.decode_graphs = False
    runs["eager"] = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    m.decode_graphs = True
    runs["capture"] = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    runs["replay"] = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    P = ctx["prompt"]["input_ids"].shape[1]
    gen = m.generate(**ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    assert gen.shape == (2, P + N_NEW) and torch.equal(gen[:, :P], ctx["prompt"]["input_ids"])
    runs["generate"] = gen[:, P:]
    _record(oracle_tokens=toks.tolist(), oracle_margins=[[round(float(v), 3) for v in r] for r in margins],
            oracle_tokens_differ_from_base=n_diff, tokens={k: v.tolist() for k, v in runs.items()})
    print(f"oracle tokens {toks.tolist()} margins {margins.tolist()} ({n_diff}/12 differ from the base model's)")
    assert n_diff >= 6  # the adapters decide the tokens: a decode that dropped them cannot pass
    for k, got in runs.items():
        assert got.shape == (2, N_NEW), k
        n_cmp, n_ok = H.greedy_tokens_agree(got, toks, margins)
        print(f"{k}: {got.tolist()} {n_ok}/{n_cmp}")
        _record(**{f"tokens_ok_{k}": [n_ok, n_cmp]})
        assert n_ok >= 8, (k, got.tolist())
    assert torch.equal(runs["capture"], runs["eager"]) and torch.equal(runs["replay"], runs["eager"])


@pytest.fixture(scope="module")
def forced(ctx):
    from spatialvla_amd import functional as Fn
    out = {"kernels": _teacher_forced(ctx["model"], ctx["bd"])}
    try:
        Fn.LORA_DECODE_KERNELS[0] = False
        out["composed"] = _teacher_forced(ctx["model"], ctx["bd"])
    finally:
        Fn.LORA_DECODE_KERNELS[0] = True
    base = H.build_hip_model(ctx["cfgd"], "cuda:0")
    base.predict_depth = ctx["model"].predict_depth
    out["base"] = _teacher_forced(base, ctx["bd"])
    return out


def _block_rels(f):
    P = f["P"]
    return {"prefill": H.rel_l2(f["prefill"], f["ref"][:, :P]), "step1": H.rel_l2(f["step1"], f["ref"][:, P:P + 1]),
            "step2": H.rel_l2(f["step2"], f["ref"][:, P + 1:P + 3])}


def test_teacher_forced_logits(ctx, forced):
    f = forced["kernels"]
    P = f["P"]
    rel, rel_base = _block_rels(f), _block_rels(forced["base"])
    moved = H.rel_l2(f["ref"], forced["base"]["ref"])
    _record(forced_rel=rel, forced_rel_base_model=rel_base, adapter_vs_base_logits_rel=moved)
    print(f"teacher-forced rel-L2 {rel} (base model {rel_base}); adapters move the logits by {moved:.3f}")
    assert moved > 0.1
    for k, v in rel.items():
        assert v < H.LOGITS_TOL, (k, v)
    _gated_argmax_equal(f["step1"], f["ref"][:, P:P + 1], "step1")
    _gated_argmax_equal(f["step2"], f["ref"][:, P + 1:P + 3], "step2")


def test_prompt_logits_bitwise(forced):
    """The cached prefill's logits equal the uncached adapter forward's over the same prompt: the base prefill is
    bit-identical, and svla_lora_up + svla_qkv_rope_fill share SVLA_EPI_ROPE's rounding with svla_lora_up's ROPE
    epilogue."""
    f = forced["kernels"]
    d = float((f["prefill"].float() - f["prompt"].float()).abs().max())
    b = forced["base"]
    _record(prefill_vs_uncached_prompt_maxabs=d,
            prefill_vs_uncached_prompt_maxabs_base_model=float((b["prefill"].float() - b["prompt"].float()).abs().max()))
    assert torch.equal(f["prefill"], f["prompt"])


def test_kernels_against_composition(forced):
    k, c = forced["kernels"], forced["composed"]
    P = k["P"]
    rel = {b: H.rel_l2(k[b], c[b]) for b in ("prefill", "step1", "step2")}
    _record(kernels_vs_composed_rel=rel, composed_rel=_block_rels(c))
    print(f"adapter GEMVs vs composition: {rel}")
    assert torch.equal(k["prefill"], c["prefill"])  # the prefill does not depend on the switch
    for b, v in rel.items():
        assert v < H.LOGITS_TOL, (b, v)
    for b, v in _block_rels(c).items():
        assert v < H.LOGITS_TOL, (b, v)
    for b, sl in (("step1", slice(P, P + 1)), ("step2", slice(P + 1, P + 3))):
        ref = k["ref"][:, sl]
        _gated_argmax_equal(k[b], ref, b)
        _gated_argmax_equal(c[b], ref, b)


def test_decode_step_runs_the_adapter_gemvs(ctx, monkeypatch):
    """A decode step takes 4 svla_lora_gemv_down + 4 svla_lora_gemv per layer (q|k|v, o, gate|up, down) and none of
    the training-path adapter kernels; with LORA_DECODE_KERNELS off it is the other way round.  The prefill uses the
    training-path kernels either way."""
    from spatialvla_amd import functional as Fn, kernels as Kn
    m = ctx["model"]
    calls = {}
    for name in ("lora_gemv_down", "lora_gemv", "lora_down", "lora_up", "gemv_rmsnorm2", "decode_mlp"):
        def wrapped(*a, _f=getattr(Kn, name), _n=name, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(Kn, name, wrapped)
    ids = ctx["bd"]["input_ids"]
    P = ids.shape[1] - 13
    nl = ctx["cfgd"]["text_config"]["num_hidden_layers"]
    with torch.no_grad():
        cache = m(input_ids=ids[:, :P], pixel_values=ctx["bd"]["pixel_values"], intrinsic=ctx["bd"]["intrinsic"],
                  use_cache=True).past_key_values
        assert calls.get("lora_gemv", 0) == 0 and calls.get("lora_gemv_down", 0) == 0 and calls["lora_up"] == 4 * nl
        calls.clear()
        m(input_ids=ids[:, P:P + 1], past_key_values=cache)
        assert calls == {"lora_gemv_down": 4 * nl, "lora_gemv": 4 * nl}, calls
        calls.clear()
        try:
            Fn.LORA_DECODE_KERNELS[0] = False
            m(input_ids=ids[:, P + 1:P + 2], past_key_values=cache)
        finally:
            Fn.LORA_DECODE_KERNELS[0] = True
        assert calls.get("lora_gemv", 0) == 0 and calls.get("lora_gemv_down", 0) == 0 and calls["lora_up"] == 4 * nl


def _uncached_step_logits(m, inputs, toks):
    """Logits of every greedy step from one uncached forward over prompt + the given tokens (teacher-forced)."""
    from spatialvla_amd.modeling_gemma2 import KVMask
    ids, pv, intr, am, dev = m._predict_inputs(inputs)
    B, P = ids.shape
    n = toks.shape[1]
    full = torch.cat([ids, toks[:, :-1].to(dev)], 1)
    cls = torch.ones(B, P + n - 1, dtype=torch.uint8, device=dev)
    cls[:, :P] = m._prompt_classes(am, B, P, dev)
    pos = m._prompt_positions(cls != 2)
    with torch.no_grad():
        logits = m(input_ids=full, pixel_values=pv, intrinsic=intr, kv_mask=KVMask(cls.contiguous()),
                   position_ids=pos).logits
    return logits[:, P - 1:].float()


def test_padded_batch(ctx, cuda):
    g = load_file(os.path.join(os.path.dirname(__file__), "golden", "decode_padded.safetensors"))
    assert bool((g["in.attention_mask"] == 0).any())
    m = ctx["model"]
    depth = g["out.depth"].to(cuda)
    keep = m.predict_depth
    m.predict_depth = lambda p: depth
    m.clear_decode_cache()
    try:
        inputs = {"input_ids": g["in.input_ids"], "attention_mask": g["in.attention_mask"],
                  "pixel_values": g["in.pixel_values"], "intrinsic": g["in.intrinsic"]}
        n = 4
        unc = m.predict_action_uncached(inputs, max_new_tokens=n, eos_token_id=-1)
        top2 = _uncached_step_logits(m, inputs, unc).topk(2, -1).values
        margins = top2[..., 0] - top2[..., 1]
        out = {}
        for graphs in (False, True):
            m.decode_graphs = graphs
            out[graphs] = m.predict_action(inputs, max_new_tokens=n, eos_token_id=-1)
        m.decode_graphs = True
        _record(padded_tokens_uncached=unc.tolist(), padded_tokens_cached=out[False].tolist(),
                padded_margins=[[round(float(v), 3) for v in r] for r in margins])
        for graphs, got in out.items():
            n_cmp, n_ok = H.greedy_tokens_agree(got, unc, margins)
            print(f"padded (graphs {graphs}): {got.tolist()} vs uncached {unc.tolist()}: {n_ok}/{n_cmp}")
            assert n_ok >= got.shape[0]  # at least every first token (an error would have raised in the margin rule)
        assert torch.equal(out[True], out[False])
    finally:
        m.predict_depth = keep
        m.clear_decode_cache()


def test_graphs_read_adapters_in_place(ctx):
    """An in-place update of A / B (an optimizer step on the flat buffer) needs no re-capture."""
    m = _lora_model(ctx)
    m.decode_graphs = True
    first = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    st = next(iter(m._svla_decode_states.values()))
    n_graphs = len(st["graphs"])
    assert n_graphs == N_NEW - 1
    with torch.no_grad():
        for _, lin in m._lora_linears():
            lin.lora.B.mul_(-1)
    replay = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    assert next(iter(m._svla_decode_states.values())) is st and len(st["graphs"]) == n_graphs  # replayed, not re-captured
    m.decode_graphs = False
    eager = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    _record(stale_first=first.tolist(), stale_replay=replay.tolist(), stale_eager=eager.tolist())
    assert torch.equal(replay, eager)
    assert not torch.equal(replay, first)


def test_merge_and_switch_clear_states(ctx):
    m = _lora_model(ctx)
    m.predict_action(ctx["prompt"], max_new_tokens=2, eos_token_id=-1)
    assert len(m._svla_decode_states) == 1
    assert next(iter(m._svla_decode_states.values()))["wptr"][2][0] is True
    m.enable_lora_decode(False)
    assert len(m._svla_decode_states) == 0
    with pytest.raises(RuntimeError, match=r"call merge_lora\(\) first"):
        m.predict_action(ctx["prompt"], max_new_tokens=2, eos_token_id=-1)
    m.enable_lora_decode(True)
    with_ad = m.predict_action(ctx["prompt"], max_new_tokens=3, eos_token_id=-1)
    assert len(m._svla_decode_states) == 1
    m.merge_lora()
    assert len(m._svla_decode_states) == 0 and not m.has_lora
    merged = m.predict_action(ctx["prompt"], max_new_tokens=3, eos_token_id=-1)
    assert next(iter(m._svla_decode_states.values()))["wptr"][2] is None  # the base path: no adapters in the key
    assert merged.shape == with_ad.shape
    _record(merged_tokens=merged.tolist(), unmerged_tokens=with_ad.tolist())


def test_mid_training_evaluation(ctx):
    from spatialvla_amd.engine import TrainEngine
    m = _lora_model(ctx)
    m.train()
    m.vision_zoe_model.eval()
    m.decode_graphs = True
    before = m.predict_action(ctx["prompt"], max_new_tokens=4, eos_token_id=-1)
    eng = TrainEngine(m, lr=2e-3, warmup_ratio=0.0, total_steps=10, max_grad_norm=1.0)
    loss = eng.train_step(ctx["bd"]).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    graphs = m.predict_action(ctx["prompt"], max_new_tokens=4, eos_token_id=-1)
    m.decode_graphs = False
    eager = m.predict_action(ctx["prompt"], max_new_tokens=4, eos_token_id=-1)
    _record(mid_training_tokens=graphs.tolist(), mid_training_before=before.tolist())
    assert graphs.shape == (2, 4) and torch.equal(graphs, eager)


def test_switch_off_refuses(ctx):
    m = _lora_model(ctx, switch=False)
    with pytest.raises(RuntimeError) as e:
        m.predict_action(ctx["prompt"], max_new_tokens=2, eos_token_id=-1)
    assert str(e.value) == ("predict_action: call merge_lora() first (unmerged LoRA adapters; the KV-cached decode "
                            "kernels read the base weights only)")
    ids = ctx["bd"]["input_ids"][:, :-13]
    with pytest.raises(RuntimeError, match=r"call merge_lora\(\) first"):
        with torch.no_grad():
            m(input_ids=ids, pixel_values=ctx["bd"]["pixel_values"], intrinsic=ctx["bd"]["intrinsic"],
              past_key_values=m.new_cache(2, 400), output_hidden_states=True)
    # output_hidden_states with a cache takes the per-layer path: with the switch on it runs there too
    on = ctx["model"]
    with torch.no_grad():
        a = on(input_ids=ids, pixel_values=ctx["bd"]["pixel_values"], intrinsic=ctx["bd"]["intrinsic"],
               past_key_values=on.new_cache(2, 400), output_hidden_states=True)
        b = on(input_ids=ids, pixel_values=ctx["bd"]["pixel_values"], intrinsic=ctx["bd"]["intrinsic"], use_cache=True)
    assert len(a.hidden_states) == ctx["cfgd"]["text_config"]["num_hidden_layers"] + 1
    assert H.rel_l2(a.logits, b.logits) < H.LOGITS_TOL
