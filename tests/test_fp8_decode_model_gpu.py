"""Weight-only MX fp8 decode (enable_fp8_decode) on the tiny model: the prefill is untouched, the kernel path equals the
bf16 path of a model whose weights are the dequantised copies W', the quantisation error against the bf16 model is
measured (fp8_decode_tiny.json, written before anything is asserted) and compared with the fp8 projections', greedy
tokens of predict_action / generate, the dispatch, the switch, and weight changes.

The W' reference model shares the fp8 model's prefill: its weights are overwritten in place with W' only after the
prompt is in the cache (the fp8 model's prefill reads the bf16 weights), so the two differ in the decode steps'
summation order only."""
import os

import pytest
import torch
from safetensors.torch import load_file

import harness as H

pytestmark = pytest.mark.gpu
SEED, N_NEW = 7, 6
_RECORDED = {}


def _record(**kv):
    from test_full4b_gpu import _dump
    _RECORDED.update(kv)
    _dump("fp8_decode_tiny.json", _RECORDED)


def _dequant_mx(q, sc):
    X = sc.exponents()
    rows, k = q.shape
    return (q.float().view(rows, k // 32, 32) * torch.exp2(X.float())[..., None]).view(rows, k)


def _quantised_weights(m):
    """[(parameter, its bf16 value, W' = the exact bf16 dequantisation of K.quant_mx_rows of it)] of every weight the fp8
    decode quantises: the seven projections of every layer and lm_head."""
    from spatialvla_amd import kernels as K
    out = []
    ws = [lin.weight for _, lin in m._lora_linears()] + [m.language_model.lm_head.weight]
    for w in ws:
        q, sc = K.quant_mx_rows(w.detach())
        wd = _dequant_mx(q, sc)
        assert torch.equal(wd.to(torch.bfloat16).float(), wd)
        out.append((w, w.detach().clone(), wd.to(torch.bfloat16)))
    return out


def _set_weights(triples, which):
    with torch.no_grad():
        for w, orig, wd in triples:
            w.copy_(wd if which == "wprime" else orig)


def _model(ctx, fp8=False):
    m = H.build_hip_model(ctx["cfgd"], "cuda:0")
    m.predict_depth = lambda pv, _d=ctx["depth"]: _d  # device tensor: no host copy inside a graph capture
    if fp8:
        m.enable_fp8_decode()
    return m


@pytest.fixture(scope="module")
def ctx(cuda):
    from spatialvla_amd import presets
    cfgd = H.cfg_dict("tiny")
    bd = H.batch_tensors(presets.synthetic_batch(cfgd, batch=2, seed=SEED), cuda)
    c = dict(cfgd=cfgd, bd=bd)
    probe = H.build_hip_model(cfgd, "cuda:0")
    with torch.no_grad():
        c["depth"] = probe.predict_depth(bd["pixel_values"]).clone()
    c["prompt"] = {"input_ids": bd["input_ids"][:, :-13], "pixel_values": bd["pixel_values"],
                   "intrinsic": bd["intrinsic"]}
    c["base"] = _model(c)
    c["fp8"] = _model(c, fp8=True)
    c["ref"] = _model(c)
    c["ref_w"] = _quantised_weights(c["ref"])
    return c


def _teacher_forced(model, bd, after_prefill=None):
    """Prefill with use_cache=True, then steps of 1 and 2 tokens through past_key_values."""
    ids = bd["input_ids"]
    P = ids.shape[1] - 13
    with torch.no_grad():
        o1 = model(input_ids=ids[:, :P], pixel_values=bd["pixel_values"], intrinsic=bd["intrinsic"], use_cache=True)
        cache = o1.past_key_values
        l1 = o1.logits.clone()
        if after_prefill is not None:
            after_prefill()
        l2 = model(input_ids=ids[:, P:P + 1], past_key_values=cache).logits.clone()
        l3 = model(input_ids=ids[:, P + 1:P + 3], past_key_values=cache).logits.clone()
        assert cache.get_seq_length() == P + 3
    return dict(P=P, prefill=l1, step1=l2, step2=l3)


def _gated_argmax_equal(a, ref, what):
    top2 = ref.float().topk(2, -1).values
    conf = (top2[..., 0] - top2[..., 1]) > H.MARGIN
    agree = a.float().argmax(-1) == ref.float().argmax(-1)
    assert bool(agree[conf].all()), what
    return int(conf.sum()), int(conf.numel())


@pytest.fixture(scope="module")
def forced(ctx):
    out = {"base": _teacher_forced(ctx["base"], ctx["bd"]), "fp8": _teacher_forced(ctx["fp8"], ctx["bd"])}
    try:
        out["ref"] = _teacher_forced(ctx["ref"], ctx["bd"], lambda: _set_weights(ctx["ref_w"], "wprime"))
    finally:
        _set_weights(ctx["ref_w"], "orig")
    return out


def test_prefill_untouched(ctx, forced):
    assert torch.equal(forced["fp8"]["prefill"], forced["base"]["prefill"])
    assert torch.equal(forced["ref"]["prefill"], forced["base"]["prefill"])
    # the first greedy token comes from the prefill's bf16 head: the e4m3 copy of lm_head is not read there
    m = ctx["fp8"]
    m.decode_graphs = False
    a = m.predict_action(ctx["prompt"], max_new_tokens=1, eos_token_id=-1)
    b = ctx["base"].predict_action(ctx["prompt"], max_new_tokens=1, eos_token_id=-1)
    m.decode_graphs = True
    assert torch.equal(a, b)


def test_kernel_path_equals_dequantised_bf16_path(forced):
    f, r = forced["fp8"], forced["ref"]
    rel = {b: H.rel_l2(f[b], r[b]) for b in ("step1", "step2")}
    moved = {b: H.rel_l2(r[b], forced["base"][b]) for b in ("step1", "step2")}
    _record(kernel_vs_wprime_rel=rel, wprime_vs_bf16_rel=moved)
    print(f"fp8 kernels vs W' on the bf16 path: {rel}; W' vs the bf16 weights: {moved}")
    assert min(moved.values()) > 1e-4  # the reference does run on other weights than the bf16 model
    for b, v in rel.items():
        assert v < H.LOGITS_TOL, (b, v)
        _gated_argmax_equal(f[b], r[b], b)


def test_quantisation_error_against_fp8_projections(ctx, forced):
    """Weight-only e4m3 against the training step's fp8 projections (weights and activations in e4m3) on the same
    tokens: the weight-only error should be the lower one; 1.25 x covers two independent random errors on a 2-layer
    model."""
    from spatialvla_amd.modeling_gemma2 import KVMask
    bd = ctx["bd"]
    ids = bd["input_ids"]
    B = ids.shape[0]
    f, b = forced["fp8"], forced["base"]
    P = f["P"]
    w_only = H.rel_l2(torch.cat([f["step1"], f["step2"]], 1), torch.cat([b["step1"], b["step2"]], 1))
    cls = torch.ones(B, P + 3, dtype=torch.uint8, device=ids.device)
    cls[:, :P] = 0
    kw = dict(input_ids=ids[:, :P + 3], pixel_values=bd["pixel_values"], intrinsic=bd["intrinsic"], kv_mask=KVMask(cls))
    m = _model(ctx)
    with torch.no_grad():
        ref = m(**kw).logits[:, P:].clone()
        m.enable_fp8_projections()
        got = m(**kw).logits[:, P:].clone()
    proj = H.rel_l2(got, ref)
    _record(fp8_decode_vs_bf16_rel=w_only, fp8_projections_vs_bf16_rel=proj,
            fp8_decode_steps_rel={k: H.rel_l2(f[k], b[k]) for k in ("step1", "step2")})
    print(f"decode-step logits rel-L2 against bf16: weight-only fp8 decode {w_only:.4e}, fp8 projections {proj:.4e}")
    assert w_only > 0  # the e4m3 copies are read
    assert w_only <= 1.25 * proj


def _ref_greedy(m, triples, prompt, n, attention_mask=None):
    """The W' model's bf16 greedy decode through the generate() surface (prepare_inputs_for_generation -> forward per
    step), the prompt prefilled on the bf16 weights: tokens [B, n] and the top-2 margin of every step's logits."""
    dev = m.language_model.lm_head.weight.device
    ids = prompt["input_ids"].to(dev)
    B, P = ids.shape
    am = attention_mask.to(dev) if attention_mask is not None else torch.ones(B, P, dtype=torch.int64, device=dev)
    pv, intr = prompt["pixel_values"].to(dev, torch.bfloat16), prompt["intrinsic"].to(dev, torch.bfloat16)
    cache = m.new_cache(B, P + n)
    pos = torch.arange(P, device=dev)
    toks, margins = [], []
    try:
        with torch.no_grad():
            for i in range(n):
                mi = m.prepare_inputs_for_generation(ids, past_key_values=cache, cache_position=pos, pixel_values=pv,
                                                     intrinsic=intr, attention_mask=am)
                mi.pop("cache_position")
                last = m(**mi, return_dict=True).logits[:, -1].float()
                if i == 0:
                    _set_weights(triples, "wprime")
                top2 = last.topk(2, -1).values
                margins.append(top2[:, 0] - top2[:, 1])
                nxt = m.action_argmax().view(B, -1)[:, -1]
                toks.append(nxt)
                ids = torch.cat([ids, nxt[:, None]], 1)
                am = torch.cat([am, torch.ones(B, 1, dtype=am.dtype, device=dev)], 1)
                pos = pos[-1:] + 1
    finally:
        _set_weights(triples, "orig")
    return torch.stack(toks, 1), torch.stack(margins, 1)


def _runs(m, prompt, n):
    runs = {}
    m.clear_decode_cache()
    m.decode_graphs = False
    runs["eager"] = m.predict_action(prompt, max_new_tokens=n, eos_token_id=-1)
    m.decode_graphs = True
    runs["capture"] = m.predict_action(prompt, max_new_tokens=n, eos_token_id=-1)
    runs["replay"] = m.predict_action(prompt, max_new_tokens=n, eos_token_id=-1)
    P = prompt["input_ids"].shape[1]
    kw = {k: v for k, v in prompt.items()}
    gen = m.generate(**kw, max_new_tokens=n, eos_token_id=-1)
    assert gen.shape[1] == P + n and torch.equal(gen[:, :P].cpu(), prompt["input_ids"].cpu())
    runs["generate"] = gen[:, P:]
    return runs


def test_tokens(ctx):
    m = ctx["fp8"]
    ref, margins = _ref_greedy(ctx["ref"], ctx["ref_w"], ctx["prompt"], N_NEW)
    runs = _runs(m, ctx["prompt"], N_NEW)
    base = ctx["base"].predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    _record(tokens={k: v.tolist() for k, v in runs.items()}, tokens_wprime=ref.tolist(), tokens_bf16=base.tolist(),
            wprime_margins=[[round(float(v), 3) for v in r] for r in margins])
    for k, got in runs.items():
        assert got.shape == (2, N_NEW), k
        n_cmp, n_ok = H.greedy_tokens_agree(got, ref, margins)
        print(f"{k}: {got.tolist()} vs W' {ref.tolist()}: {n_ok}/{n_cmp}")
        _record(**{f"tokens_ok_{k}": [n_ok, n_cmp]})
        assert n_ok >= got.shape[0]  # at least the first token of every row; a disagreement above the margin raises
    for k in ("capture", "replay", "generate"):
        assert torch.equal(runs[k], runs["eager"]), k


def test_tokens_padded_prompt(ctx, cuda):
    g = load_file(os.path.join(os.path.dirname(__file__), "golden", "decode_padded.safetensors"))
    assert bool((g["in.attention_mask"] == 0).any())
    depth = g["out.depth"].to(cuda)
    m, r = ctx["fp8"], ctx["ref"]
    keep = (m.predict_depth, r.predict_depth)
    m.predict_depth = r.predict_depth = lambda p: depth
    try:
        prompt = {"input_ids": g["in.input_ids"], "pixel_values": g["in.pixel_values"], "intrinsic": g["in.intrinsic"]}
        inputs = dict(prompt, attention_mask=g["in.attention_mask"])
        n = 4
        ref, margins = _ref_greedy(r, ctx["ref_w"], prompt, n, attention_mask=g["in.attention_mask"])
        runs = _runs(m, inputs, n)
        _record(padded_tokens={k: v.tolist() for k, v in runs.items()}, padded_tokens_wprime=ref.tolist(),
                padded_wprime_margins=[[round(float(v), 3) for v in row] for row in margins])
        for k, got in runs.items():
            n_cmp, n_ok = H.greedy_tokens_agree(got, ref, margins)
            print(f"padded {k}: {got.tolist()} vs W' {ref.tolist()}: {n_ok}/{n_cmp}")
            assert n_ok >= got.shape[0]
        for k in ("capture", "replay", "generate"):
            assert torch.equal(runs[k], runs["eager"]), k
    finally:
        m.predict_depth, r.predict_depth = keep
        m.clear_decode_cache()


def test_decode_step_runs_the_fp8_gemvs(ctx, monkeypatch):
    """A decode step takes 4 svla_gemv_mxfp8 per layer (q|k|v, o, gate|up, down) and one svla_head_gemv_mxfp8, and none
    of the bf16 decode GEMVs; the prefill takes none of the fp8 kernels."""
    from spatialvla_amd import kernels as Kn
    m = ctx["fp8"]
    calls = {}
    for name in ("gemv_mxfp8", "head_gemv_mxfp8", "gemv_rmsnorm2", "decode_mlp", "linear_fwd", "quant_mx_rows"):
        def wrapped(*a, _f=getattr(Kn, name), _n=name, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(Kn, name, wrapped)
    bd = ctx["bd"]
    ids = bd["input_ids"]
    P = ids.shape[1] - 13
    nl = ctx["cfgd"]["text_config"]["num_hidden_layers"]
    with torch.no_grad():
        cache = m(input_ids=ids[:, :P], pixel_values=bd["pixel_values"], intrinsic=bd["intrinsic"],
                  use_cache=True).past_key_values
        assert calls.get("gemv_mxfp8", 0) == 0 and calls.get("head_gemv_mxfp8", 0) == 0
        calls.clear()
        m(input_ids=ids[:, P:P + 1], past_key_values=cache)
        calls.pop("quant_mx_rows", None)  # the lazily built copies, if this is the model's first fp8 step
        assert calls == {"gemv_mxfp8": 4 * nl, "head_gemv_mxfp8": 1}, calls
        calls.clear()
        m(input_ids=ids[:, P + 1:P + 3], past_key_values=cache)
        assert calls == {"gemv_mxfp8": 4 * nl, "head_gemv_mxfp8": 1}, calls  # the copies are reused


def test_switch_off(ctx):
    """Off again: tokens and logits are bitwise those of a model that never enabled it, and the decode state is
    rebuilt (the switch is part of the state's key)."""
    m = _model(ctx, fp8=True)
    on = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    st_on = next(iter(m._svla_decode_states.values()))
    assert st_on["wptr"][3] is not None and st_on["wptr"][3][0] is True
    m.enable_fp8_decode(False)
    assert len(m._svla_decode_states) == 0
    off = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    st_off = next(iter(m._svla_decode_states.values()))
    assert st_off is not st_on and st_off["wptr"][3] is None
    base = ctx["base"].predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    assert torch.equal(off, base)
    f = _teacher_forced(m, ctx["bd"])
    b = _teacher_forced(ctx["base"], ctx["bd"])
    for k in ("prefill", "step1", "step2"):
        assert torch.equal(f[k], b[k]), k
    _record(tokens_switch_on=on.tolist(), tokens_switch_off=off.tolist())


def test_weight_change(ctx):
    """An in-place weight change: the next decode step's logits follow the new weights (the copy is rebuilt), and the
    captured graphs of predict_action are dropped with it."""
    from spatialvla_amd import functional as Fn
    m = _model(ctx, fp8=True)
    before = _teacher_forced(m, ctx["bd"])
    first = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    st = next(iter(m._svla_decode_states.values()))
    builds = Fn.FP8DecodeWeights.BUILDS[0]
    again = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    assert next(iter(m._svla_decode_states.values())) is st and Fn.FP8DecodeWeights.BUILDS[0] == builds  # replayed
    assert torch.equal(again, first)
    down = m.language_model.model.layers[-1].mlp.down_proj.weight
    with torch.no_grad():
        down.mul_(-1)
    triples = _quantised_weights(m)
    after = _teacher_forced(m, ctx["bd"])
    assert Fn.FP8DecodeWeights.BUILDS[0] == builds + 1  # the one copy whose weight changed
    try:
        want = _teacher_forced(m, ctx["bd"], lambda: (m.enable_fp8_decode(False), _set_weights(triples, "wprime")))
    finally:
        _set_weights(triples, "orig")
        m.enable_fp8_decode(True)
    moved = H.rel_l2(after["step1"], before["step1"])
    rel = H.rel_l2(after["step1"], want["step1"])
    _record(weight_change_moved_rel=moved, weight_change_vs_wprime_rel=rel)
    assert moved > 10 * H.LOGITS_TOL and rel < H.LOGITS_TOL
    graphs = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    assert next(iter(m._svla_decode_states.values())) is not st  # re-captured on the rebuilt copies
    m.decode_graphs = False
    eager = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    assert torch.equal(graphs, eager)
