"""Weight-only fp8 decode under unmerged adapters (enable_fp8_lora_decode) on the tiny model, batch 2, in the pattern
of test_fp8_decode_model_gpu.py: the reference is the same adapter model on the bf16 enable_lora_decode() path whose
base weights are overwritten in place, after the prefill, with W' = the exact bf16 dequantisation of the e4m3 copies --
so the two differ in the decode steps' summation order only.  Every measured distance goes to
profiles/fp8_lora_decode_tiny.json before it is asserted."""
import os

import pytest
import torch
from safetensors.torch import load_file

import harness as H
from test_fp8_decode_model_gpu import (_gated_argmax_equal, _quantised_weights, _ref_greedy, _runs, _set_weights,
                                       _teacher_forced)

pytestmark = pytest.mark.gpu
R, ALPHA, SEED, N_NEW = 8, 16.0, 7, 6
EMB_H = "spatialvla-linear+emb+h"
_RECORDED = {}


def _record(**kv):
    from test_full4b_gpu import _dump
    _RECORDED.update(kv)
    _dump("fp8_lora_decode_tiny.json", _RECORDED)


def _set_adapters(m, seed):
    """Non-zero A and B on every attached adapter, from one CPU generator: A ~ N(0, 1/r^2), B ~ N(0, 0.02^2); the
    Embedding adapter A ~ N(0, 0.01^2), B ~ N(0, 1) (peft's B init, A moved off zero)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in list(m.modules()):
            ad = getattr(mod, "lora", None)
            if ad is None:
                continue
            emb = isinstance(mod, torch.nn.Embedding)
            ad.A.copy_((torch.randn(ad.A.shape, generator=g) * (0.01 if emb else 1.0 / ad.r)).to(ad.A.dtype))
            ad.B.copy_((torch.randn(ad.B.shape, generator=g) * (1.0 if emb else 0.02)).to(ad.B.dtype))


def _model(ctx, fp8=False, targets="gemma2-linear", ad_seed=11):
    m = H.build_hip_model(ctx["cfgd"], "cuda:0")
    m.predict_depth = lambda pv, _d=ctx["depth"]: _d  # device tensor: no host copy inside a graph capture
    m.add_lora(R, ALPHA, target_modules=targets, seed=0)
    _set_adapters(m, ad_seed)
    m.enable_lora_decode(True, emb_head=targets == EMB_H)
    if fp8:
        m.enable_fp8_lora_decode()
    return m


def _builds(m):
    return sum(h.builds for h in m.language_model.fp8_lora_decode_holders())


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
    c["base"] = _model(c)            # the bf16 adapter GEMVs on the bf16 weights
    c["fp8"] = _model(c, fp8=True)
    c["ref"] = _model(c)             # the bf16 adapter GEMVs, its base weights W' after the prefill
    c["ref_w"] = _quantised_weights(c["ref"])
    return c


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
    # the first greedy token comes from the prefill's bf16 head: no e4m3 copy is read there
    m = ctx["fp8"]
    m.decode_graphs = False
    a = m.predict_action(ctx["prompt"], max_new_tokens=1, eos_token_id=-1)
    b = ctx["base"].predict_action(ctx["prompt"], max_new_tokens=1, eos_token_id=-1)
    m.decode_graphs = True
    assert torch.equal(a, b)
    assert m.fp8_lora_decode and not m.fp8_decode


def test_kernel_path_equals_dequantised_bf16_adapter_path(forced):
    f, r = forced["fp8"], forced["ref"]
    rel = {b: H.rel_l2(f[b], r[b]) for b in ("step1", "step2")}
    moved = {b: H.rel_l2(r[b], forced["base"][b]) for b in ("step1", "step2")}
    _record(kernel_vs_wprime_rel=rel, wprime_vs_bf16_rel=moved)
    print(f"e4m3 adapter GEMVs vs W' on the bf16 adapter path: {rel}; W' vs the bf16 weights: {moved}")
    assert min(moved.values()) > 1e-4  # the reference does run on other weights than the bf16 model
    for b, v in rel.items():
        assert v < H.LOGITS_TOL, (b, v)
        _gated_argmax_equal(f[b], r[b], b)


def _check_tokens(runs, ref, margins, tag):
    for k, got in runs.items():
        assert got.shape == ref.shape, k
        n_cmp, n_ok = H.greedy_tokens_agree(got, ref, margins)
        print(f"{tag}{k}: {got.tolist()} vs W' {ref.tolist()}: {n_ok}/{n_cmp}")
        _record(**{f"{tag}tokens_ok_{k}": [n_ok, n_cmp]})
        assert n_ok >= got.shape[0]  # at least the first token of every row; a disagreement above the margin raises
    for k in ("capture", "replay", "generate"):
        assert torch.equal(runs[k], runs["eager"]), k


def test_tokens(ctx):
    ref, margins = _ref_greedy(ctx["ref"], ctx["ref_w"], ctx["prompt"], N_NEW)
    runs = _runs(ctx["fp8"], ctx["prompt"], N_NEW)
    base = ctx["base"].predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    _record(tokens={k: v.tolist() for k, v in runs.items()}, tokens_wprime=ref.tolist(), tokens_bf16=base.tolist(),
            wprime_margins=[[round(float(v), 3) for v in r] for r in margins])
    _check_tokens(runs, ref, margins, "")


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
        ref, margins = _ref_greedy(r, ctx["ref_w"], prompt, 4, attention_mask=g["in.attention_mask"])
        runs = _runs(m, inputs, 4)
        _record(padded_tokens={k: v.tolist() for k, v in runs.items()}, padded_tokens_wprime=ref.tolist())
        _check_tokens(runs, ref, margins, "padded_")
    finally:
        m.predict_depth, r.predict_depth = keep
        m.clear_decode_cache()


def _count_calls(monkeypatch, names):
    from spatialvla_amd import kernels as Kn
    calls = {}
    for name in names:
        def wrapped(*a, _f=getattr(Kn, name), _n=name, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(Kn, name, wrapped)
    return calls


WATCHED = ("lora_gemv_mxfp8", "lora_head_gemv_mxfp8", "lora_gemv", "lora_head_gemv", "lora_gemv_down", "gemv_mxfp8",
           "head_gemv_mxfp8", "linear_fwd", "quant_mx_rows")


def _step_calls(m, ctx, calls):
    bd = ctx["bd"]
    ids = bd["input_ids"]
    P = ids.shape[1] - 13
    with torch.no_grad():
        cache = m(input_ids=ids[:, :P], pixel_values=bd["pixel_values"], intrinsic=bd["intrinsic"],
                  use_cache=True).past_key_values
        for k in ("lora_gemv_mxfp8", "lora_head_gemv_mxfp8", "gemv_mxfp8", "head_gemv_mxfp8"):
            assert calls.get(k, 0) == 0, k  # the prefill takes none of the e4m3 kernels
        calls.clear()
        m(input_ids=ids[:, P:P + 1], past_key_values=cache)
        calls.pop("quant_mx_rows", None)  # the lazily built copies, if this is the model's first such step
        first = dict(calls)
        calls.clear()
        m(input_ids=ids[:, P + 1:P + 3], past_key_values=cache)
        return first, dict(calls)


def test_decode_step_runs_the_e4m3_adapter_gemvs(ctx, monkeypatch):
    """A decode step takes 4 svla_lora_gemv_down + 4 svla_lora_gemv_mxfp8 per layer and, without a head adapter, the
    head of enable_fp8_decode; no bf16 svla_lora_gemv; the copies are reused by the next step."""
    calls = _count_calls(monkeypatch, WATCHED)
    nl = ctx["cfgd"]["text_config"]["num_hidden_layers"]
    want = {"lora_gemv_down": 4 * nl, "lora_gemv_mxfp8": 4 * nl, "head_gemv_mxfp8": 1}
    first, second = _step_calls(ctx["fp8"], ctx, calls)
    assert first == want, first
    assert second == want, second


def test_emb_head_set(ctx, monkeypatch):
    """The "+emb+h" set under enable_lora_decode(True, emb_head=True): greedy tokens against the W' reference, and the
    head as svla_lora_gemv_down + svla_lora_head_gemv_mxfp8."""
    m = _model(ctx, fp8=True, targets=EMB_H, ad_seed=12)
    r = _model(ctx, targets=EMB_H, ad_seed=12)
    triples = _quantised_weights(r)
    ref, margins = _ref_greedy(r, triples, ctx["prompt"], N_NEW)
    runs = _runs(m, ctx["prompt"], N_NEW)
    _record(emb_h_tokens={k: v.tolist() for k, v in runs.items()}, emb_h_tokens_wprime=ref.tolist())
    _check_tokens(runs, ref, margins, "emb_h_")
    calls = _count_calls(monkeypatch, WATCHED)
    nl = ctx["cfgd"]["text_config"]["num_hidden_layers"]
    first, _ = _step_calls(m, ctx, calls)
    assert first == {"lora_gemv_down": 4 * nl + 1, "lora_gemv_mxfp8": 4 * nl, "lora_head_gemv_mxfp8": 1}, first


def test_copies_survive_adapter_updates_and_swaps(ctx, tmp_path):
    nl = ctx["cfgd"]["text_config"]["num_hidden_layers"]
    m = _model(ctx, fp8=True)
    first = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    st = next(iter(m._svla_decode_states.values()))
    assert st["wptr"][4] == (True, 4 * nl + 1) and _builds(m) == 4 * nl + 1
    before = _teacher_forced(m, ctx["bd"])
    # A / B updated in place (an optimizer step on the adapters): nothing is rebuilt, the graphs read them in place
    with torch.no_grad():
        for _, lin in m._lora_linears():
            lin.lora.B.mul_(1.5)
    again = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    assert _builds(m) == 4 * nl + 1 and next(iter(m._svla_decode_states.values())) is st
    m.decode_graphs = False
    eager = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    m.decode_graphs = True
    assert torch.equal(again, eager)
    # load_lora of a second adapter directory over the attached set: copied in place, no copy rebuilt, and the decode
    # is that adapter's (the W' reference with the same adapters)
    other = _model(ctx, ad_seed=23)
    other.save_lora(str(tmp_path))
    m.load_lora(str(tmp_path))
    assert m.fp8_lora_decode and _builds(m) == 4 * nl + 1
    after = _teacher_forced(m, ctx["bd"])
    moved = H.rel_l2(after["step1"], before["step1"])
    ref, margins = _ref_greedy(other, _quantised_weights(other), ctx["prompt"], N_NEW)
    got = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    n_cmp, n_ok = H.greedy_tokens_agree(got, ref, margins)
    _record(load_lora_moved_rel=moved, load_lora_tokens=got.tolist(), load_lora_tokens_wprime=ref.tolist(),
            tokens_first_adapter=first.tolist())
    assert _builds(m) == 4 * nl + 1
    assert moved > 1e-3 and n_ok >= got.shape[0]


def test_base_weight_change_rebuilds_and_drops_the_graphs(ctx):
    nl = ctx["cfgd"]["text_config"]["num_hidden_layers"]
    m = _model(ctx, fp8=True)
    m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    st = next(iter(m._svla_decode_states.values()))
    down = m.language_model.model.layers[-1].mlp.down_proj.weight
    with torch.no_grad():
        down.mul_(-1)
    graphs = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    st2 = next(iter(m._svla_decode_states.values()))
    assert _builds(m) == 4 * nl + 2 and st2 is not st and st2["wptr"][4] == (True, 4 * nl + 2)
    m.decode_graphs = False
    eager = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    assert torch.equal(graphs, eager)


@pytest.mark.parametrize("how", ["fp8_lora_decode_off", "lora_decode_off", "merge"])
def test_switch_off(ctx, how):
    m = _model(ctx, fp8=True)
    on = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    assert next(iter(m._svla_decode_states.values()))["wptr"][4][0] is True
    if how == "fp8_lora_decode_off":
        m.enable_fp8_lora_decode(False)
    elif how == "lora_decode_off":
        m.enable_lora_decode(False)
        m.enable_lora_decode(True)
    else:
        m.merge_lora()
    assert not m.fp8_lora_decode and m.language_model.fp8_lora_decode_holders() == []
    assert len(m._svla_decode_states) == 0
    off = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    assert next(iter(m._svla_decode_states.values()))["wptr"][4] is None
    _record(**{f"tokens_{how}": off.tolist(), "tokens_switch_on": on.tolist()})
    if how != "merge":  # the bf16 unmerged path again, bit for bit
        base = ctx["base"].predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
        assert torch.equal(off, base)
        f, b = _teacher_forced(m, ctx["bd"]), _teacher_forced(ctx["base"], ctx["bd"])
        for k in ("prefill", "step1", "step2"):
            assert torch.equal(f[k], b[k]), k
