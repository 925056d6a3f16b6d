"""Batched decode (enable_batched_decode) on the tiny model with 12 sequences: the prefill is untouched, the decode
steps of 12 and 24 rows agree with the switch-off model and with the uncached forward, greedy tokens of predict_action
(eager, captured, replayed) and generate, the dispatch window and the switch."""
import os

import pytest
import torch
from safetensors.torch import load_file

import harness as H

pytestmark = pytest.mark.gpu
SEED, N_NEW, BATCH = 7, 6, 12


def _depth_for(d):
    """predict_depth stand-in: the fixed depth maps of the batch, cycled for other batch sizes (device tensors only: no
    host copy inside a graph capture)."""
    def f(pv, _d=d):
        n = pv.shape[0]
        return _d[:n] if n <= _d.shape[0] else torch.cat([_d, _d[:n - _d.shape[0]]], 0)
    return f


def _model(ctx, on=False):
    m = H.build_hip_model(ctx["cfgd"], "cuda:0")
    m.predict_depth = _depth_for(ctx["depth"])
    if on:
        m.enable_batched_decode()
    return m


@pytest.fixture(scope="module")
def ctx(cuda):
    from spatialvla_amd import presets
    cfgd = H.cfg_dict("tiny")
    bd = H.batch_tensors(presets.synthetic_batch(cfgd, batch=BATCH, seed=SEED), cuda)
    c = dict(cfgd=cfgd, bd=bd)
    probe = H.build_hip_model(cfgd, "cuda:0")
    with torch.no_grad():
        c["depth"] = probe.predict_depth(bd["pixel_values"]).clone()
    c["prompt"] = {"input_ids": bd["input_ids"][:, :-13], "pixel_values": bd["pixel_values"],
                   "intrinsic": bd["intrinsic"]}
    c["base"] = _model(c)
    c["on"] = _model(c, on=True)
    return c


def _teacher_forced(model, bd, rows=slice(None), steps=(1, 2)):
    """Prefill with use_cache=True, then steps of 1 and 2 tokens through past_key_values."""
    ids = bd["input_ids"][rows]
    P = ids.shape[1] - 13
    out = {"P": P}
    with torch.no_grad():
        o1 = model(input_ids=ids[:, :P], pixel_values=bd["pixel_values"][rows], intrinsic=bd["intrinsic"][rows],
                   use_cache=True)
        cache = o1.past_key_values
        out["prefill"] = o1.logits.clone()
        p = P
        for i, n in enumerate(steps):
            out[f"step{i + 1}"] = model(input_ids=ids[:, p:p + n], past_key_values=cache).logits.clone()
            p += n
        assert cache.get_seq_length() == p
    return out


@pytest.fixture(scope="module")
def forced(ctx):
    return {k: _teacher_forced(ctx[k], ctx["bd"]) for k in ("base", "on")}


def test_switch_default_and_prefill_untouched(ctx, forced):
    assert ctx["base"].batched_decode is False and ctx["on"].batched_decode is True
    assert torch.equal(forced["on"]["prefill"], forced["base"]["prefill"])


def test_teacher_forced_steps(ctx, forced):
    from spatialvla_amd.modeling_gemma2 import KVMask
    bd = ctx["bd"]
    ids = bd["input_ids"]
    P = forced["on"]["P"]
    cls = torch.ones(BATCH, P + 3, dtype=torch.uint8, device=ids.device)
    cls[:, :P] = 0
    with torch.no_grad():
        unc = ctx["base"](input_ids=ids[:, :P + 3], pixel_values=bd["pixel_values"], intrinsic=bd["intrinsic"],
                          kv_mask=KVMask(cls)).logits[:, P:].clone()
    got = torch.cat([forced["on"]["step1"], forced["on"]["step2"]], 1)
    off = torch.cat([forced["base"]["step1"], forced["base"]["step2"]], 1)
    assert got.shape == off.shape == unc.shape == (BATCH, 3, unc.shape[-1])
    assert not torch.equal(got, off)  # another summation order: the new kernels did run
    for name, ref in (("switch off", off), ("uncached", unc)):
        rel = H.rel_l2(got, ref)
        top2 = ref.float().topk(2, -1).values
        conf = (top2[..., 0] - top2[..., 1]) > H.MARGIN
        agree = got.float().argmax(-1) == ref.float().argmax(-1)
        frac = float(conf.float().mean())
        print(f"vs {name}: rel-L2 {rel:.3e}, confident {int(conf.sum())}/{conf.numel()}, "
              f"argmax agree {int(agree.sum())}/{agree.numel()}")
        assert rel < H.LOGITS_TOL, (name, rel)
        assert bool(agree[conf].all()), name
        assert frac >= 2.0 / 3.0, (name, frac)  # not a vacuous pass


def _ref_greedy(m, prompt, n, attention_mask=None):
    """The switch-off model's greedy decode through prepare_inputs_for_generation -> forward per step: tokens [B, n]
    and the top-2 margin of every step's logits."""
    dev = m.language_model.lm_head.weight.device
    ids = prompt["input_ids"].to(dev)
    B, P = ids.shape
    am = attention_mask.to(dev) if attention_mask is not None else torch.ones(B, P, dtype=torch.int64, device=dev)
    pv, intr = prompt["pixel_values"].to(dev, torch.bfloat16), prompt["intrinsic"].to(dev, torch.bfloat16)
    cache = m.new_cache(B, P + n)
    pos = torch.arange(P, device=dev)
    toks, margins = [], []
    with torch.no_grad():
        for i in range(n):
            mi = m.prepare_inputs_for_generation(ids, past_key_values=cache, cache_position=pos, pixel_values=pv,
                                                 intrinsic=intr, attention_mask=am)
            mi.pop("cache_position")
            last = m(**mi, return_dict=True).logits[:, -1].float()
            top2 = last.topk(2, -1).values
            margins.append(top2[:, 0] - top2[:, 1])
            nxt = m.action_argmax().view(B, -1)[:, -1]
            toks.append(nxt)
            ids = torch.cat([ids, nxt[:, None]], 1)
            am = torch.cat([am, torch.ones(B, 1, dtype=am.dtype, device=dev)], 1)
            pos = pos[-1:] + 1
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
    gen = m.generate(**dict(prompt), max_new_tokens=n, eos_token_id=-1)
    assert gen.shape[1] == P + n and torch.equal(gen[:, :P].cpu(), prompt["input_ids"].cpu())
    runs["generate"] = gen[:, P:]
    return runs


def _check_runs(runs, ref, margins, B, n):
    for k, got in runs.items():
        assert got.shape == (B, n), k
        n_cmp, n_ok = H.greedy_tokens_agree(got, ref, margins)
        print(f"{k}: {n_ok}/{n_cmp} tokens equal to the switch-off model's")
        assert n_ok >= B  # at least the first token of every row; a disagreement above the margin raises
    for k in ("capture", "replay", "generate"):
        assert torch.equal(runs[k], runs["eager"]), k


def test_tokens(ctx):
    ref, margins = _ref_greedy(ctx["base"], ctx["prompt"], N_NEW)
    _check_runs(_runs(ctx["on"], ctx["prompt"], N_NEW), ref, margins, BATCH, N_NEW)


def test_tokens_padded_prompt(ctx, cuda):
    g = load_file(os.path.join(os.path.dirname(__file__), "golden", "decode_padded.safetensors"))
    assert bool((g["in.attention_mask"] == 0).any())
    rep = -(-BATCH // g["in.input_ids"].shape[0])

    def rows(t):
        return t.repeat(rep, *([1] * (t.dim() - 1)))[:BATCH].contiguous()

    depth = rows(g["out.depth"]).to(cuda)
    m, r = ctx["on"], ctx["base"]
    keep = (m.predict_depth, r.predict_depth)
    m.predict_depth = r.predict_depth = _depth_for(depth)
    try:
        prompt = {"input_ids": rows(g["in.input_ids"]), "pixel_values": rows(g["in.pixel_values"]),
                  "intrinsic": rows(g["in.intrinsic"])}
        am = rows(g["in.attention_mask"])
        n = 4
        ref, margins = _ref_greedy(r, prompt, n, attention_mask=am)
        _check_runs(_runs(m, dict(prompt, attention_mask=am), n), ref, margins, BATCH, n)
    finally:
        m.predict_depth, r.predict_depth = keep
        m.clear_decode_cache()


def _count(monkeypatch):
    from spatialvla_amd import kernels as Kn
    calls = {"n": 0}

    def wrapped(*a, _f=Kn.gemm_skinny, **kw):
        calls["n"] += 1
        return _f(*a, **kw)
    monkeypatch.setattr(Kn, "gemm_skinny", wrapped)
    return calls


def test_dispatch_window(ctx, forced, monkeypatch):
    """12 and 24 rows call the wrapper (q|k|v and o of every layer), the prefill and 8 rows do not; the 8-row logits
    are bitwise those of a model that never saw the switch; 65 rows (B = 13, Lq = 5) keep the old path.
    The 65-row step is checked for its path and shape only: on the general path, with the switch on or off, its
    logits for the thirteenth sequence came out NaN in some runs and finite in others while this test was written
    (the input is the 12-sequence batch plus a copy of its first sequence, the depth maps cycled the same way); that
    instability is in code this switch does not touch and is not looked into here."""
    m, bd = ctx["on"], ctx["bd"]
    nl = ctx["cfgd"]["text_config"]["num_hidden_layers"]
    per_step = 2 * nl
    calls = _count(monkeypatch)
    ids = bd["input_ids"]
    P = ids.shape[1] - 13
    with torch.no_grad():
        cache = m(input_ids=ids[:, :P], pixel_values=bd["pixel_values"], intrinsic=bd["intrinsic"],
                  use_cache=True).past_key_values
        assert calls["n"] == 0
        m(input_ids=ids[:, P:P + 1], past_key_values=cache)
        assert calls["n"] == per_step
        m(input_ids=ids[:, P + 1:P + 3], past_key_values=cache)
        assert calls["n"] == 2 * per_step
    calls["n"] = 0
    eight = _teacher_forced(m, bd, rows=slice(0, 8), steps=(1, 1))
    assert calls["n"] == 0
    never = _teacher_forced(ctx["base"], bd, rows=slice(0, 8), steps=(1, 1))
    for k in ("prefill", "step1", "step2"):
        assert torch.equal(eight[k], never[k]), k
    big = {k: torch.cat([v, v[:1]], 0) for k, v in bd.items() if k in ("input_ids", "pixel_values", "intrinsic")}
    out = _teacher_forced(m, big, steps=(5,))  # 65 rows: the general path, untouched by the switch
    assert calls["n"] == 0 and out["step1"].shape[:2] == (13, 5)


def test_toggle_recaptures(ctx):
    m = _model(ctx, on=True)
    on = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    st_on = next(iter(m._svla_decode_states.values()))
    assert st_on["wptr"][5:] == ("batched",) and len(st_on["graphs"]) > 0
    m.enable_batched_decode(False)
    assert len(m._svla_decode_states) == 0
    off = m.predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    st_off = next(iter(m._svla_decode_states.values()))
    assert st_off is not st_on and len(st_off["wptr"]) == 5 and len(st_off["graphs"]) > 0
    base = ctx["base"].predict_action(ctx["prompt"], max_new_tokens=N_NEW, eos_token_id=-1)
    assert torch.equal(off, base)
    assert on.shape == off.shape
