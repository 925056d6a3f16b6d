"""Sampled decode (enable_sampled_decode) on the tiny model, 12 new tokens: greedy tokens unchanged, bitwise
reproducibility per seed with and without the step graphs, the allowed-range constraint, batched and fp8 decode, and
generate(do_sample=True)."""
import pytest
import torch

import harness as H

pytestmark = pytest.mark.gpu
SEED, N_NEW = 7, 12
RANGES = [(513, 543), (543, 573), (573, 577)]  # processor-style: translation, rotation, gripper of the tiny vocabulary


def _depth_for(d):
    def f(pv, _d=d):
        n = pv.shape[0]
        return _d[:n] if n <= _d.shape[0] else torch.cat([_d, _d[:n - _d.shape[0]]], 0)
    return f


def _model(ctx, sampled=True):
    m = H.build_hip_model(ctx["cfgd"], "cuda:0")
    m.predict_depth = _depth_for(ctx["depth"])
    if sampled:
        m.enable_sampled_decode()
    return m


@pytest.fixture(scope="module")
def ctx(cuda):
    from spatialvla_amd import presets
    cfgd = H.cfg_dict("tiny")
    bd = H.batch_tensors(presets.synthetic_batch(cfgd, batch=9, seed=SEED), cuda)
    c = dict(cfgd=cfgd, bd=bd)
    probe = H.build_hip_model(cfgd, "cuda:0")
    with torch.no_grad():
        c["depth"] = probe.predict_depth(bd["pixel_values"]).clone()
    c["base"] = _model(c, sampled=False)
    c["on"] = _model(c)
    return c


def _prompt(ctx, B):
    bd = ctx["bd"]
    return {"input_ids": bd["input_ids"][:B, :-13], "pixel_values": bd["pixel_values"][:B],
            "intrinsic": bd["intrinsic"][:B]}


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_greedy_unchanged(ctx):
    want = ctx["base"].predict_action(_prompt(ctx, 2), max_new_tokens=N_NEW, eos_token_id=-1)
    toks, lp, lpr = ctx["on"].predict_action(_prompt(ctx, 2), max_new_tokens=N_NEW, eos_token_id=-1,
                                             return_logprobs=True)
    assert torch.equal(toks, want) and toks.shape == (2, N_NEW)
    assert lp.shape == lpr.shape == (2, N_NEW) and lp.dtype == lpr.dtype == torch.float32
    assert torch.equal(lp, lpr) and bool((lp < 0).all())  # greedy, no range: both are the raw log-softmax
    assert torch.equal(ctx["on"].predict_action(_prompt(ctx, 2), max_new_tokens=N_NEW, eos_token_id=-1), want)


def test_logprobs_are_the_log_softmax_of_the_steps_logits(ctx):
    """logprob_raw of a sampled token against the teacher-forced forward's logits at that position."""
    m, pr = ctx["on"], _prompt(ctx, 2)
    toks, lp, lpr = m.predict_action(pr, max_new_tokens=4, eos_token_id=-1, do_sample=True, temperature=2.0, seed=3,
                                     return_logprobs=True)
    with torch.no_grad():
        o = m(input_ids=pr["input_ids"], pixel_values=pr["pixel_values"], intrinsic=pr["intrinsic"], use_cache=True)
        logits = [o.logits[:, -1].float()]
        for i in range(3):
            logits.append(m(input_ids=toks[:, i:i + 1], past_key_values=o.past_key_values).logits[:, -1].float())
    for i, lg in enumerate(logits):
        ref = torch.log_softmax(lg.double(), -1).gather(1, toks[:, i:i + 1])[:, 0]
        ref_t = torch.log_softmax(lg.double() / 2.0, -1).gather(1, toks[:, i:i + 1])[:, 0]
        assert float((lpr[:, i].double() - ref).abs().max()) < 2e-6
        assert float((lp[:, i].double() - ref_t).abs().max()) < 2e-6


@pytest.mark.parametrize("graphs", [True, False])
def test_same_seed_same_bits(ctx, graphs):
    m = ctx["on"]
    kw = dict(max_new_tokens=N_NEW, eos_token_id=-1, do_sample=True, temperature=2.0, top_k=40, top_p=0.95, seed=11,
              return_logprobs=True)
    saved = m.decode_graphs
    try:
        ref = m.predict_action(_prompt(ctx, 2), **kw)  # with the step graphs
        m.decode_graphs = graphs
        a = m.predict_action(_prompt(ctx, 2), **kw)
        b = m.predict_action(_prompt(ctx, 2), **kw)
    finally:
        m.decode_graphs = saved
    assert _same(a, b) and _same(a, ref)
    other = m.predict_action(_prompt(ctx, 2), **dict(kw, seed=12))
    assert not torch.equal(other[0], a[0])


def test_unseeded_calls_follow_torch_manual_seed(ctx):
    m = ctx["on"]
    kw = dict(max_new_tokens=N_NEW, eos_token_id=-1, do_sample=True, temperature=2.0)
    torch.manual_seed(5)
    a, b = m.predict_action(_prompt(ctx, 2), **kw), m.predict_action(_prompt(ctx, 2), **kw)
    torch.manual_seed(5)
    c, d = m.predict_action(_prompt(ctx, 2), **kw), m.predict_action(_prompt(ctx, 2), **kw)
    assert torch.equal(a, c) and torch.equal(b, d) and not torch.equal(a, b)


def test_constraint(ctx):
    m = ctx["on"]
    toks, lp, lpr = m.predict_action(_prompt(ctx, 2), max_new_tokens=N_NEW, do_sample=True, temperature=5.0, seed=4,
                                     allowed_ranges=RANGES, return_logprobs=True)
    assert toks.shape == (2, N_NEW)  # eos is never allowed: the loop runs every step
    for i in range(N_NEW):
        lo, hi = RANGES[i % 3]
        assert bool(((toks[:, i] >= lo) & (toks[:, i] < hi)).all()), (i, toks[:, i])
    assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all()) and bool((lpr < 0).all())
    # unconstrained at this temperature the sampler does leave the action ranges
    free = m.predict_action(_prompt(ctx, 2), max_new_tokens=N_NEW, eos_token_id=-1, do_sample=True, temperature=5.0,
                            seed=4)
    assert bool((free < 513).any())
    # constrained greedy
    g = m.predict_action(_prompt(ctx, 2), max_new_tokens=N_NEW, allowed_ranges=RANGES)
    for i in range(N_NEW):
        lo, hi = RANGES[i % 3]
        assert bool(((g[:, i] >= lo) & (g[:, i] < hi)).all())


def test_batched_decode(ctx):
    m = _model(ctx)
    m.enable_batched_decode()
    kw = dict(max_new_tokens=N_NEW, eos_token_id=-1, do_sample=True, temperature=1.5, top_k=8, seed=21,
              return_logprobs=True)
    a = m.predict_action(_prompt(ctx, 9), **kw)
    b = m.predict_action(_prompt(ctx, 9), **kw)
    assert _same(a, b) and a[0].shape == (9, N_NEW)
    # row 0's tokens lie inside the kept sets: the top 8 of the teacher-forced steps' logits
    pr = _prompt(ctx, 9)
    toks = a[0]
    with torch.no_grad():
        o = m(input_ids=pr["input_ids"], pixel_values=pr["pixel_values"], intrinsic=pr["intrinsic"], use_cache=True)
        lg = o.logits[0, -1].float()
        for i in range(N_NEW):
            kth = torch.topk(lg, 8).values[-1]
            assert float(lg[toks[0, i]]) >= float(kth), i
            assert float(a[1][0, i]) <= 0
            if i + 1 < N_NEW:
                lg = m(input_ids=toks[:, i:i + 1], past_key_values=o.past_key_values).logits[0, -1].float()


def test_fp8_decode(ctx):
    m = _model(ctx)
    m.enable_fp8_decode()
    kw = dict(max_new_tokens=N_NEW, eos_token_id=-1, do_sample=True, temperature=2.0, top_p=0.9, seed=31,
              return_logprobs=True)
    a = m.predict_action(_prompt(ctx, 2), **kw)
    b = m.predict_action(_prompt(ctx, 2), **kw)
    assert _same(a, b) and a[0].shape == (2, N_NEW) and bool(torch.isfinite(a[1]).all())


@pytest.mark.parametrize("fp8", [False, True])
def test_lora_decode_both_ends(ctx, fp8):
    """Unmerged adapters on the projections, spatial_embed_tokens and lm_head (svla_lora_head_gemv, and its e4m3 form
    under enable_fp8_lora_decode): the sampler reads the logits those heads write."""
    m = _model(ctx)
    m.add_lora(8, 8.0, target_modules="spatialvla-linear+emb+h", seed=1)
    gen = torch.Generator(device="cpu").manual_seed(2)
    with torch.no_grad():
        ad = m.language_model.lm_head.lora  # B starts at zero: move it so the adapter changes the logits
        ad.B.copy_((torch.randn(ad.B.shape, generator=gen) * 0.05).to(torch.bfloat16))
    m.enable_lora_decode(True, emb_head=True)
    if fp8:
        m.enable_fp8_lora_decode()
    kw = dict(max_new_tokens=N_NEW, do_sample=True, temperature=3.0, seed=41, allowed_ranges=RANGES,
              return_logprobs=True)
    a = m.predict_action(_prompt(ctx, 2), **kw)
    b = m.predict_action(_prompt(ctx, 2), **kw)
    assert _same(a, b) and a[0].shape == (2, N_NEW) and bool(torch.isfinite(a[1]).all())
    for i in range(N_NEW):
        lo, hi = RANGES[i % 3]
        assert bool(((a[0][:, i] >= lo) & (a[0][:, i] < hi)).all())
    g = m.predict_action(_prompt(ctx, 2), max_new_tokens=N_NEW, eos_token_id=-1)
    m.enable_sampled_decode(False)
    assert torch.equal(g, m.predict_action(_prompt(ctx, 2), max_new_tokens=N_NEW, eos_token_id=-1))


def test_generate(ctx):
    m, pr = ctx["on"], _prompt(ctx, 2)
    P = pr["input_ids"].shape[1]
    kw = dict(max_new_tokens=N_NEW, do_sample=True, temperature=2.0, eos_token_id=-1)
    torch.manual_seed(9)
    a = m.generate(**pr, **kw)
    torch.manual_seed(9)
    b = m.generate(**pr, **kw)
    assert a.shape == (2, P + N_NEW) and torch.equal(a[:, :P], pr["input_ids"]) and torch.equal(a, b)
    c = m.generate(**pr, **dict(kw, seed=1))
    assert torch.equal(c, m.generate(**pr, **dict(kw, seed=1))) and not torch.equal(c, a)
    # top_k = 1: every token's logit is the maximum of the step's logits (the sampler read the right rows)
    k1 = m.generate(**pr, **dict(kw, top_k=1, seed=2))[:, P:]
    with torch.no_grad():
        o = m(input_ids=pr["input_ids"], pixel_values=pr["pixel_values"], intrinsic=pr["intrinsic"], use_cache=True)
        lg = o.logits[:, -1].float()
        for i in range(N_NEW):
            assert torch.equal(lg.gather(1, k1[:, i:i + 1])[:, 0], lg.max(1).values), i
            lg = m(input_ids=k1[:, i:i + 1], past_key_values=o.past_key_values).logits[:, -1].float()
    with pytest.raises(NotImplementedError):
        ctx["base"].generate(**pr, max_new_tokens=2, do_sample=True)
