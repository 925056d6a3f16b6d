"""The "spatialvla-linear+emb" / "+emb+h" recipes and modules_to_save on the CPU: the oracle helper
(tests/lora_emb_head_ref.py) against a hand fp32 formula, add_lora's surface and initialisation, the adapter files
(save_lora -> load_lora bit for bit for all four sets with and without the saved table, exact key lists, peft's
alternative key spellings), and the refusals, which leave the model as it was."""
import json
import os

import pytest
import torch

import harness as H
import lora_emb_head_ref as LE

R, ALPHA, SEED = 8, 16.0, 7
S = ALPHA / R
FULL13 = ["q_proj", "o_proj", "k_proj", "v_proj", "gate_proj", "up_proj", "down_proj", "fc1", "fc2", "out_proj",
          "linear", "position_embedding_head.0", "position_embedding_head.3"]
EMB_LIST = FULL13 + ["spatial_embed_tokens"]
EMB_H_LIST = FULL13[:7] + ["lm_head"] + FULL13[7:] + ["spatial_embed_tokens"]
PRE = "base_model.model."


@pytest.fixture()
def cpu_model():
    return H.build_hip_model(H.cfg_dict("tiny"), "cpu")


def _snapshot(m):
    return {n: (p.detach().clone(), p.requires_grad) for n, p in m.named_parameters()}


def _assert_unchanged(m, snap):
    now = dict(m.named_parameters())
    assert now.keys() == snap.keys()
    for n, (v, rg) in snap.items():
        assert torch.equal(now[n].detach(), v) and now[n].requires_grad == rg, n


# ---------------------------------------------------------------------------------------- the oracle helper
def test_oracle_helper_matches_hand_formula():
    import spatialvla_oracle as O
    cfgd = H.cfg_dict("tiny")
    P, _ = H.build_oracle(cfgd)
    ads = LE.make_adapters(P, cfgd, R, SEED)
    A, B = ads[LE.EMB]
    Ah, Bh = ads[LE.HEAD]
    W, Wh = P[LE.EMB_KEY], P[LE.HEAD + ".weight"]
    x = (torch.randn(5, Wh.shape[1], generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16)
    with LE.oracle_lora(P, ads, S):
        eff = P[LE.EMB_KEY]
        assert eff is not W and eff.dtype == torch.bfloat16 and eff.requires_grad
        want = W.detach().float() + S * (B.detach().float() @ A.detach().float()).t()
        # three bf16 roundings (product, scale, sum) of values of the table's magnitude
        assert H.rel_l2(eff.detach(), want) < 3 * 2.0 ** -8
        assert H.rel_l2(eff.detach(), W.detach()) > 0.1  # the adapter moves the table
        y = O._lin(x, Wh)
        yw = x.float() @ Wh.detach().float().t() + S * (x.float() @ Ah.detach().float().t()) @ Bh.detach().float().t()
        assert H.rel_l2(y.detach(), yw) < 4 * 2.0 ** -8
        assert H.rel_l2(y.detach(), x.float() @ Wh.detach().float().t()) > 1e-3
        (eff.float().sum() + y.float().sum()).backward()
    assert P[LE.EMB_KEY] is W  # restored
    for t in (A, B, Ah, Bh):
        assert t.grad is not None and float(t.grad.abs().max()) > 0
    # dA[j, id] = s sum_h B[h, j] for a sum loss
    assert H.rel_l2(A.grad, (S * B.detach().float().sum(0))[:, None].expand_as(A)) < 2.0 ** -6
    # modules_to_save: the oracle's own table, a leaf with a gradient
    W.grad = None
    with LE.oracle_lora(P, {}, S, modules_to_save=True):
        assert P[LE.EMB_KEY] is W and W.requires_grad
    Q = LE.merged_params(P, ads, S)
    assert H.rel_l2(Q[LE.EMB_KEY], want) < 2.0 ** -8 and Q[LE.EMB_KEY].dtype == torch.bfloat16
    assert not torch.equal(Q[LE.HEAD + ".weight"], Wh)


# ---------------------------------------------------------------------------------------- add_lora
def _walk(m, r, seed, emb, head):
    """The documented generator walk, replayed outside the model."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _, lin in m._lora_linears() + m._lora_vision_linears():
        out.append((torch.randn(r, lin.weight.shape[1], generator=gen) / r).to(torch.bfloat16))
    eb = ha = None
    if emb:
        eb = torch.randn(m.spatial_embed_tokens.weight.shape[1], r, generator=gen).to(torch.bfloat16)
    if head:
        ha = (torch.randn(r, m.language_model.lm_head.weight.shape[1], generator=gen) / r).to(torch.bfloat16)
    return out, eb, ha


@pytest.mark.parametrize("name,names,n_ad", [("spatialvla-linear+emb", EMB_LIST, 60),
                                             ("spatialvla-linear+emb+h", EMB_H_LIST, 62)])
def test_add_lora_new_sets(cpu_model, name, names, n_ad):
    m = cpu_model
    keys0 = set(m.state_dict())
    m.add_lora(R, ALPHA, target_modules=name, seed=3)
    assert m.lora_targets == name and m.lora_modules_to_save == []
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    assert len(trainable) == n_ad and all(n.endswith(("lora.A", "lora.B")) for n in trainable)
    assert keys0 <= set(m.state_dict())
    head = name.endswith("+h")
    A_lin, eb, ha = _walk(m, R, 3, True, head)
    for (p, lin), a in zip(m._lora_all_linears(), A_lin):
        assert torch.equal(lin.lora.A, a) and float(lin.lora.B.abs().max()) == 0.0, p
    ad = m.spatial_embed_tokens.lora
    na, Hd = m.spatial_embed_tokens.weight.shape
    assert ad.A.shape == (R, na) and ad.B.shape == (Hd, R) and ad.A.dtype == ad.B.dtype == torch.bfloat16
    assert float(ad.A.abs().max()) == 0.0 and torch.equal(ad.B, eb)  # peft's Embedding init: A = 0, B ~ N(0, 1)
    assert abs(float(ad.B.float().std()) - 1.0) < 0.1
    if head:
        hd = m.language_model.lm_head.lora
        assert torch.equal(hd.A, ha) and float(hd.B.abs().max()) == 0.0
        assert hd.B.shape == (m.language_model.lm_head.weight.shape[0], R)
    else:
        assert not hasattr(m.language_model.lm_head, "lora")
    # the exact name list of the reference selects the same set, in any order
    m2 = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    m2.add_lora(R, ALPHA, target_modules=list(reversed(names)), seed=3)
    assert m2.lora_targets == name and torch.equal(m2.spatial_embed_tokens.lora.B, ad.B)


def test_existing_sets_draw_the_same_bits(cpu_model):
    """The two existing sets under a seed: the bits of the documented walk (what add_lora drew before the new sets
    joined its tail), and the 58 shared adapters are the same values in all sets."""
    m = cpu_model
    m.add_lora(R, ALPHA, target_modules="spatialvla-linear", seed=11)
    A_lin, _, _ = _walk(m, R, 11, False, False)
    assert len(A_lin) == 29
    for (p, lin), a in zip(m._lora_all_linears(), A_lin):
        assert torch.equal(lin.lora.A, a), p
    mg = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    mg.add_lora(R, ALPHA, seed=11)
    assert mg.lora_targets == "gemma2-linear"
    for (p, lin), a in zip(mg._lora_all_linears(), A_lin[:14]):
        assert torch.equal(lin.lora.A, a), p
    assert not hasattr(m.spatial_embed_tokens, "lora") and not hasattr(m.language_model.lm_head, "lora")
    assert not m.spatial_embed_tokens.weight.requires_grad


@pytest.mark.parametrize("mts", [["spatial_embed_tokens"], "spatial_embed_tokens"])
@pytest.mark.parametrize("name,n_ad", [("gemma2-linear", 28), ("spatialvla-linear", 58)])
def test_modules_to_save(cpu_model, name, n_ad, mts):
    m = cpu_model
    m.add_lora(R, ALPHA, target_modules=name, seed=3, modules_to_save=mts)
    assert m.lora_targets == name and m.lora_modules_to_save == ["spatial_embed_tokens"]
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    assert len(trainable) == n_ad + 1 and "spatial_embed_tokens.weight" in trainable
    m3 = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    m3.add_lora(R, ALPHA, target_modules=name, seed=3, modules_to_save=[])
    assert m3.lora_modules_to_save == [] and not m3.spatial_embed_tokens.weight.requires_grad


def test_add_lora_refusals_leave_the_model(cpu_model):
    m = cpu_model
    snap = _snapshot(m)
    with pytest.raises(NotImplementedError, match="lm_head"):
        m.add_lora(R, ALPHA, modules_to_save=["lm_head"])
    with pytest.raises(NotImplementedError, match="embed_tokens"):
        m.add_lora(R, ALPHA, modules_to_save=["spatial_embed_tokens", "embed_tokens"])
    for name in ("spatialvla-linear+emb", "spatialvla-linear+emb+h"):
        with pytest.raises(ValueError, match="modules_to_save"):
            m.add_lora(R, ALPHA, target_modules=name, modules_to_save=["spatial_embed_tokens"])
    with pytest.raises(NotImplementedError, match="lm_head"):  # lm_head without the Embedding adapter is no recipe
        m.add_lora(R, ALPHA, target_modules=FULL13 + ["lm_head"])
    with pytest.raises(NotImplementedError, match="spatial_embed_tokens"):
        m.add_lora(R, ALPHA, target_modules=["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj",
                                             "down_proj", "spatial_embed_tokens"])
    with pytest.raises(NotImplementedError):
        m.add_lora(R, ALPHA, target_modules="linear+emb")
    assert not m.has_lora and m.lora_targets is None and m.lora_modules_to_save == []
    assert not hasattr(m.spatial_embed_tokens, "lora") and not hasattr(m.language_model.lm_head, "lora")
    _assert_unchanged(m, snap)


def test_decode_refusals(cpu_model):
    m = cpu_model
    m.add_lora(R, ALPHA, target_modules="spatialvla-linear+emb+h", seed=1)
    m.clear_decode_cache()
    ids = torch.zeros(1, 4, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match=r"merge_lora\(\)"):
        m.enable_lora_decode(True)
    assert not m.lora_decode
    for call in (lambda: m.predict_action({"input_ids": ids}), lambda: m.generate(input_ids=ids, max_new_tokens=1),
                 lambda: m(input_ids=ids, past_key_values=m.new_cache(1, 8)),
                 lambda: m(input_ids=ids, use_cache=True)):
        with pytest.raises(NotImplementedError, match=r"merge_lora\(\)"):
            with torch.no_grad():
                call()
    assert m.__dict__["_svla_decode_states"] == {}
    m.enable_lora_decode(False)  # turning it off is always allowed
    m.enable_fp8_lora(True)      # neither new site is an fp8 site; the switch keeps working
    assert m.fp8_lora
    m.enable_fp8_lora(False)
    # a modules_to_save table does not block the unmerged decode of the "spatialvla-linear" set
    m2 = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    m2.add_lora(R, ALPHA, target_modules="spatialvla-linear", seed=1, modules_to_save="spatial_embed_tokens")
    m2.enable_lora_decode(True)
    assert m2.lora_decode


# ---------------------------------------------------------------------------------------- adapter files
def _randomise(m, seed=5):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.requires_grad:
                p.copy_((torch.randn(p.shape, generator=gen) * 0.02).to(p.dtype))


def _expected_keys(m, name, table):
    keys = []
    for p, _ in m._lora_linears() + (m._lora_vision_linears() if name != "gemma2-linear" else []):
        keys += [f"{PRE}{p}.lora_A.weight", f"{PRE}{p}.lora_B.weight"]
    if "+emb" in name:
        keys += [PRE + "spatial_embed_tokens.lora_embedding_A", PRE + "spatial_embed_tokens.lora_embedding_B"]
    if name.endswith("+h"):
        keys += [PRE + "language_model.lm_head.lora_A.weight", PRE + "language_model.lm_head.lora_B.weight"]
    if table:
        keys.append(PRE + "spatial_embed_tokens.weight")
    return sorted(keys)


CASES = [("gemma2-linear", False), ("gemma2-linear", True), ("spatialvla-linear", False), ("spatialvla-linear", True),
         ("spatialvla-linear+emb", False), ("spatialvla-linear+emb+h", False)]
LISTS = {"gemma2-linear": ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"],
         "spatialvla-linear": FULL13, "spatialvla-linear+emb": EMB_LIST, "spatialvla-linear+emb+h": EMB_H_LIST}


@pytest.mark.parametrize("name,table", CASES)
def test_save_load_round_trip(cpu_model, tmp_path, name, table):
    from safetensors.torch import load_file
    m = cpu_model
    m.add_lora(R, ALPHA, target_modules=name, seed=5, modules_to_save=["spatial_embed_tokens"] if table else None)
    _randomise(m)
    d = str(tmp_path / "a")
    m.save_lora(d)
    cfg = json.load(open(os.path.join(d, "adapter_config.json")))
    assert cfg["target_modules"] == LISTS[name]
    assert cfg["modules_to_save"] == (["spatial_embed_tokens"] if table else None)
    assert cfg["r"] == R and cfg["lora_alpha"] == ALPHA and cfg["peft_type"] == "LORA"
    tens = load_file(os.path.join(d, "adapter_model.safetensors"))
    assert sorted(tens) == _expected_keys(m, name, table)
    m2 = H.build_hip_model(H.cfg_dict("tiny"), "cpu", seed=H.SEED + 1)  # another base: the table must come from the file
    base2 = _snapshot(m2)
    m2.load_lora(d)
    assert m2.lora_targets == name and m2.lora_modules_to_save == (["spatial_embed_tokens"] if table else [])
    mine, theirs = dict(m.named_parameters()), dict(m2.named_parameters())
    assert mine.keys() == theirs.keys()
    for n, p in mine.items():
        assert theirs[n].requires_grad == p.requires_grad, n
        if p.requires_grad:
            assert torch.equal(theirs[n], p), n
        else:
            assert torch.equal(theirs[n].detach(), base2[n][0]), n  # frozen weights are not the file's business
    if "+emb" in name:
        assert m2.spatial_embed_tokens.lora.scaling == S
    # loading the same file again into the model that holds the set is allowed; another set is refused
    m2.load_lora(d)
    other = "gemma2-linear" if name != "gemma2-linear" else "spatialvla-linear"
    m3 = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    m3.add_lora(R, ALPHA, target_modules=other, seed=1)
    snap = _snapshot(m3)
    with pytest.raises(ValueError, match=name.replace("+", r"\+")):
        m3.load_lora(d)
    assert m3.lora_targets == other
    _assert_unchanged(m3, snap)


def _write(tmp_path, name, tensors, cfg):
    from safetensors.torch import save_file
    dd = str(tmp_path / name)
    os.makedirs(dd)
    save_file({k: v.clone() for k, v in tensors.items()}, os.path.join(dd, "adapter_model.safetensors"))
    json.dump(cfg, open(os.path.join(dd, "adapter_config.json"), "w"))
    return dd


def test_alternative_spellings_and_bad_files(cpu_model, tmp_path):
    from safetensors.torch import load_file
    m = cpu_model
    m.add_lora(R, ALPHA, target_modules="spatialvla-linear", seed=5, modules_to_save=["spatial_embed_tokens"])
    _randomise(m)
    d = str(tmp_path / "a")
    m.save_lora(d)
    cfg = json.load(open(os.path.join(d, "adapter_config.json")))
    tens = load_file(os.path.join(d, "adapter_model.safetensors"))
    tk = PRE + "spatial_embed_tokens.weight"
    for i, alt in enumerate(("spatial_embed_tokens.modules_to_save.weight",
                             "spatial_embed_tokens.modules_to_save.default.weight")):
        t2 = {k: v for k, v in tens.items() if k != tk}
        t2[PRE + alt] = tens[tk]
        # peft's unstripped adapter names on the linears too
        t2 = {k.replace(".lora_A.weight", ".lora_A.default.weight").replace(".lora_B.weight", ".lora_B.default.weight"): v
              for k, v in t2.items()}
        m2 = H.build_hip_model(H.cfg_dict("tiny"), "cpu", seed=H.SEED + 1)
        m2.load_lora(_write(tmp_path, f"alt{i}", t2, cfg))
        assert m2.lora_modules_to_save == ["spatial_embed_tokens"]
        assert torch.equal(m2.spatial_embed_tokens.weight, m.spatial_embed_tokens.weight)
        assert torch.equal(m2.multi_modal_projector.linear.lora.B, m.multi_modal_projector.linear.lora.B)
    fresh = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    snap = _snapshot(fresh)
    # the table under two spellings, a table the config does not announce, an announced table that is missing,
    # another module in modules_to_save: refused, keys listed, model untouched
    with pytest.raises(ValueError, match=r"spatial_embed_tokens\.(modules_to_save\.)?weight"):
        fresh.load_lora(_write(tmp_path, "twice", {**tens, PRE + "spatial_embed_tokens.modules_to_save.weight": tens[tk]},
                               cfg))
    with pytest.raises(ValueError, match="spatial_embed_tokens"):
        fresh.load_lora(_write(tmp_path, "unannounced", tens, {**cfg, "modules_to_save": None}))
    with pytest.raises(ValueError, match="modules_to_save"):
        fresh.load_lora(_write(tmp_path, "absent", {k: v for k, v in tens.items() if k != tk}, cfg))
    with pytest.raises(NotImplementedError, match="lm_head"):
        fresh.load_lora(_write(tmp_path, "other", tens, {**cfg, "modules_to_save": ["lm_head"]}))
    assert not fresh.has_lora
    _assert_unchanged(fresh, snap)

    # "+emb+h" files: an incomplete Embedding adapter, a table beside the Embedding adapter, a wrong shape
    mh = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    mh.add_lora(R, ALPHA, target_modules="spatialvla-linear+emb+h", seed=5)
    _randomise(mh)
    dh = str(tmp_path / "h")
    mh.save_lora(dh)
    cfgh = json.load(open(os.path.join(dh, "adapter_config.json")))
    th = load_file(os.path.join(dh, "adapter_model.safetensors"))
    ea = PRE + "spatial_embed_tokens.lora_embedding_A"
    with pytest.raises(ValueError, match="spatial_embed_tokens.lora_embedding_A"):
        fresh.load_lora(_write(tmp_path, "no_emb_a", {k: v for k, v in th.items() if k != ea}, cfgh))
    with pytest.raises(ValueError, match=r"lm_head\.lora_A\.weight"):
        fresh.load_lora(_write(tmp_path, "no_head_a", {k: v for k, v in th.items()
                                                       if k != PRE + "language_model.lm_head.lora_A.weight"}, cfgh))
    with pytest.raises(ValueError, match="both adapted"):
        fresh.load_lora(_write(tmp_path, "both", {**th, tk: tens[tk]}, cfgh))
    with pytest.raises(ValueError, match="spatial_embed_tokens"):
        fresh.load_lora(_write(tmp_path, "shape", {**th, ea: th[ea][:, :-1]}, cfgh))
    with pytest.raises(ValueError, match="ranks differ"):
        fresh.load_lora(_write(tmp_path, "rank", {**th, ea: torch.cat([th[ea], th[ea]], 0),
                                                  ea[:-1] + "B": torch.cat([th[ea[:-1] + "B"]] * 2, 1)}, cfgh))
    assert not fresh.has_lora and not hasattr(fresh.spatial_embed_tokens, "lora")
    _assert_unchanged(fresh, snap)


def test_merge_embeds_adds_the_embedding_term(cpu_model):
    """forward(inputs_embeds=...) goes through _merge_embeds (torch ops): the Embedding adapter's term is added there."""
    m = cpu_model
    cfg = m.config
    a0 = int(cfg.action_token_begin_idx)
    ids = torch.tensor([[5, a0 + 3, a0 + 3, 7, a0 + int(cfg.spatial_token_num) - 1]])
    emb_in = torch.zeros(1, 5, cfg.text_config.hidden_size, dtype=torch.bfloat16)
    base = m._merge_embeds(ids, emb_in, None)
    m.add_lora(R, ALPHA, target_modules="spatialvla-linear+emb", seed=2)
    with torch.no_grad():
        assert torch.equal(m._merge_embeds(ids, emb_in, None), base)  # A = 0: the base function
        m.spatial_embed_tokens.lora.A.normal_(0, 0.05)
    out = m._merge_embeds(ids, emb_in, None)
    ad = m.spatial_embed_tokens.lora
    W = m.spatial_embed_tokens.weight.detach().float()
    sid = ids[0] - a0
    norm = float(torch.tensor(cfg.text_config.hidden_size ** 0.5, dtype=torch.bfloat16))
    for t in (1, 2, 4):
        want = (W[sid[t]] + S * (ad.B.detach().float() @ ad.A.detach().float()[:, sid[t]])) * norm
        assert H.rel_l2(out[0, t].detach(), want) < 3 * 2.0 ** -8
    assert torch.equal(out[0, 0], base[0, 0]) and torch.equal(out[0, 3], base[0, 3])
    out.float().sum().backward()
    assert ad.A.grad is not None and float(ad.A.grad[:, sid[1]].abs().max()) > 0
    assert float(ad.A.grad[:, 0].abs().max()) == 0.0 and float(ad.B.grad.abs().max()) > 0
