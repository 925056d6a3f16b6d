"""LoRA surface that needs no GPU: the patched-oracle facts the GPU parity tests rest on, the peft-format adapter
files, and the guards."""
import json
import os

import pytest
import torch

import harness as H
import lora_ref as LR

R, ALPHA, SEED = 8, 16.0, 7


@pytest.fixture(scope="module")
def oracle_runs():
    """The tiny oracle once without adapters, once with zero-B adapters, once with seeded adapters, once merged."""
    import spatialvla_oracle as O
    from spatialvla_amd import presets
    cfgd = H.cfg_dict("tiny")
    bc = H.batch_tensors(presets.synthetic_batch(cfgd, batch=2, seed=SEED), "cpu")
    P, zoe = H.build_oracle(cfgd)
    cap = {}
    with torch.no_grad():
        loss0, logits0 = O.forward(P, cfgd, bc, zoe, cap=cap)
        depth = cap["depth"]
        zero = LR.make_adapters(P, cfgd, R, SEED, b_std=0.0)
        with LR.oracle_lora(P, zero, ALPHA / R):
            loss_z, logits_z = O.forward(P, cfgd, bc, zoe, depth=depth)
        ads = LR.make_adapters(P, cfgd, R, SEED)
        with LR.oracle_lora(P, ads, ALPHA / R):
            loss_a, logits_a = O.forward(P, cfgd, bc, zoe, depth=depth)
        loss_m, logits_m = O.forward(LR.merged_params(P, ads, ALPHA / R), cfgd, bc, zoe, depth=depth)
        loss0d, logits0d = O.forward(P, cfgd, bc, zoe, depth=depth)
    return dict(base=(loss0d, logits0d), zero=(loss_z, logits_z), lora=(loss_a, logits_a), merged=(loss_m, logits_m),
                n_targets=len(ads))


def test_oracle_zero_B_is_bit_exact(oracle_runs):
    (l0, g0), (lz, gz) = oracle_runs["base"], oracle_runs["zero"]
    assert oracle_runs["n_targets"] == 14
    assert torch.equal(l0, lz) and torch.equal(g0, gz)


def test_oracle_adapters_move_logits_and_merge_is_close(oracle_runs, capsys):
    """The seeded adapters move the logits far from the base (an implementation that drops one cannot pass the parity
    tests), and the fp32-merged, bf16-rounded weights stay close to the adapter form: that distance is the yardstick of
    the GPU merge test."""
    moved = H.rel_l2(oracle_runs["lora"][1], oracle_runs["base"][1])
    merged = H.rel_l2(oracle_runs["merged"][1], oracle_runs["lora"][1])
    with capsys.disabled():
        print(f"\n[lora oracle] logits rel-L2: adapters vs base {moved:.3e}, merged vs adapters {merged:.3e}")
    assert moved > 0.1
    assert merged < 0.1 * moved  # merging is a re-rounding of the weights, far from dropping the adapters


@pytest.fixture()
def cpu_model():
    m = H.build_hip_model(H.cfg_dict("tiny", ), "cpu")
    return m


def test_add_lora_attaches_and_freezes(cpu_model):
    m = cpu_model
    keys0 = set(m.state_dict())
    m.add_lora(R, ALPHA, seed=3)
    assert m.has_lora
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    assert len(trainable) == 2 * 14 and all(n.endswith(("lora.A", "lora.B")) for n in trainable)
    assert keys0 <= set(m.state_dict())  # base keys unchanged
    lin = m.language_model.model.layers[0].self_attn.q_proj
    assert lin.lora.A.shape == (R, lin.in_features) and lin.lora.B.shape == (lin.out_features, R)
    assert lin.lora.A.dtype == torch.bfloat16 and float(lin.lora.B.detach().abs().max()) == 0.0
    assert abs(float(lin.lora.A.detach().float().std()) - 1.0 / R) < 0.2 / R
    # the engine's q|k|v grouping regex must not catch the adapter names
    from spatialvla_amd.engine import _group_params
    ps = _group_params(m.language_model.model.layers[0])
    assert sum(p.requires_grad for p in ps) == 14
    m2 = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    m2.add_lora(R, ALPHA, seed=3)
    assert torch.equal(m2.language_model.model.layers[1].mlp.down_proj.lora.A,
                       m.language_model.model.layers[1].mlp.down_proj.lora.A)


def test_add_lora_rejections(cpu_model):
    m = cpu_model
    for bad in (4, 12, 72, 0):
        with pytest.raises(ValueError):
            m.add_lora(bad, ALPHA)
    with pytest.raises(NotImplementedError, match="lm_head"):
        m.add_lora(R, ALPHA, target_modules=["q_proj", "lm_head"])
    with pytest.raises(NotImplementedError, match="fc1"):
        m.add_lora(R, ALPHA, target_modules=["fc1"])
    with pytest.raises(NotImplementedError):
        m.add_lora(R, ALPHA, target_modules="linear")
    with pytest.raises(NotImplementedError):
        m.add_lora(R, ALPHA, target_modules=["q_proj", "v_proj"])
    assert not m.has_lora
    m.enable_fp8_projections(True)
    with pytest.raises(NotImplementedError):
        m.add_lora(R, ALPHA)
    m.enable_fp8_projections(False)
    m.add_lora(R, ALPHA, target_modules=list(("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj",
                                              "down_proj")))
    with pytest.raises(NotImplementedError):
        m.enable_fp8_projections(True)
    with pytest.raises(RuntimeError):
        m.add_lora(R, ALPHA)


def test_unmerged_guards(cpu_model):
    m = cpu_model
    m.add_lora(R, ALPHA, seed=1)
    ids = torch.zeros(1, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match=r"call merge_lora\(\) first"):
        m.predict_action({"input_ids": ids})
    with pytest.raises(RuntimeError, match=r"call merge_lora\(\) first"):
        m.generate(input_ids=ids, max_new_tokens=1)
    with pytest.raises(RuntimeError, match=r"call merge_lora\(\) first"):
        m(input_ids=ids, past_key_values=m.new_cache(1, 8))


def test_save_load_round_trip(cpu_model, tmp_path):
    from safetensors.torch import load_file, save_file
    m = cpu_model
    m.add_lora(R, ALPHA, seed=5)
    with torch.no_grad():
        for _, lin in m._lora_linears():
            lin.lora.B.normal_(0, 0.02)
    d = str(tmp_path / "adapter")
    m.save_lora(d)
    cfg = json.load(open(os.path.join(d, "adapter_config.json")))
    assert cfg["peft_type"] == "LORA" and cfg["r"] == R and cfg["lora_alpha"] == ALPHA
    assert cfg["init_lora_weights"] == "gaussian"
    assert sorted(cfg["target_modules"]) == sorted(["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj",
                                                    "down_proj"])
    tens = load_file(os.path.join(d, "adapter_model.safetensors"))
    assert len(tens) == 28
    k = "base_model.model.language_model.model.layers.1.mlp.down_proj.lora_B.weight"
    assert k in tens and tens[k].shape == (256, R)
    assert tens["base_model.model.language_model.model.layers.0.self_attn.k_proj.lora_A.weight"].shape == (R, 256)
    m2 = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    m2.load_lora(d)
    assert m2.has_lora
    for (p, a), (_, b) in zip(m._lora_linears(), m2._lora_linears()):
        assert torch.equal(a.lora.A, b.lora.A) and torch.equal(a.lora.B, b.lora.B), p
        assert b.lora.scaling == ALPHA / R
    assert not any(p.requires_grad for n, p in m2.named_parameters() if ".lora." not in n)
    # foreign keys and unequal ranks are rejected, listing the keys
    foreign = dict(tens)
    fk = "base_model.model.language_model.lm_head.lora_A.weight"
    foreign[fk] = torch.zeros(R, 256, dtype=torch.bfloat16)
    d2 = str(tmp_path / "foreign")
    os.makedirs(d2)
    save_file(foreign, os.path.join(d2, "adapter_model.safetensors"))
    json.dump(cfg, open(os.path.join(d2, "adapter_config.json"), "w"))
    m3 = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    with pytest.raises(ValueError, match="lm_head"):
        m3.load_lora(d2)
    assert not m3.has_lora
    ragged = dict(tens)
    ka = "base_model.model.language_model.model.layers.0.self_attn.q_proj.lora_A.weight"
    ragged[ka] = torch.zeros(2 * R, 256, dtype=torch.bfloat16)
    ragged[ka.replace("lora_A", "lora_B")] = torch.zeros(512, 2 * R, dtype=torch.bfloat16)
    d3 = str(tmp_path / "ragged")
    os.makedirs(d3)
    save_file(ragged, os.path.join(d3, "adapter_model.safetensors"))
    json.dump(cfg, open(os.path.join(d3, "adapter_config.json"), "w"))
    with pytest.raises(ValueError, match="q_proj.lora_A.weight"):
        m3.load_lora(d3)
    assert not m3.has_lora
