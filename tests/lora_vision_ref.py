"""The full "spatialvla-linear" adapter set on the CPU oracle: what tests/lora_ref.py does for the seven Gemma2
projections, extended to the SigLIP q/k/v/out_proj/fc1/fc2, the projector and both Ego3D linears.  The oracle already
routes every one of them through spatialvla_oracle._lin with the P tensors themselves, so lora_ref.oracle_lora's id(w)
patch covers them; only the names differ (the oracle's vision keys have no `vision_model.` infix).  Adapters are keyed
by the model's module path, as the adapter files are.  Helper module, not a test."""
import torch

import lora_ref as LR

VISION_PER_LAYER = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2")


def vision_names(cfgd):
    """Module paths of the vision-side targets, in add_lora's order."""
    n = cfgd["vision_config"]["num_hidden_layers"]
    out = [f"vision_tower.vision_model.encoder.layers.{i}.{t}" for i in range(n) for t in VISION_PER_LAYER]
    out.append("multi_modal_projector.linear")
    if cfgd.get("use_vision_zoe", True):
        out += ["position_embedding_3d.position_embedding_head.0", "position_embedding_3d.position_embedding_head.3"]
    return out


def target_names(cfgd):
    return LR.target_names(cfgd) + vision_names(cfgd)


def oracle_key(path):
    """Oracle parameter name of a module path's weight."""
    return path.replace("vision_tower.vision_model.", "vision_tower.") + ".weight"


def make_adapters(P, cfgd, r, seed, b_std=0.02, vision_b_std=None):
    """{module path: (A, B)} for all targets: the Gemma2 adapters of lora_ref.make_adapters (same seed, same values),
    then the vision-side ones from a second generator; vision_b_std (default b_std) is the std of the vision B."""
    out = LR.make_adapters(P, cfgd, r, seed, b_std=b_std)
    vb = b_std if vision_b_std is None else vision_b_std
    gen = torch.Generator().manual_seed(seed + 1000)
    for name in vision_names(cfgd):
        w = P[oracle_key(name)]
        A = (torch.randn(r, w.shape[1], generator=gen) / r).to(torch.bfloat16).requires_grad_(True)
        B = (torch.randn(w.shape[0], r, generator=gen) * vb).to(torch.bfloat16).requires_grad_(True)
        out[name] = (A, B)
    return out


def _oracle_named(adapters):
    """The adapters under names lora_ref's helpers can look up in P (name + '.weight')."""
    return {oracle_key(p)[:-len(".weight")]: ab for p, ab in adapters.items()}


def oracle_lora(P, adapters, scaling):
    return LR.oracle_lora(P, _oracle_named(adapters), scaling)


def merged_params(P, adapters, scaling):
    return LR.merged_params(P, _oracle_named(adapters), scaling)


set_model_adapters = LR.set_model_adapters
