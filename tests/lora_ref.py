"""LoRA on the CPU oracle, without editing oracle/: a context manager that replaces spatialvla_oracle._lin with
y = _lin(x, w, b) + linear(linear(x, A), B) * s (peft's Linear.forward: base(x) + lora_B(lora_A(x)) * scaling) for the
weights that carry an adapter, keyed by id(w) of the oracle's parameter tensors.  A and B carry requires_grad, so the
oracle's backward yields the adapter gradients.  Helper module, not a test."""
import contextlib

import torch
import torch.nn.functional as F

LORA_TARGETS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
                "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def target_names(cfgd):
    """Module paths (= oracle weight names without '.weight') of the adapted projections, in layer order."""
    n = cfgd["text_config"]["num_hidden_layers"]
    return [f"language_model.model.layers.{i}.{t}" for i in range(n) for t in LORA_TARGETS]


def make_adapters(P, cfgd, r, seed, b_std=0.02):
    """{module path: (A [r, in], B [out, r])} bf16 leaves with requires_grad: A ~ N(0, 1/r^2) (peft "gaussian"),
    B ~ N(0, b_std^2) (0 gives peft's initial state)."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for name in target_names(cfgd):
        w = P[name + ".weight"]
        A = (torch.randn(r, w.shape[1], generator=gen) / r).to(torch.bfloat16).requires_grad_(True)
        B = (torch.randn(w.shape[0], r, generator=gen) * b_std).to(torch.bfloat16).requires_grad_(True)
        out[name] = (A, B)
    return out


@contextlib.contextmanager
def oracle_lora(P, adapters, scaling):
    import spatialvla_oracle as O
    by_id = {id(P[name + ".weight"]): ab for name, ab in adapters.items()}
    base = O._lin

    def lin(x, w, b=None):
        y = base(x, w, b)
        ab = by_id.get(id(w))
        if ab is not None:
            y = y + F.linear(F.linear(x, ab[0]), ab[1]) * scaling
        return y

    O._lin = lin
    try:
        yield
    finally:
        O._lin = base


def merged_params(P, adapters, scaling):
    """A copy of P with W <- bf16(W + s B A) (fp32 product, one rounding) on the adapted projections."""
    Q = dict(P)
    for name, (A, B) in adapters.items():
        w = P[name + ".weight"]
        Q[name + ".weight"] = (w.detach().float() + scaling * (B.detach().float() @ A.detach().float())).to(w.dtype)
    return Q


def set_model_adapters(model, adapters):
    """Copy the oracle's adapter values (bf16, shared bit for bit) into a model that has add_lora() applied."""
    mods = dict(model.named_modules())
    with torch.no_grad():
        for name, (A, B) in adapters.items():
            ad = mods[name].lora
            ad.A.copy_(A.detach().to(ad.A.device))
            ad.B.copy_(B.detach().to(ad.B.device))
