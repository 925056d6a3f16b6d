"""The "spatialvla-linear+emb" / "+emb+h" recipes and modules_to_save on the CPU oracle, without editing oracle/.
lm_head goes through spatialvla_oracle._lin with the P tensor itself, so lora_ref.oracle_lora's id(w) patch covers it.
The Embedding adapter on spatial_embed_tokens replaces P["spatial_embed_tokens.weight"], for the duration of the
context, with the differentiable effective table W + ((A^T B^T) * s) in bf16 (peft's Embedding layer: the looked-up
row plus (after_A @ B^T) * scaling, after_A = A^T[id]); modules_to_save is requires_grad_(True) on the oracle's own
table.  Adapters are keyed by the model's module path.  Helper module, not a test."""
import contextlib

import torch

import lora_vision_ref as LV

EMB = "spatial_embed_tokens"
HEAD = "language_model.lm_head"
EMB_KEY = EMB + ".weight"


def make_adapters(P, cfgd, r, seed, emb=True, head=True, b_std=0.02, vision_b_std=None, emb_a_std=0.01):
    """lora_vision_ref.make_adapters (same values under the same seed) plus, from a third generator, the Embedding
    adapter (A [r, na] ~ N(0, emb_a_std^2), B [H, r] ~ N(0, 1): peft's B init, A moved off zero) and the lm_head adapter
    (A ~ N(0, 1/r^2), B ~ N(0, b_std^2)).  emb_a_std = 0 / b_std = 0 give the initial state."""
    out = LV.make_adapters(P, cfgd, r, seed, b_std=b_std, vision_b_std=vision_b_std)
    gen = torch.Generator().manual_seed(seed + 2000)
    if emb:
        w = P[EMB_KEY]
        A = (torch.randn(r, w.shape[0], generator=gen) * emb_a_std).to(torch.bfloat16).requires_grad_(True)
        B = torch.randn(w.shape[1], r, generator=gen).to(torch.bfloat16).requires_grad_(True)
        out[EMB] = (A, B)
    if head:
        w = P[HEAD + ".weight"]
        A = (torch.randn(r, w.shape[1], generator=gen) / r).to(torch.bfloat16).requires_grad_(True)
        B = (torch.randn(w.shape[0], r, generator=gen) * b_std).to(torch.bfloat16).requires_grad_(True)
        out[HEAD] = (A, B)
    return out


def effective_table(W, A, B, scaling):
    """W + ((A^T B^T) * s), every op on bf16 tensors; differentiable in A and B (and W when it requires grad)."""
    return W + (A.t() @ B.t()) * scaling


@contextlib.contextmanager
def oracle_lora(P, adapters, scaling, modules_to_save=False):
    """Patch the oracle for the duration of the context; P is restored on exit.  With modules_to_save the table is
    left a leaf that requires grad (its .grad is the table's gradient)."""
    table = P[EMB_KEY]
    lin = {p: ab for p, ab in adapters.items() if p != EMB}
    try:
        if EMB in adapters:
            assert not modules_to_save, "the table is adapted or trained in full, not both"
            P[EMB_KEY] = effective_table(table.detach(), *adapters[EMB], scaling)
        elif modules_to_save:
            table.requires_grad_(True)
        with LV.oracle_lora(P, lin, scaling):
            yield
    finally:
        P[EMB_KEY] = table


def merged_params(P, adapters, scaling):
    """lora_vision_ref.merged_params (one fp32 product, one rounding) with the table folded the same way."""
    Q = LV.merged_params(P, {p: ab for p, ab in adapters.items() if p != EMB}, scaling)
    if EMB in adapters:
        A, B = adapters[EMB]
        w = P[EMB_KEY]
        Q[EMB_KEY] = (w.detach().float() + scaling * (B.detach().float() @ A.detach().float()).t()).to(w.dtype)
    return Q


set_model_adapters = LV.set_model_adapters
