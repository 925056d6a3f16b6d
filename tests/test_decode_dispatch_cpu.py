"""Which kernel wrappers a KV-cached step issues, in which order and in which form, for every decode mode -- on the CPU.

Every public function of spatialvla_amd.kernels except the pure helpers is replaced by a recorder, so the tiny model
(H 256, I 512, 2 layers) runs Gemma2Model.forward(cache=...) and Gemma2ForCausalLM.head without a device and leaves the
exact launch sequence.  An entry is the wrapper's name and, in brackets, what selects its form: the number of weight
segments, `norm` (a norm-pair prologue), `geglu`, `k_back`, `rope` (the RoPE epilogue), `o` (the o projection inside
svla_decode_mlp) and `site=` (the name handed to FP8DecodeWeights.get for the weights it streams).

EXPECTED is the behaviour of commit 898e381, the parent of the change that folded the projection choice into
Fn.decode_proj: the table was printed by this test's _run on that commit and pasted here before the refactor."""
import inspect

import pytest
import torch

import harness as H

R, ALPHA = 8, 16.0
PURE = ("lora_R", "round_up", "ceil_div", "attn_args")
SEG_ARGS = ("weights", "wq", "mats", "ws")  # the first of these that is a list: the projection's row segments
FLAGS = ("DECODE_FUSED", "DECODE_NORM_FUSED", "LORA_DECODE_KERNELS", "LORA_DECODE_EMB_HEAD_KERNELS",
         "DECODE_MLP_PERSIST", "DECODE_O_FUSED", "PREFILL_ROPE_FILL")
DEFAULTS = {f: f != "DECODE_O_FUSED" for f in FLAGS}  # the values without any SVLA_* variable set


class _OnDevice(torch.Tensor):
    """Hidden rows that claim a device: the decode heads are gated on h.is_cuda."""
    is_cuda = True


def _recorders(monkeypatch, grid=0):
    """Replace the kernel wrappers; returns the log the recorders append to."""
    from spatialvla_amd import functional as Fn
    from spatialvla_amd import kernels as Kn
    log, sites = [], []

    def recorder(name, fn):
        sig = inspect.signature(fn)

        def rec(*args, **kw):
            a = sig.bind(*args, **kw).arguments
            tags = [str(len(a[s])) for s in SEG_ARGS if isinstance(a.get(s), (list, tuple))][:1]
            tags += [t for t, key in (("norm", "norm"), ("geglu", "geglu_out"), ("k_back", "k_back"), ("rope", "rope"),
                                      ("o", "o")) if a.get(key) not in (None, False)]
            tags += ["site=" + s for s in sites]
            del sites[:]
            log.append(name + ("[" + ",".join(tags) + "]" if tags else ""))
        return rec

    for name, fn in list(vars(Kn).items()):
        if (name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != Kn.__name__
                or name.endswith("_ok") or name in PURE):
            continue
        monkeypatch.setattr(Kn, name, recorder(name, fn))
    # shape-only fakes: the grid of svla_decode_mlp (0: it can not run) and the quantiser behind FP8DecodeWeights
    monkeypatch.setattr(Kn, "decode_mlp_grid", lambda M, Hd, I: grid)
    monkeypatch.setattr(Kn, "quant_mx_rows", lambda x: (torch.empty(x.shape, dtype=torch.uint8), tuple(x.shape)))
    monkeypatch.setattr(Kn, "mx_scales_rowmajor", lambda sc: torch.empty(sc[0], sc[1] // 32, dtype=torch.uint8))
    get = Fn.FP8DecodeWeights.get

    def get_logged(self, name, mats):
        sites.append(name)
        return get(self, name, mats)
    monkeypatch.setattr(Fn.FP8DecodeWeights, "get", get_logged)
    return log


def _model(lora=None):
    """lora: None, "layers" (the seven Gemma2 projections) or "emb_head" (also spatial_embed_tokens and lm_head)."""
    m = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    if lora is not None:
        kw = {"target_modules": "spatialvla-linear+emb+h"} if lora == "emb_head" else {}
        m.add_lora(R, ALPHA, seed=0, **kw)
    return m


def _step(m, rows, seen):
    """One KV-cached forward of the decoder: the prefill of one `rows`-token prompt, or a decode step of `rows`
    sequences with `seen` tokens in the cache."""
    from spatialvla_amd.modeling_gemma2 import Gemma2KVCache, KVMask
    g = m.language_model.model
    B, Lq = (1, rows) if seen == 0 else (rows, 1)
    cache = Gemma2KVCache(g.config, B, 32, "cpu")
    cache.seen_tokens = seen
    hidden = torch.zeros(B, Lq, g.config.hidden_size, dtype=torch.bfloat16)
    pos = torch.arange(seen, seen + Lq)[None].expand(B, -1)
    with torch.no_grad():
        g(hidden, KVMask(torch.zeros(B, Lq, dtype=torch.uint8)), pos, cache=cache)
    assert cache.seen_tokens == seen + Lq


def _head(m):
    lm = m.language_model
    h = torch.zeros(1, 1, lm.config.hidden_size, dtype=torch.bfloat16).as_subclass(_OnDevice)
    with torch.no_grad():
        lm.head(h, torch.zeros(1, dtype=torch.int64), {}, decode=True)


def _lora_decode(m, fp8=False, emb_head=False):
    m.enable_lora_decode(True, emb_head=emb_head)
    if fp8:
        m.enable_fp8_lora_decode()
    return m


# case -> (model's adapters, switches to turn on, flags off / on, svla_decode_mlp's grid, what runs)
CASES = {
    "prefill": (None, None, {}, 0, lambda m: _step(m, 5, 0)),
    "decode": (None, None, {}, 0, lambda m: _step(m, 1, 5)),
    "decode_norm_unfused": (None, None, {"DECODE_NORM_FUSED": False}, 0, lambda m: _step(m, 1, 5)),
    "decode_attn_unfused": (None, None, {"DECODE_FUSED": False}, 0, lambda m: _step(m, 1, 5)),
    "decode_persist": (None, None, {}, 64, lambda m: _step(m, 1, 5)),
    "decode_persist_o_fused": (None, None, {"DECODE_O_FUSED": True}, 64, lambda m: _step(m, 1, 5)),
    "prefill_rope_epilogue": (None, None, {"PREFILL_ROPE_FILL": False}, 0, lambda m: _step(m, 5, 0)),
    "batched_16": (None, lambda m: m.enable_batched_decode(), {}, 0, lambda m: _step(m, 16, 5)),
    "batched_8_not_routed": (None, lambda m: m.enable_batched_decode(), {}, 0, lambda m: _step(m, 8, 5)),
    "fp8_decode": (None, lambda m: m.enable_fp8_decode(), {}, 0, lambda m: _step(m, 1, 5)),
    "lora_decode": ("layers", _lora_decode, {}, 0, lambda m: _step(m, 1, 5)),
    "lora_decode_composed": ("layers", _lora_decode, {"LORA_DECODE_KERNELS": False}, 0, lambda m: _step(m, 1, 5)),
    "lora_fp8_decode": ("layers", lambda m: _lora_decode(m, fp8=True), {}, 0, lambda m: _step(m, 1, 5)),
    "lora_prefill": ("layers", _lora_decode, {}, 0, lambda m: _step(m, 5, 0)),
    "lora_decode_9_rows": ("layers", _lora_decode, {}, 0, lambda m: _step(m, 9, 5)),
    "head": (None, None, {}, 0, _head),
    "head_fp8": (None, lambda m: m.enable_fp8_decode(), {}, 0, _head),
    "head_lora": ("emb_head", lambda m: _lora_decode(m, emb_head=True), {}, 0, _head),
    "head_lora_fp8": ("emb_head", lambda m: _lora_decode(m, fp8=True, emb_head=True), {}, 0, _head),
}


def _run(case, monkeypatch):
    from spatialvla_amd import functional as Fn
    lora, switches, flags, grid, run = CASES[case]
    for f in FLAGS:
        monkeypatch.setattr(Fn, f, [flags.get(f, DEFAULTS[f])])
    m = _model(lora)
    if switches is not None:
        switches(m)
    log = _recorders(monkeypatch, grid)
    run(m)
    return log


EXPECTED = {
    "prefill": [
        "rmsnorm_fwd", "linear_fwd[3]", "qkv_rope_append[k_back]", "attn_fwd", "linear_fwd[1]", "add_rmsnorm2_fwd",
        "linear_geglu_fwd", "linear_fwd[1]", "add_rmsnorm2_fwd", "linear_fwd[3]", "qkv_rope_append[k_back]",
        "attn_fwd", "linear_fwd[1]", "add_rmsnorm2_fwd", "linear_geglu_fwd", "linear_fwd[1]", "add_rmsnorm2_fwd"
    ],
    "decode": [
        "rmsnorm_fwd", "linear_fwd[3]", "attn_decode_rope", "linear_fwd[1]", "gemv_rmsnorm2[2,geglu]",
        "linear_fwd[1]", "gemv_rmsnorm2[3]", "attn_decode_rope", "linear_fwd[1]", "gemv_rmsnorm2[2,geglu]",
        "linear_fwd[1]", "add_rmsnorm2_fwd"
    ],
    "decode_norm_unfused": [
        "rmsnorm_fwd", "linear_fwd[3]", "attn_decode_rope", "linear_fwd[1]", "add_rmsnorm2_fwd", "linear_geglu_fwd",
        "linear_fwd[1]", "add_rmsnorm2_fwd", "linear_fwd[3]", "attn_decode_rope", "linear_fwd[1]", "add_rmsnorm2_fwd",
        "linear_geglu_fwd", "linear_fwd[1]", "add_rmsnorm2_fwd"
    ],
    "decode_attn_unfused": [
        "rmsnorm_fwd", "linear_fwd[3]", "qkv_rope_append", "attn_decode", "linear_fwd[1]", "gemv_rmsnorm2[2,geglu]",
        "linear_fwd[1]", "gemv_rmsnorm2[3]", "qkv_rope_append", "attn_decode", "linear_fwd[1]",
        "gemv_rmsnorm2[2,geglu]", "linear_fwd[1]", "add_rmsnorm2_fwd"
    ],
    "decode_persist": [
        "rmsnorm_fwd", "linear_fwd[3]", "attn_decode_rope", "linear_fwd[1]", "decode_mlp", "gemv_rmsnorm2[3]",
        "attn_decode_rope", "linear_fwd[1]", "decode_mlp", "add_rmsnorm2_fwd"
    ],
    "decode_persist_o_fused": [
        "rmsnorm_fwd", "linear_fwd[3]", "attn_decode_rope", "decode_mlp[o]", "gemv_rmsnorm2[3]", "attn_decode_rope",
        "decode_mlp[o]", "add_rmsnorm2_fwd"
    ],
    "prefill_rope_epilogue": [
        "rmsnorm_fwd", "linear_fwd[3,rope]", "attn_fwd", "linear_fwd[1]", "add_rmsnorm2_fwd", "linear_geglu_fwd",
        "linear_fwd[1]", "add_rmsnorm2_fwd", "linear_fwd[3,rope]", "attn_fwd", "linear_fwd[1]", "add_rmsnorm2_fwd",
        "linear_geglu_fwd", "linear_fwd[1]", "add_rmsnorm2_fwd"
    ],
    "batched_16": [
        "rmsnorm_fwd", "gemm_skinny[3]", "attn_decode_rope", "gemm_skinny[1]", "add_rmsnorm2_fwd", "linear_geglu_fwd",
        "linear_fwd[1]", "add_rmsnorm2_fwd", "gemm_skinny[3]", "attn_decode_rope", "gemm_skinny[1]",
        "add_rmsnorm2_fwd", "linear_geglu_fwd", "linear_fwd[1]", "add_rmsnorm2_fwd"
    ],
    "batched_8_not_routed": [
        "rmsnorm_fwd", "linear_fwd[3]", "attn_decode_rope", "linear_fwd[1]", "gemv_rmsnorm2[2,geglu]",
        "linear_fwd[1]", "gemv_rmsnorm2[3]", "attn_decode_rope", "linear_fwd[1]", "gemv_rmsnorm2[2,geglu]",
        "linear_fwd[1]", "add_rmsnorm2_fwd"
    ],
    "fp8_decode": [
        "rmsnorm_fwd", "gemv_mxfp8[1,site=qkv]", "attn_decode_rope", "gemv_mxfp8[1,site=o]",
        "gemv_mxfp8[2,norm,geglu,site=gate_up]", "gemv_mxfp8[1,site=down]", "gemv_mxfp8[1,norm,site=qkv]",
        "attn_decode_rope", "gemv_mxfp8[1,site=o]", "gemv_mxfp8[2,norm,geglu,site=gate_up]",
        "gemv_mxfp8[1,site=down]", "add_rmsnorm2_fwd"
    ],
    "lora_decode": [
        "rmsnorm_fwd", "lora_gemv_down[3]", "lora_gemv[3]", "attn_decode_rope", "lora_gemv_down[1]", "lora_gemv[1]",
        "lora_gemv_down[2,norm]", "lora_gemv[2,geglu]", "lora_gemv_down[1]", "lora_gemv[1]", "lora_gemv_down[3,norm]",
        "lora_gemv[3]", "attn_decode_rope", "lora_gemv_down[1]", "lora_gemv[1]", "lora_gemv_down[2,norm]",
        "lora_gemv[2,geglu]", "lora_gemv_down[1]", "lora_gemv[1]", "add_rmsnorm2_fwd"
    ],
    "lora_decode_composed": [
        "rmsnorm_fwd", "lora_down[3]", "linear_fwd[3]", "lora_up[3]", "attn_decode_rope", "linear_fwd[1]",
        "linear_fwd[1]", "lora_up[1]", "add_rmsnorm2_fwd", "lora_down[2]", "linear_fwd[2]", "lora_up[2]",
        "linear_fwd[1]", "linear_fwd[1]", "lora_up[1]", "add_rmsnorm2_fwd", "lora_down[3]", "linear_fwd[3]",
        "lora_up[3]", "attn_decode_rope", "linear_fwd[1]", "linear_fwd[1]", "lora_up[1]", "add_rmsnorm2_fwd",
        "lora_down[2]", "linear_fwd[2]", "lora_up[2]", "linear_fwd[1]", "linear_fwd[1]", "lora_up[1]",
        "add_rmsnorm2_fwd"
    ],
    "lora_fp8_decode": [
        "rmsnorm_fwd", "lora_gemv_down[3]", "lora_gemv_mxfp8[1,site=qkv]", "attn_decode_rope", "lora_gemv_down[1]",
        "lora_gemv_mxfp8[1,site=o]", "lora_gemv_down[2,norm]", "lora_gemv_mxfp8[2,geglu,site=gate_up]",
        "lora_gemv_down[1]", "lora_gemv_mxfp8[1,site=down]", "lora_gemv_down[3,norm]", "lora_gemv_mxfp8[1,site=qkv]",
        "attn_decode_rope", "lora_gemv_down[1]", "lora_gemv_mxfp8[1,site=o]", "lora_gemv_down[2,norm]",
        "lora_gemv_mxfp8[2,geglu,site=gate_up]", "lora_gemv_down[1]", "lora_gemv_mxfp8[1,site=down]",
        "add_rmsnorm2_fwd"
    ],
    "lora_prefill": [
        "rmsnorm_fwd", "lora_down[3]", "linear_fwd[3]", "lora_up[3]", "qkv_rope_append[k_back]", "attn_fwd",
        "linear_fwd[1]", "linear_fwd[1]", "lora_up[1]", "add_rmsnorm2_fwd", "lora_down[2]", "linear_fwd[2]",
        "lora_up[2]", "linear_fwd[1]", "linear_fwd[1]", "lora_up[1]", "add_rmsnorm2_fwd", "lora_down[3]",
        "linear_fwd[3]", "lora_up[3]", "qkv_rope_append[k_back]", "attn_fwd", "linear_fwd[1]", "linear_fwd[1]",
        "lora_up[1]", "add_rmsnorm2_fwd", "lora_down[2]", "linear_fwd[2]", "lora_up[2]", "linear_fwd[1]",
        "linear_fwd[1]", "lora_up[1]", "add_rmsnorm2_fwd"
    ],
    "lora_decode_9_rows": [
        "rmsnorm_fwd", "lora_down[3]", "linear_fwd[3]", "lora_up[3]", "attn_decode_rope", "linear_fwd[1]",
        "linear_fwd[1]", "lora_up[1]", "add_rmsnorm2_fwd", "lora_down[2]", "linear_fwd[2]", "lora_up[2]",
        "linear_fwd[1]", "linear_fwd[1]", "lora_up[1]", "add_rmsnorm2_fwd", "lora_down[3]", "linear_fwd[3]",
        "lora_up[3]", "attn_decode_rope", "linear_fwd[1]", "linear_fwd[1]", "lora_up[1]", "add_rmsnorm2_fwd",
        "lora_down[2]", "linear_fwd[2]", "lora_up[2]", "linear_fwd[1]", "linear_fwd[1]", "lora_up[1]",
        "add_rmsnorm2_fwd"
    ],
    "head": [
        "linear_fwd[1]", "softcap_ce_rows", "ce_finalize"
    ],
    "head_fp8": [
        "head_gemv_mxfp8[site=lm_head]", "ce_finalize"
    ],
    "head_lora": [
        "lora_gemv_down[1]", "lora_head_gemv", "ce_finalize"
    ],
    "head_lora_fp8": [
        "lora_gemv_down[1]", "lora_head_gemv_mxfp8[site=lm_head]", "ce_finalize"
    ],
}


@pytest.mark.parametrize("case", list(CASES))
def test_launch_sequence(case, monkeypatch):
    got = _run(case, monkeypatch)
    print(case, got)
    assert got == EXPECTED[case]


def test_adapters_refused_with_lora_decode_off(monkeypatch):
    from spatialvla_amd.modeling_gemma2 import LORA_MERGE_MSG
    m = _model("layers")
    log = _recorders(monkeypatch)
    for rows, seen in ((5, 0), (1, 5), (9, 5)):
        with pytest.raises(RuntimeError) as e:
            _step(m, rows, seen)
        assert str(e.value) == LORA_MERGE_MSG
    assert log == []


@pytest.mark.parametrize("what", ["pre", "lora", "f8d", "prefill"])
def test_batched_takes_a_plain_decode_step_only(what, monkeypatch):
    from spatialvla_amd import functional as Fn
    log = _recorders(monkeypatch)
    m = _model()
    at = m.language_model.model.layers[0].self_attn
    x = torch.zeros(16, 256, dtype=torch.bfloat16)
    kc = torch.zeros(16, 32, 256, dtype=torch.bfloat16)
    tab = torch.zeros(16, 128, dtype=torch.bfloat16)
    w = torch.zeros(256)
    kw = {"pre": {"pre": (x, x, w, w, 1e-6, 1e-6, x)}, "lora": {"lora": (R, 2.0) + 4 * ((None, None),)},
          "f8d": {"f8d": Fn.FP8DecodeWeights()}, "prefill": {}}[what]
    with pytest.raises(ValueError, match="batched is a plain bf16 decode step"):
        Fn.gemma_attention_cached(x, at.q_proj.weight, at.k_proj.weight, at.v_proj.weight, at.o_proj.weight, tab, tab,
                                  kc, kc.clone(), torch.zeros(16, 32, dtype=torch.uint8), 0 if what == "prefill" else 5,
                                  at.attn_cfg(16, 1), batched=True, **kw)
    assert log == []
