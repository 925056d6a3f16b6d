"""Weight-only fp8 decode under unmerged adapters (enable_fp8_lora_decode) on the CPU: the switch's surface, its
refusals with the message that names the way out, what turns it off, that the existing fp8-decode switch and state keys
are what they were, the exported symbols, and the seed choice of the adapter decode-head kernel test."""
import ctypes
import os
import re

import pytest
import torch

import harness as H

R, ALPHA = 8, 16.0


@pytest.fixture()
def cpu_model():
    return H.build_hip_model(H.cfg_dict("tiny"), "cpu")


def _on(m, **kw):
    m.add_lora(R, ALPHA, seed=0, **kw)
    m.enable_lora_decode(True, emb_head="target_modules" in kw)
    m.enable_fp8_lora_decode()
    return m


def test_switch_surface(cpu_model):
    from spatialvla_amd import functional as Fn
    m = cpu_model
    lm = m.language_model
    assert m.fp8_lora_decode is False and lm.model.fp8_lora_decode is False
    assert lm.fp8_lora_decode_holders() == [] and m._fp8_lora_decode_key() is None
    m.add_lora(R, ALPHA, seed=0)
    m.enable_lora_decode()
    m._svla_decode_states = {"stale": object()}
    m.enable_fp8_lora_decode()
    assert m.fp8_lora_decode is True and m._svla_decode_states == {}  # toggling drops the decode states
    holders = lm.fp8_lora_decode_holders()
    assert len(holders) == len(lm.model.layers) + 1 and all(isinstance(h, Fn.FP8DecodeWeights) for h in holders)
    assert len({id(h) for h in holders}) == len(holders)
    assert all(h.mats == {} and h.frozen for h in holders)  # built lazily; the base weights are frozen
    # the existing switch and its holders are not involved: load_lora / add_lora's refusal does not fire
    assert m.fp8_decode is False and lm.fp8_decode_holders() == [] and m._fp8_decode_key() is None
    m._refuse_lora_under_fp8_decode("load_lora")
    # independent of the training step's fp8 base projections
    m.enable_fp8_lora()
    assert m.fp8_lora_decode and m.fp8_lora
    m.enable_fp8_lora(False)
    assert m.fp8_lora_decode and not m.fp8_lora
    m.enable_fp8_lora_decode(False)
    assert not m.fp8_lora_decode and lm.fp8_lora_decode_holders() == [] and m.lora_decode


def test_refused_without_adapters_or_lora_decode(cpu_model):
    m = cpu_model
    with pytest.raises(RuntimeError) as e:
        m.enable_fp8_lora_decode()
    assert str(e.value) == ("enable_fp8_lora_decode: no adapters attached (add_lora() / load_lora() first); a merged "
                            "model streams its e4m3 weights through enable_fp8_decode()")
    assert not m.fp8_lora_decode
    m.add_lora(R, ALPHA, seed=0)
    m._svla_decode_states = {"kept": 1}
    with pytest.raises(RuntimeError) as e:
        m.enable_fp8_lora_decode()
    assert str(e.value) == ("enable_fp8_lora_decode: the unmerged decode is off: call enable_lora_decode() first "
                            "(the e4m3 copies replace the base weights of its adapter GEMVs)")
    assert not m.fp8_lora_decode and m._svla_decode_states == {"kept": 1}  # before any state change
    m.enable_fp8_lora_decode(False)  # turning it off is always allowed
    m.enable_lora_decode()
    m.enable_fp8_lora_decode()
    assert m.fp8_lora_decode


def test_emb_head_permit_stays_with_enable_lora_decode(cpu_model):
    m = cpu_model
    m.add_lora(R, ALPHA, target_modules="spatialvla-linear+emb+h", seed=0)
    with pytest.raises(NotImplementedError, match="enable_lora_decode"):
        m.enable_lora_decode()
    with pytest.raises(RuntimeError, match=r"call enable_lora_decode\(\) first"):
        m.enable_fp8_lora_decode()
    m.enable_lora_decode(True, emb_head=True)
    m.enable_fp8_lora_decode()
    assert m.fp8_lora_decode and m.lora_decode_emb_head


def test_fp8_decode_still_refused_with_adapters(cpu_model):
    m = _on(cpu_model)
    with pytest.raises(RuntimeError) as e:
        m.enable_fp8_decode()
    assert str(e.value) == ("enable_fp8_decode: LoRA adapters are attached: call merge_lora() first (the e4m3 decode "
                            "copies are made from the merged weights)")
    assert m.fp8_decode is False and m.fp8_lora_decode is True


def test_load_lora_keeps_the_switch_and_the_holders(cpu_model, tmp_path):
    other = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    other.add_lora(R, ALPHA, seed=3)
    with torch.no_grad():
        other.language_model.model.layers[0].mlp.down_proj.lora.B.fill_(0.25)
    other.save_lora(str(tmp_path))
    m = _on(cpu_model)
    holders = m.language_model.fp8_lora_decode_holders()
    m.load_lora(str(tmp_path))  # the same set and rank: A / B copied in place
    assert m.fp8_lora_decode and m.lora_decode
    now = m.language_model.fp8_lora_decode_holders()
    assert len(now) == len(holders) and all(a is b for a, b in zip(now, holders))
    assert float(m.language_model.model.layers[0].mlp.down_proj.lora.B.float().mean()) == 0.25


@pytest.mark.parametrize("how", ["off", "lora_decode_off"])
def test_turned_off(cpu_model, how):
    m = _on(cpu_model)
    m._svla_decode_states = {"stale": object()}
    if how == "off":
        m.enable_fp8_lora_decode(False)
        assert m.lora_decode
    else:
        m.enable_lora_decode(False)
        assert not m.lora_decode
    assert not m.fp8_lora_decode and m.language_model.fp8_lora_decode_holders() == []
    assert m._svla_decode_states == {} and m._fp8_lora_decode_key() is None
    assert not hasattr(m.language_model, "_svla_fp8_lora_decode_head") or m.language_model._svla_fp8_lora_decode_head is None


def test_state_keys_unchanged_with_the_switch_off(cpu_model):
    m = cpu_model
    dev = torch.device("cpu")
    k0 = m._decode_state(1, 16, dev)["wptr"]
    assert len(k0) == 5 and k0[2] is None and k0[3] is None and k0[4] is None
    assert k0[:2] == (m.language_model.lm_head.weight.data_ptr(), -1)
    assert m._adapter_key() is None and m._fp8_decode_key() is None and m.fp8_decode is False
    m.add_lora(R, ALPHA, seed=1)
    m.enable_lora_decode()
    ad = m.language_model.model.layers[0].self_attn.q_proj.lora
    assert m._adapter_key() == (True, ad.A.data_ptr(), R, ALPHA / R)
    k1 = m._decode_state(1, 16, dev)["wptr"]
    assert k1[:2] == k0[:2] and k1[2] == m._adapter_key() and k1[3] is None and k1[4] is None
    # on and off again: the keys of the other switches are what they were
    m.enable_fp8_lora_decode()
    assert m._adapter_key() == k1[2] and m._fp8_decode_key() is None and m.fp8_decode is False
    m.enable_fp8_lora_decode(False)
    assert m._decode_state(1, 16, dev)["wptr"] == k1


def test_new_symbols_in_header_library_and_bindings():
    from spatialvla_amd import _lib, kernels as Kn
    hdr = open(os.path.join(H.REPO, "include", "svla.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("svla_lora_gemv_mxfp8", "svla_lora_head_gemv_mxfp8"):
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, re.M), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is _lib.c_i32
    assert len(_lib.SIGNATURES["svla_lora_gemv_mxfp8"][1]) == 14
    assert len(_lib.SIGNATURES["svla_lora_head_gemv_mxfp8"][1]) == 20
    doc = hdr.split("int svla_lora_gemv_mxfp8")[0].rsplit("/*", 1)[1]
    for word in ("K % 128 == 0", "ldq % 16 == 0", "svla_mx_scales_rowmajor", "SLICED"):
        assert word in doc, word
    assert callable(Kn.lora_gemv_mxfp8) and callable(Kn.lora_head_gemv_mxfp8)
    # the union of the parents' shape gates
    assert Kn.lora_gemv_mxfp8_ok(1, 2304, [2048, 1024, 1024]) and Kn.lora_gemv_mxfp8_ok(8, 9216, [2304])
    assert not Kn.lora_gemv_mxfp8_ok(9, 2304, [2304])       # M > 8
    assert not Kn.lora_gemv_mxfp8_ok(1, 264, [48])          # K % 128 (svla_lora_gemv alone takes it)
    assert Kn.lora_gemv_ok(1, 264, [48])
    assert not Kn.lora_gemv_mxfp8_ok(1, 2304, [24, 40])     # slice starts off the multiples of 16
    assert Kn.lora_head_gemv_mxfp8_ok(8, 2304, 32) and not Kn.lora_head_gemv_mxfp8_ok(8, 9216, 32)
    assert not Kn.lora_head_gemv_mxfp8_ok(1, 264, 32) and not Kn.lora_head_gemv_mxfp8_ok(1, 2304, 12)


def test_frozen_holder_ignores_the_weight_epoch():
    """A frozen holder's key does not carry WEIGHT_EPOCH (an optimizer step on A and B rebuilds nothing); the holder of
    enable_fp8_decode still does."""
    from spatialvla_amd import functional as Fn
    w = torch.zeros(4, 4)
    assert Fn.FP8DecodeWeights(frozen=True)._epoch([w]) == -1
    assert Fn.FP8DecodeWeights()._epoch([w]) == Fn.WEIGHT_EPOCH[0]


def test_head_seed_is_confident():
    """The seeds of test_fp8_lora_decode_kernels_gpu.HEAD_CASES: with the quantiser emulated on the CPU (X =
    ceil(log2(amax / 448)), e4m3 round to nearest even) and T = bf16(x A^T) at least 3/4 of the rows of the float64
    reference have a top-2 margin above H.MARGIN, and no row sits within a few bf16 ulps of it, where the roundings of
    the logit chain could decide."""
    import test_fp8_lora_decode_kernels_gpu as T
    for M, n, k, r, seed in T.HEAD_CASES:
        w, x, A, B, s = T._head_case(M, n, k, r, seed)
        b = w.float().view(n, k // 32, 32)
        amax = b.abs().amax(-1)
        X = torch.where(amax > 0, torch.ceil(torch.log2(amax.double() / 448)).float(), torch.full_like(amax, -127.0))
        q = (b * torch.exp2(-X)[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn).float()
        wd = (q * torch.exp2(X)[..., None]).view(n, k)
        t = (x.double() @ A.double().T).to(torch.bfloat16)
        ref = T.head_reference(x, wd, t, B, s)
        moved = ref - T.CAP * torch.tanh(x.double() @ wd.double().T / T.CAP)
        assert float(moved.std()) > 0.25, (M, n, k, seed)  # the adapter term is a visible part of the logits
        top2 = ref.topk(2, -1).values
        mg = top2[:, 0] - top2[:, 1]
        assert int((mg > H.MARGIN).sum()) * 4 >= 3 * M, (M, n, k, seed, mg.tolist())
        assert not bool(((mg > 0.6 * H.MARGIN) & (mg < 3 * H.MARGIN)).any()), (M, n, k, seed, mg.tolist())
