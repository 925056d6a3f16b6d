"""The opt-in switch for KV-cached decode with unmerged LoRA adapters, as far as it needs no GPU: it exists and is off
by default, the refusals keep their text while it is off, the new entry points are in header, library and bindings, and
the decode-state key follows the switch and the adapters' storage."""
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


def test_switch_exists_and_defaults_off(cpu_model):
    from spatialvla_amd import functional as Fn
    m = cpu_model
    assert m.lora_decode is False and m.language_model.model.lora_decode is False
    m.enable_lora_decode()
    assert m.lora_decode is True and m.language_model.model.lora_decode is True
    assert all(l.self_attn._svla_lora_decode for l in m.language_model.model.layers)
    m.enable_lora_decode(False)
    assert m.lora_decode is False
    assert not any(l.self_attn._svla_lora_decode for l in m.language_model.model.layers)
    # the language model on its own carries the same switch
    m.language_model.enable_lora_decode(True)
    assert m.lora_decode is True
    assert isinstance(Fn.LORA_DECODE_KERNELS, list) and Fn.LORA_DECODE_KERNELS[0] is True


def test_refusals_unchanged_while_off(cpu_model):
    from spatialvla_amd.modeling_gemma2 import LORA_MERGE_MSG, KVMask
    m = cpu_model
    m.add_lora(R, ALPHA, seed=1)
    ids = torch.zeros(1, 4, dtype=torch.int64)
    tail = (": call merge_lora() first (unmerged LoRA adapters; the KV-cached decode kernels read the base weights "
            "only)")
    with pytest.raises(RuntimeError) as e:
        m.predict_action({"input_ids": ids})
    assert str(e.value) == "predict_action" + tail
    with pytest.raises(RuntimeError) as e:
        m.generate(input_ids=ids, max_new_tokens=1)
    assert str(e.value) == "generate" + tail
    with pytest.raises(RuntimeError) as e:
        m(input_ids=ids, past_key_values=m.new_cache(1, 8))
    assert str(e.value) == "forward(past_key_values=...)" + tail
    with pytest.raises(RuntimeError) as e:
        with torch.no_grad():
            m(input_ids=ids, use_cache=True)
    assert str(e.value) == "forward(use_cache=True) (it creates a KV cache)" + tail
    # the language model used on its own refuses in its cached layer loop, with its own message
    assert LORA_MERGE_MSG == ("unmerged LoRA adapters: call merge_lora() first (the KV-cached kernels read the base "
                              "weights only)")
    lm = m.language_model.model
    hidden = torch.zeros(1, 4, lm.config.hidden_size, dtype=torch.bfloat16)
    mask = KVMask(torch.zeros(1, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError) as e:
        with torch.no_grad():
            lm(hidden, mask, torch.arange(4)[None] + 1, cache=m.new_cache(1, 8))
    assert str(e.value) == LORA_MERGE_MSG


def test_new_symbols_in_header_library_and_bindings():
    from spatialvla_amd import _lib, kernels as Kn
    hdr = open(os.path.join(H.REPO, "include", "svla.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("svla_lora_gemv_down", "svla_lora_gemv"):
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, re.M), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is _lib.c_i32
    assert "svla_lora_norm2" in hdr and ctypes.sizeof(_lib.LoraNorm2) == 5 * 8 + 8 + 2 * 4
    assert "train/spatialvla_finetune.py:262-300" in hdr.split("svla_lora_gemv_down")[0].rsplit("/*", 1)[1]
    assert callable(Kn.lora_gemv_down) and callable(Kn.lora_gemv)
    assert Kn.lora_gemv_ok(1, 2304, [2048, 1024, 1024], norm=True)
    assert Kn.lora_gemv_ok(8, 9216, [2304]) and not Kn.lora_gemv_ok(8, 9216, [2304], norm=True)
    assert not Kn.lora_gemv_ok(9, 2304, [2304]) and not Kn.lora_gemv_ok(1, 2304, [24, 40])


def test_decode_state_key_follows_switch_and_adapters(cpu_model):
    m = cpu_model
    dev = torch.device("cpu")
    k0 = m._decode_state(1, 16, dev)["wptr"]
    assert k0[2] is None
    m.add_lora(R, ALPHA, seed=1)
    assert m.__dict__["_svla_decode_states"] == {}          # add_lora dropped the states
    k1 = m._decode_state(1, 16, dev)["wptr"]
    ad = m.language_model.model.layers[0].self_attn.q_proj.lora
    assert k1[:2] == k0[:2] and k1[2] == (False, ad.A.data_ptr(), R, ALPHA / R)
    st = m._decode_state(1, 16, dev)
    assert m._decode_state(1, 16, dev) is st                # unchanged key: the state is reused
    m.enable_lora_decode(True)
    assert m.__dict__["_svla_decode_states"] == {}          # the switch itself dropped the states
    k2 = m._decode_state(1, 16, dev)["wptr"]
    assert k2 != k1 and k2[2][0] is True
    # the adapters rebound to other storage (what TrainEngine's flat buffers do): a stale state is replaced
    st2 = m._decode_state(1, 16, dev)
    with torch.no_grad():
        ad.A.data = ad.A.data.clone()
    st3 = m._decode_state(1, 16, dev)
    assert st3 is not st2 and st3["wptr"] != k2 and st3["wptr"][2][1] == ad.A.data_ptr()
    # values changed in place: same key, same state (the graphs read the current values)
    with torch.no_grad():
        ad.B.add_(1.0)
    assert m._decode_state(1, 16, dev) is st3
