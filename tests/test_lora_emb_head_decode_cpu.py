"""enable_lora_decode(emb_head=True), as far as it needs no GPU: the default refusals of the "spatialvla-linear+emb" /
"+emb+h" sets are intact, the second opt-in is accepted and cleared by switching off, the decode-state key keeps its
tuple for the sets without those adapters and gains the Embedding / lm_head adapters' storage with them, and the two
new entry points are in header, library and bindings."""
import ctypes
import os
import re

import pytest
import torch

import harness as H

R, ALPHA = 8, 16.0
SETS = ("gemma2-linear", "spatialvla-linear", "spatialvla-linear+emb", "spatialvla-linear+emb+h")


def _model(targets=None):
    m = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    if targets is not None:
        m.add_lora(R, ALPHA, target_modules=targets, seed=1)
    return m


@pytest.mark.parametrize("targets", SETS[2:])
def test_default_refusals_intact(targets):
    m = _model(targets)
    m.clear_decode_cache()
    assert m.lora_decode_emb_head is False
    ids = torch.zeros(1, 4, dtype=torch.int64)
    for call in (lambda: m.enable_lora_decode(), lambda: m.enable_lora_decode(True),
                 lambda: m.enable_lora_decode(True, emb_head=False)):
        with pytest.raises(NotImplementedError, match=r"merge_lora\(\)"):
            call()
        assert not m.lora_decode and not m.lora_decode_emb_head
    for call in (lambda: m.predict_action({"input_ids": ids}), lambda: m.generate(input_ids=ids, max_new_tokens=1),
                 lambda: m(input_ids=ids, past_key_values=m.new_cache(1, 8)),
                 lambda: m(input_ids=ids, use_cache=True)):
        with pytest.raises(NotImplementedError, match=r"merge_lora\(\)"):
            with torch.no_grad():
                call()
    assert m.__dict__["_svla_decode_states"] == {}


@pytest.mark.parametrize("targets", SETS)
def test_emb_head_opt_in_and_off(targets):
    m = _model(targets)
    m._decode_state(1, 16, torch.device("cpu"))
    m.enable_lora_decode(True, emb_head=True)
    assert m.lora_decode is True and m.lora_decode_emb_head is True
    assert m.__dict__["_svla_decode_states"] == {}  # toggling drops the decode states
    m._require_merged("predict_action")             # the entry points' gate passes
    m._decode_state(1, 16, torch.device("cpu"))
    m.enable_lora_decode(False)
    assert m.lora_decode is False and m.lora_decode_emb_head is False
    assert m.__dict__["_svla_decode_states"] == {}
    if "+emb" in targets:  # off again: the refusal is back, and the plain switch does not grant the permission
        with pytest.raises(NotImplementedError, match=r"merge_lora\(\)"):
            m._require_merged("predict_action")
        with pytest.raises(NotImplementedError, match=r"merge_lora\(\)"):
            m.enable_lora_decode(True)
        assert not m.lora_decode and not m.lora_decode_emb_head
    else:
        m.enable_lora_decode(True)
        assert m.lora_decode and not m.lora_decode_emb_head


def test_property_is_read_only():
    m = _model()
    with pytest.raises(AttributeError):
        m.lora_decode_emb_head = True


def test_adapter_key_per_set():
    assert _model()._adapter_key() is None
    m = _model("gemma2-linear")
    q = m.language_model.model.layers[0].self_attn.q_proj.lora
    assert m._adapter_key() == (False, q.A.data_ptr(), R, ALPHA / R)
    m = _model("spatialvla-linear")
    q = m.language_model.model.layers[0].self_attn.q_proj.lora
    vis = m.multi_modal_projector.linear.lora
    assert m._adapter_key() == (False, q.A.data_ptr(), R, ALPHA / R, vis.A.data_ptr())
    m = _model("spatialvla-linear+emb")
    q = m.language_model.model.layers[0].self_attn.q_proj.lora
    vis = m.multi_modal_projector.linear.lora
    emb = m.spatial_embed_tokens.lora
    assert m._adapter_key() == (False, q.A.data_ptr(), R, ALPHA / R, vis.A.data_ptr(), emb.A.data_ptr())
    m = _model("spatialvla-linear+emb+h")
    q = m.language_model.model.layers[0].self_attn.q_proj.lora
    vis = m.multi_modal_projector.linear.lora
    emb, head = m.spatial_embed_tokens.lora, m.language_model.lm_head.lora
    key = (False, q.A.data_ptr(), R, ALPHA / R, vis.A.data_ptr(), emb.A.data_ptr(), head.A.data_ptr())
    assert m._adapter_key() == key
    m.enable_lora_decode(True, emb_head=True)
    assert m._adapter_key() == (True,) + key[1:]


@pytest.mark.parametrize("which", ("emb", "head"))
def test_rebinding_either_adapter_changes_the_key(which):
    """What TrainEngine's flat buffers do to the storage; a change in place (an optimizer step) keeps key and state."""
    m = _model("spatialvla-linear+emb+h")
    m.enable_lora_decode(True, emb_head=True)
    dev = torch.device("cpu")
    ad = m.spatial_embed_tokens.lora if which == "emb" else m.language_model.lm_head.lora
    st = m._decode_state(1, 16, dev)
    with torch.no_grad():
        ad.B.add_(1.0)
        ad.A.add_(1.0)
    assert m._decode_state(1, 16, dev) is st
    k = m._adapter_key()
    with torch.no_grad():
        ad.A.data = ad.A.data.clone()
    assert m._adapter_key() != k and ad.A.data_ptr() in m._adapter_key()
    assert m._decode_state(1, 16, dev) is not st


@pytest.mark.parametrize("targets", SETS[2:])
def test_load_lora_rebinds_and_changes_the_key(targets, tmp_path):
    src = _model(targets)
    src.save_lora(str(tmp_path))
    m = _model()
    m.enable_lora_decode(True, emb_head=True)
    st = m._decode_state(1, 16, torch.device("cpu"))
    assert m._adapter_key() is None
    m.load_lora(str(tmp_path))  # attaches the set: new adapter storage
    assert m.lora_targets == targets and m.lora_decode and m.lora_decode_emb_head
    key = m._adapter_key()
    assert key is not None and len(key) == len(src._adapter_key()) == (7 if targets.endswith("+h") else 6)
    assert not set(key[4:]) & set(src._adapter_key()[4:])  # both models alive: the storage is distinct
    assert m.__dict__["_svla_decode_states"] == {}          # load_lora dropped the states
    assert m._decode_state(1, 16, torch.device("cpu")) is not st


def test_new_symbols_in_header_library_and_bindings():
    from spatialvla_amd import _lib, kernels as Kn
    hdr = open(os.path.join(H.REPO, "include", "svla.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("svla_lora_head_gemv", "svla_lora_embed_decode"):
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, re.M), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is _lib.c_i32
    doc = hdr.split("int svla_lora_head_gemv")[0].rsplit("/*", 1)[1]
    assert "modeling_gemma2.py:993-997" in doc and "train/spatialvla_finetune.py:279-286" in doc
    assert callable(Kn.lora_head_gemv) and callable(Kn.lora_embed_decode)
    assert Kn.lora_head_gemv_ok(1, 2304, 32) and Kn.lora_head_gemv_ok(8, 256, 64)
    assert not Kn.lora_head_gemv_ok(9, 2304, 32) and not Kn.lora_head_gemv_ok(1, 2300, 32)
    assert not Kn.lora_head_gemv_ok(1, 2304, 12) and not Kn.lora_head_gemv_ok(1, 8192, 32)
