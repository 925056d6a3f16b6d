"""enable_fp8_lora()'s surface that needs no GPU: the switch, what turns it off, and the C-ABI struct layout."""
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


def _layer_state(m):
    return [(getattr(l.self_attn, "_svla_fp8_lora", None), getattr(l.mlp, "_svla_fp8_lora", None))
            for l in m.language_model.model.layers]


def test_enable_fp8_lora_needs_adapters(cpu_model):
    m = cpu_model
    assert m.fp8_lora is False
    with pytest.raises(RuntimeError, match=r"enable_fp8_projections\(\)"):
        m.enable_fp8_lora()
    assert m.fp8_lora is False
    m.enable_fp8_lora(False)  # turning it off is always allowed


def test_switch_and_what_clears_it(cpu_model, tmp_path):
    from spatialvla_amd import functional as Fn
    m = cpu_model
    m.add_lora(R, ALPHA, seed=1)
    m.save_lora(str(tmp_path))
    with pytest.raises(AttributeError):
        m.fp8_lora = True  # read-only
    m.__dict__["_svla_decode_states"] = {"stale": 1}
    m.enable_fp8_lora()
    assert m.fp8_lora is True and not m.__dict__["_svla_decode_states"]
    for a, b in _layer_state(m):
        assert isinstance(a, Fn.FP8Weights) and a is b and a.frozen
    m.load_lora(str(tmp_path))  # new adapter values under the same frozen base: the switch stays on
    assert m.fp8_lora is True
    # the plain switch stays refused with adapters, and leaves this one alone
    with pytest.raises(NotImplementedError):
        m.enable_fp8_projections(True)
    assert m.fp8_lora is True
    assert all(getattr(l.mlp, "_svla_fp8", None) is None for l in m.language_model.model.layers)
    m.enable_fp8_lora(False)
    assert m.fp8_lora is False and all(a is None and b is None for a, b in _layer_state(m))
    m.enable_fp8_lora(True)
    m.enable_fp8_projections(False)
    assert m.fp8_lora is False and all(a is None and b is None for a, b in _layer_state(m))
    m.enable_fp8_lora(True)
    with pytest.raises(RuntimeError, match="GPU"):  # merge_lora's guard path: the kernels need the GPU ...
        m.merge_lora()
    assert m.fp8_lora is False  # ... and the copies of the unmerged weights are dropped before anything is merged


def test_frozen_copies_ignore_the_optimizer_epoch_unless_flat():
    """FP8Weights(frozen): the cache key does not follow WEIGHT_EPOCH (TrainEngine steps rewrite the adapters only),
    except for a weight that sits in an engine's flat buffers; the plain object follows it as before."""
    from spatialvla_amd import functional as Fn
    w = torch.zeros(4, 4)
    e0 = Fn.WEIGHT_EPOCH[0]
    try:
        frozen, plain = Fn.FP8Weights(frozen=True), Fn.FP8Weights()
        k_f, k_p = frozen._epoch((w,)), plain._epoch((w,))
        Fn.WEIGHT_EPOCH[0] += 1
        assert frozen._epoch((w,)) == k_f and plain._epoch((w,)) != k_p
        Fn.register_flat_param(w)
        k_f = frozen._epoch((w,))
        Fn.WEIGHT_EPOCH[0] += 1
        assert frozen._epoch((w,)) != k_f
    finally:
        Fn.WEIGHT_EPOCH[0] = e0


def test_lora_epilogue_struct_matches_header():
    from spatialvla_amd import _lib
    names = [f[0] for f in _lib.LoraEpilogue._fields_]
    assert names[-4:] == ["mx_q", "mx_ldq", "mx_scales", "mx_sld"]
    types = dict((f[0], f[1]) for f in _lib.LoraEpilogue._fields_)
    assert types["mx_q"] is ctypes.c_void_p and types["mx_scales"] is ctypes.c_void_p
    assert types["mx_ldq"] is ctypes.c_int64 and types["mx_sld"] is ctypes.c_int64
    hdr = open(os.path.join(H.REPO, "include", "svla.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} svla_lora_epilogue;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.split(r"[\s*]+", d.strip())[-1] for d in body.split(";") if d.strip()]
    assert fields == names
    assert ctypes.sizeof(_lib.LoraEpilogue) == 16 + 8 * (len(names) - 4)
