"""Batched decode (enable_batched_decode) on the CPU: the switch's surface, the routing predicate's truth table, the
decode-state key, and the exported symbol."""
import ctypes
import os

import torch

import harness as H


def _model():
    return H.build_hip_model(H.cfg_dict("tiny"), "cpu")


def test_switch_exists_and_defaults_off():
    m = _model()
    lm = m.language_model
    assert m.batched_decode is False and lm.batched_decode is False and lm.model.batched_decode is False
    m._svla_decode_states = {"stale": object()}
    m.enable_batched_decode()
    assert m.batched_decode is True and lm.batched_decode is True and lm.model.batched_decode is True
    assert m._svla_decode_states == {}  # toggling drops the decode states
    m.enable_batched_decode(False)
    assert m.batched_decode is False and lm.model.batched_decode is False
    # the other switches are not involved
    assert m.fp8_decode is False and m.fp8_lora_decode is False and m.lora_decode is False


def test_predicate_truth_table():
    from spatialvla_amd import functional as Fn
    ok = Fn.batched_decode_ok
    # the window the measurement left (profiles/batched_decode_ab.txt)
    lo, hi = Fn.BATCHED_DECODE_MIN_ROWS, Fn.BATCHED_DECODE_MAX_ROWS
    assert (lo, hi) == (9, 64)
    step = dict(seen_tokens=40, grad_enabled=False)
    assert [ok(True, r, **step) for r in (8, 9, hi, hi + 1, 65)] == [False, True, True, False, False]
    assert not any(ok(False, r, **step) for r in (8, 9, hi, 64, 65))  # the switch is off
    assert not ok(True, 16, seen_tokens=0, grad_enabled=False)  # the prefill
    assert not ok(True, 16, seen_tokens=40, grad_enabled=True)
    assert not ok(True, 16, adapters=True, **step)
    assert not ok(True, 16, fp8_decode=True, **step)
    assert not ok(True, 16, fp8_projections=True, **step)
    assert not ok(True, 16, bf16=False, **step)
    assert ok(True, 16, widths=(2304, 2048, 9216), **step) and not ok(True, 16, widths=(2304, 40), **step)


def test_model_predicate_follows_the_configuration():
    from spatialvla_amd import functional as Fn
    m = _model()
    g = m.language_model.model
    with torch.no_grad():
        assert not g._batched_decode_ok(16, 40)  # off
        m.enable_batched_decode()
        assert g._batched_decode_ok(16, 40) and g._batched_decode_ok(9, 1) and g._batched_decode_ok(Fn.BATCHED_DECODE_MAX_ROWS, 1)
        assert not g._batched_decode_ok(8, 40) and not g._batched_decode_ok(65, 40) and not g._batched_decode_ok(16, 0)
        m.add_lora(8, 16.0, seed=0)
        assert not g._batched_decode_ok(16, 40)  # adapters attached
    m = _model()
    m.enable_batched_decode()
    assert not m.language_model.model._batched_decode_ok(16, 40)  # grad enabled
    with torch.no_grad():
        m.enable_fp8_decode()
        assert not m.language_model.model._batched_decode_ok(16, 40)
        m.enable_fp8_decode(False)
        assert m.language_model.model._batched_decode_ok(16, 40)


def test_decode_state_key_changes_with_the_switch():
    m = _model()
    dev = torch.device("cpu")
    st0 = m._decode_state(1, 16, dev)
    k0 = st0["wptr"]
    assert len(k0) == 5 and k0[1] == -1
    m.enable_batched_decode()
    st1 = m._decode_state(1, 16, dev)
    k1 = st1["wptr"]
    assert st1 is not st0 and k1 == k0 + ("batched",)
    m.enable_batched_decode(False)
    assert m._decode_state(1, 16, dev)["wptr"] == k0


def test_symbol_in_header_library_and_bindings():
    from spatialvla_amd import _lib, kernels as Kn
    hdr = open(os.path.join(H.REPO, "include", "svla.h")).read()
    assert "int svla_gemm_skinny(" in hdr and "svla_bf16_rows" in hdr
    assert "svla_gemm_skinny" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "svla_gemm_skinny")
    assert callable(Kn.gemm_skinny) and Kn.GEMM_SKINNY_MAX_M == 64
    assert Kn.gemm_skinny_ok(64, 9216) and not Kn.gemm_skinny_ok(65, 9216) and not Kn.gemm_skinny_ok(16, 40)
