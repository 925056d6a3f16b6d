"""Weight-only fp8 decode (enable_fp8_decode) on the CPU: the switch's surface and its refusals, each with the message
that names the way out -- no kernel is reached -- and the seed choice of the decode-head kernel test."""
import pytest
import torch

import harness as H

R, ALPHA = 8, 16.0


@pytest.fixture()
def cpu_model():
    return H.build_hip_model(H.cfg_dict("tiny"), "cpu")


def test_switch_surface(cpu_model):
    from spatialvla_amd import functional as Fn
    m = cpu_model
    lm = m.language_model
    assert not m.fp8_decode and lm.fp8_decode_holders() == [] and m._fp8_decode_key() is None
    m._svla_decode_states = {"stale": object()}
    m.enable_fp8_decode()
    assert m.fp8_decode and m._svla_decode_states == {}  # toggling drops the decode states
    holders = lm.fp8_decode_holders()
    assert len(holders) == len(lm.model.layers) + 1 and all(isinstance(h, Fn.FP8DecodeWeights) for h in holders)
    assert len({id(h) for h in holders}) == len(holders)
    assert all(h.mats == {} for h in holders)  # built lazily: nothing is quantised when the switch is turned
    # independent of the training step's fp8 projections
    m.enable_fp8_projections()
    assert m.fp8_decode
    m.enable_fp8_projections(False)
    assert m.fp8_decode
    m.enable_fp8_decode(False)
    assert not m.fp8_decode and lm.fp8_decode_holders() == []


def test_enable_refused_with_adapters(cpu_model):
    m = cpu_model
    m.add_lora(R, ALPHA, seed=0)
    with pytest.raises(RuntimeError) as e:
        m.enable_fp8_decode()
    assert str(e.value) == ("enable_fp8_decode: LoRA adapters are attached: call merge_lora() first (the e4m3 decode "
                            "copies are made from the merged weights)")
    assert not m.fp8_decode and m.has_lora
    m.enable_fp8_decode(False)  # turning it off is always allowed
    assert m.has_lora


def test_add_and_load_lora_refused_while_on(cpu_model, tmp_path):
    m = cpu_model
    other = H.build_hip_model(H.cfg_dict("tiny"), "cpu")
    other.add_lora(R, ALPHA, seed=0)
    other.save_lora(str(tmp_path))
    m.enable_fp8_decode()
    snap = {n: p.detach().clone() for n, p in m.named_parameters()}
    for what, call in (("add_lora", lambda: m.add_lora(R, ALPHA, seed=0)),
                       ("load_lora", lambda: m.load_lora(str(tmp_path)))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == (f"{what}: weight-only fp8 decode is on (enable_fp8_decode): call "
                                "enable_fp8_decode(False) first -- the e4m3 decode copies hold the base weights only")
        assert not m.has_lora and m.fp8_decode
    now = dict(m.named_parameters())
    assert now.keys() == snap.keys() and all(torch.equal(now[n].detach(), v) for n, v in snap.items())
    m.enable_fp8_decode(False)
    m.load_lora(str(tmp_path))
    assert m.has_lora


def test_head_seed_is_confident():
    """The seeds of test_fp8_decode_kernels_gpu.HEAD_CASES: with the quantiser emulated on the CPU (X = ceil(log2(amax /
    448)), e4m3 round to nearest even) at least 3/4 of the rows of the float64 reference have a top-2 margin above
    H.MARGIN, and no row sits within a few bf16 ulps of it, where the roundings of the logit chain could decide."""
    import test_fp8_decode_kernels_gpu as T
    for M, n, k, seed in T.HEAD_CASES:
        w, x = T._head_data(M, n, k, seed)
        b = w.float().view(n, k // 32, 32)
        amax = b.abs().amax(-1)
        X = torch.where(amax > 0, torch.ceil(torch.log2(amax.double() / 448)).float(), torch.full_like(amax, -127.0))
        q = (b * torch.exp2(-X)[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn).float()
        wd = (q * torch.exp2(X)[..., None]).view(n, k)
        ref = T.CAP * torch.tanh(x.double() @ wd.double().T / T.CAP)
        top2 = ref.topk(2, -1).values
        mg = top2[:, 0] - top2[:, 1]
        assert int((mg > H.MARGIN).sum()) * 4 >= 3 * M, (M, n, k, seed, mg.tolist())
        assert not bool(((mg > 0.6 * H.MARGIN) & (mg < 3 * H.MARGIN)).any()), (M, n, k, seed, mg.tolist())
