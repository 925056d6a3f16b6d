"""Sampled decode, the part that needs no GPU: the Philox4x32-10 known answer and the chi-square of the numpy
restatement (tests/sample_ref.py) that the kernel is compared with, the parameter block's layout, the refusals while
enable_sampled_decode is off, and SpatialVLAProcessor.action_token_ranges()."""
import json
import os

import numpy as np
import pytest
import torch

import harness as H
import sample_ref as R


def test_philox_known_answer():
    """Random123's known-answer vector of philox4x32-10 for the zero counter and key."""
    assert [int(x) for x in R.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = [int(x) for x in R.philox4x32_10(*[0xffffffff] * 6)]
    assert ones == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]  # Random123 kat_vectors, all-ones line


def test_restatement_chi_square():
    """20 000 Gumbel-max draws of one row (N = 577, distinct (row id, position) pairs) follow softmax(v): Pearson's
    statistic over the 31 most probable columns + rest stays below the 1 - 1e-6 quantile of chi-square(31)."""
    v = R.make_logits(np.random.default_rng(5), 1, 577, 2.0)[0].astype(np.float64)
    cols = np.arange(577)
    toks = []
    for r0 in range(0, 80, 8):  # 80 row ids x 250 positions, 8 row ids at a time
        rows = np.arange(r0, r0 + 8)[:, None, None]
        pos = np.arange(250)[None, :, None]
        toks.append(np.argmax(v + R.gumbel(cols[None, None, :], pos, rows, 99), -1).ravel())
    toks = np.concatenate(toks)
    assert toks.shape == (20000,)
    chi = R.chi_square_top31(v, toks)
    print(f"chi-square(31) of the restatement: {chi:.1f}")
    assert chi < R.CHI2_31_Q
    # the same draws through sample_row: the vectorised noise above is the function's
    for rid, pos in ((0, 0), (3, 17), (79, 249)):
        assert R.sample_row(v, 1.0, seed=99, position=pos, row_id=rid)["token"] == toks[rid * 250 + pos]


def test_restatement_filters():
    v = np.array([1.0, 3.0, 2.0, 3.0, 0.5, -1.0, 2.5], dtype=np.float64)
    r = R.sample_row(v, 1.0, top_k=2)
    assert r["kept"] == 2 and r["thr"] == 3.0 and r["token"] in (1, 3)
    assert abs(R.logprobs(r, v, 1)[0] - np.log(0.5)) < 1e-12
    r = R.sample_row(v, 1.0, top_k=3)  # ties at the threshold are all kept; 2.5 is the third largest
    assert r["kept"] == 3 and r["thr"] == 2.5
    w = np.exp(v - 3.0)
    p_two = 2.0 / w.sum()  # the mass of the two 3.0 columns
    assert R.sample_row(v, 1.0, top_p=p_two - 1e-3)["kept"] == 2
    assert R.sample_row(v, 1.0, top_p=p_two + 1e-3)["kept"] == 3
    r = R.sample_row(v, 0.0, lo=4, hi=7)  # greedy inside a range
    assert r["token"] == 6 and r["kept"] == 3
    lp, lpr = R.logprobs(r, v, 6)
    assert abs(lp - (2.5 - np.log(np.exp(v[4:7]).sum()))) < 1e-12 and abs(lpr - (2.5 - np.log(np.exp(v).sum()))) < 1e-12
    vn = v.copy()
    vn[5] = np.nan
    assert R.sample_row(vn, 1.0, lo=4, hi=7)["token"] == 5 and not R.sample_row(vn, 1.0, lo=0, hi=5)["nan"]


def test_param_block_layout():
    import struct
    from spatialvla_amd import _lib as L
    from spatialvla_amd import kernels as K
    assert L.ctypes.sizeof(L.SampleParams) == 32
    blk = K.pack_sample_params(0.7, 0.95, 50, seed=0x0123456789ABCDEF, draw=3, nranges=2)
    assert blk.dtype == torch.uint8 and blk.numel() == 32
    t, p, k, n, seed, draw = struct.unpack("<ffiiQQ", bytes(blk.tolist()))
    assert (np.float32(t), np.float32(p), k, n, seed, draw) == (np.float32(0.7), np.float32(0.95), 50, 2,
                                                                0x0123456789ABCDEF, 3)


@pytest.fixture(scope="module")
def tiny_model():
    from spatialvla_amd import SpatialVLAConfig
    from spatialvla_amd.modeling_spatialvla import SpatialVLAForConditionalGeneration
    return SpatialVLAForConditionalGeneration(SpatialVLAConfig(**H.cfg_dict("tiny"))).to(torch.bfloat16)


def test_switch_and_refusals(tiny_model):
    m = tiny_model
    assert m.sampled_decode is False
    inputs = {"input_ids": torch.ones(1, 3, dtype=torch.int64)}
    for kw in (dict(do_sample=True), dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9), dict(seed=1),
               dict(allowed_ranges=[(513, 577)]), dict(return_logprobs=True)):
        with pytest.raises(RuntimeError, match="enable_sampled_decode"):
            m.predict_action(inputs, max_new_tokens=2, **kw)
    with pytest.raises(NotImplementedError, match="enable_sampled_decode"):
        m.generate(torch.ones(1, 3, dtype=torch.int64), do_sample=True)
    m.enable_sampled_decode()
    try:
        assert m.sampled_decode is True
        with pytest.raises(ValueError, match="temperature"):
            m.predict_action(inputs, max_new_tokens=2, do_sample=True, temperature=0.0)
        with pytest.raises(ValueError, match="allowed_ranges"):
            m.predict_action(inputs, max_new_tokens=2, allowed_ranges=[(5, 5)])
        with pytest.raises(ValueError, match="allowed_ranges"):
            m.predict_action(inputs, max_new_tokens=2, allowed_ranges=[(0, 578)])
        with pytest.raises(NotImplementedError, match="beam"):
            m.generate(torch.ones(1, 3, dtype=torch.int64), do_sample=True, num_beams=2)
        # an explicit seed determines the call; without one every call takes a fresh seed from torch's generator
        a = m._sample_args("t", True, 1.0, 0, 1.0, 5, None)
        assert (a["seed"], a["draw"]) == (5, 0)
        torch.manual_seed(3)
        b, c = m._sample_args("t", True, 1.0, 0, 1.0, None, None), m._sample_args("t", True, 1.0, 0, 1.0, None, None)
        torch.manual_seed(3)
        d = m._sample_args("t", True, 1.0, 0, 1.0, None, None)
        assert b["seed"] == d["seed"] != c["seed"]
        g = m._sample_args("t", False, 1.0, 0, 1.0, None, [(513, 545), (545, 577)], True)
        assert g["temperature"] == 0.0 and g["ranges"] == [(513, 545), (545, 577)]
    finally:
        m.enable_sampled_decode(False)
    assert m.sampled_decode is False


def test_processor_action_token_ranges():
    import processor_fixtures as PF
    from spatialvla_amd import SpatialVLAProcessor
    gold = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "processor.npz")))
    proc = SpatialVLAProcessor(PF.build_image_processor(), PF.build_tokenizer(),
                               statistics=json.loads(str(gold["statistics"])),
                               intrinsic_config=json.loads(str(gold["intrinsic_config"])),
                               action_config=json.loads(str(gold["action_config"])), action_chunk_size=4)
    at = proc.action_tokenizer
    rg = proc.action_token_ranges()
    want = [(t.token_start_idx, t.token_end_idx + 1)
            for t in (at.translation_tokenizer, at.rotation_tokenizer, at.gripper_tokenizer)]
    assert rg == want and len(rg) == 3
    assert rg[0][0] == at.action_token_begin_idx and rg[0][1] == rg[1][0] and rg[1][1] == rg[2][0]
    assert all(isinstance(v, int) for r in rg for v in r) and all(lo < hi for lo, hi in rg)
