"""SpatialActionTokenizer.spatial_embedding_adaption against the reference's own run (tools/gen_adapt_emb_golden.py:
the real bin counts, gs_bridge -> gs_fractal, an E = 8 bf16 table).  CPU only.  The reference method is deterministic
on one machine (two runs give identical bits), so the table is compared bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

pytest.importorskip("scipy")

from spatialvla_amd import action_tokenizer as AT  # noqa: E402
from spatialvla_amd import functional as Fn  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "adapt_emb.npz")
BASE = 257153


class FakeTokenizer:
    def __init__(self, base=BASE):
        self.vocab, self.base = {}, base

    def add_tokens(self, toks, special_tokens=False):
        for t in toks:
            self.vocab.setdefault(t, self.base + len(self.vocab))

    def convert_tokens_to_ids(self, t):
        return self.vocab[t]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _bits(t):
    return t.detach().cpu().view(torch.int16).numpy().view(np.uint16)


def _setup(gold):
    nb = json.loads(str(gold["num_bins"]))
    sat = AT.SpatialActionTokenizer(FakeTokenizer(), nb, gs_params=json.loads(str(gold["gs0"])),
                                    use_spherical=bool(gold["use_spherical"]), min_sigma=0.0)
    emb = torch.nn.Embedding(sat.vocab_size, gold["before"].shape[1])
    emb.weight.data = torch.from_numpy(gold["before"].view(np.int16).copy()).view(torch.bfloat16)
    return sat, emb


def _check_policy(sat, gold):
    for kind, axes in AT.RANGE_BINS.items():
        for a in axes:
            np.testing.assert_array_equal(np.asarray(sat.bin_policy[kind][a]), gold[f"policy/{kind}/{a}"])
    for tok, kind in ((sat.translation_tokenizer, "translation"), (sat.rotation_tokenizer, "rotation")):
        for a, e in zip(tok.axes, tok.edges):
            np.testing.assert_array_equal(e, gold[f"policy/{kind}/{a}"])


def test_adapt_feature_matches_reference_bits(gold):
    sat, emb = _setup(gold)
    old_ids = sat.token_ids(gold["actions"])
    sat.spatial_embedding_adaption(json.loads(str(gold["gs1"])), emb, min_sigma=0.0, adpt_feature=True)
    _check_policy(sat, gold)
    assert emb.weight.dtype == torch.bfloat16
    after = _bits(emb.weight.data)
    np.testing.assert_array_equal(after, gold["after"])
    np.testing.assert_array_equal(after[8192:], gold["before"][8192:])  # the gripper rows
    assert (after[:8192] != gold["before"][:8192]).any(1).all()  # every grid row is resampled
    ids = sat.token_ids(gold["actions"])
    np.testing.assert_array_equal(ids, gold["ids"])  # tokenising uses the new bins
    assert (ids != old_ids).any()


def test_policy_only_leaves_table(gold):
    sat, emb = _setup(gold)
    sat.spatial_embedding_adaption(json.loads(str(gold["gs1"])), emb, min_sigma=0.0, adpt_feature=False)
    _check_policy(sat, gold)
    np.testing.assert_array_equal(_bits(emb.weight.data), gold["before"])
    np.testing.assert_array_equal(sat.token_ids(gold["actions"]), gold["ids"])


def test_norm_meshgrid_shape_and_order(gold):
    sat, _ = _setup(gold)
    tg, rg = sat.get_norm_meshgrid(sat.bin_policy)
    assert tg.shape == (18 * 34 * 10, 3) and rg.shape == (18 * 18 * 18, 3)
    assert tg.min() == 0.0 and tg.max() == 1.0
    # "xy" indexing: the list's slowest index walks axis 1 (phi), then axis 0 (theta), then axis 2 (r)
    g = tg.reshape(34, 18, 10, 3)
    assert (g[:, 0, 0, 1] == np.unique(tg[:, 1])).all() and (g[0, :, 0, 0] == np.unique(tg[:, 0])).all()


def test_flat_buffer_view_refused(gold):
    sat, emb = _setup(gold)
    Fn.register_flat_param(emb.weight)
    policy = sat.bin_policy
    with pytest.raises(RuntimeError, match="before building the engine"):
        sat.spatial_embedding_adaption(json.loads(str(gold["gs1"])), emb, adpt_feature=True)
    assert sat.bin_policy is policy
    np.testing.assert_array_equal(_bits(emb.weight.data), gold["before"])
