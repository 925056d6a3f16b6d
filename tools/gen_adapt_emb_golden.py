"""Golden vectors for SpatialActionTokenizer.spatial_embedding_adaption, produced by the REFERENCE itself.

TEST INFRASTRUCTURE ONLY (needs the reference tree and scipy).  Imports the reference's model/action_tokenizer.py the
way oracle/gen_action_golden.py does (and reuses its FakeTokenizer), builds the tokenizer with the real bin counts
(scripts/action_config.json) on the gs_bridge statistics, and adapts an E = 8 bf16 spatial table to gs_fractal with
adpt_feature=True.  Writes tests/golden/adapt_emb.npz: both Gaussian parameter sets and the bin counts as JSON
strings, the table before and after as bf16 bit patterns (uint16), the new bin edges, and the token ids of a few
actions under the new bins.  The reference module is imported, never copied.

    python tools/gen_adapt_emb_golden.py
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
OUT = os.path.join(REPO, "tests", "golden", "adapt_emb.npz")
E = 8


def main():
    import torch
    import gen_action_golden as G
    at, _ = G._import_reference()
    cfg = json.load(open(os.path.join(G.REF, "scripts", "action_config.json")))
    gs0 = json.load(open(os.path.join(G.REF, "scripts", "gs_bridge.json")))
    gs1 = json.load(open(os.path.join(G.REF, "scripts", "gs_fractal.json")))
    tok = G.FakeTokenizer()
    with contextlib.redirect_stdout(io.StringIO()):
        sat = at.SpatialActionTokenizer(tok, num_bins=cfg["num_bins"], gs_params=gs0,
                                        use_spherical=cfg["use_spherical"], min_sigma=0.0)
    gen = torch.Generator().manual_seed(11)
    emb = torch.nn.Embedding(sat.vocab_size, E)
    emb.weight.data = torch.randn(sat.vocab_size, E, generator=gen).to(torch.bfloat16)
    out = {"gs0": np.array(json.dumps(gs0)), "gs1": np.array(json.dumps(gs1)),
           "num_bins": np.array(json.dumps(cfg["num_bins"])), "use_spherical": np.array(bool(cfg["use_spherical"])),
           "before": emb.weight.data.view(torch.int16).numpy().view(np.uint16).copy()}
    with contextlib.redirect_stdout(io.StringIO()):
        sat.spatial_embedding_adaption(gs1, emb, min_sigma=0.0, adpt_feature=True)
    out["after"] = emb.weight.data.view(torch.int16).numpy().view(np.uint16).copy()
    for kind, axes in sat.bin_policy.items():
        for axis, edges in axes.items():
            out[f"policy/{kind}/{axis}"] = np.asarray(edges, dtype=np.float64)
    rng = np.random.default_rng(5)
    a = np.clip(rng.normal(0, 0.3, (64, 7)), -1, 1)
    out["actions"] = a
    out["ids"] = np.vectorize(tok.convert_tokens_to_ids)(sat(a)).astype(np.int64)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
