"""Inference latency of SpatialVLA-4B greedy decode on one MI355X (BASELINE configs[1]: 1 image + prompt ->
action tokens, bf16), KV-cached (predict_action) beside the uncached re-forward (predict_action_uncached).

Prints one JSON line: prefill ms (SigLIP + Ego3D/Zoe + 299-token Gemma2 prefill + first token), ms per cached
decode token, and that step's weight-streaming roofline — a decode step at B=1 reads every Gemma2 weight and
the lm_head once (algorithmic bytes = their bf16 size), so achieved GB/s = bytes / step time against 8 TB/s.
Synthetic OXE-shaped prompt, random-init weights.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    times.sort()
    return times[len(times) // 2], out


def lora_main(args):
    """--lora R: ms per decode token (and prefill + first token) of three variants in one process, three alternating
    rounds: the adapters merged into the weights (the base path), unmerged on svla_lora_gemv_down / svla_lora_gemv
    (enable_lora_decode), and unmerged composed from the training-path kernels (SVLA_LORA_DECODE_KERNELS=0).  One model
    per variant, each warmed up (and its graphs captured) under its own setting, so the rounds only replay.
    --lora-targets spatialvla-linear+emb / +emb+h: the same three with the Embedding (and lm_head) adapter attached
    (enable_lora_decode(True, emb_head=True): svla_lora_embed_decode / svla_lora_head_gemv at the two ends), and the
    variant adapters_kernels_ends_composed (SVLA_LORA_DECODE_EMB_HEAD_KERNELS=0: the layers' GEMVs kept, the two ends
    composed), which isolates the two new kernels."""
    from bench import build_model, make_batch
    from spatialvla_amd import functional as Fn, presets
    dev = torch.device("cuda:0")
    cfgd = json.loads(json.dumps(presets.spatialvla_4b()))
    b = make_batch(cfgd, args.batch, 4321, dev)
    P = int((b["token_type_ids"][0] == 0).sum())
    inputs = {"input_ids": b["input_ids"][:, :P], "pixel_values": b["pixel_values"], "intrinsic": b["intrinsic"]}
    n_long = args.new_tokens + args.long
    ends = "+emb" in args.lora_targets
    variants = args.variants.split(",")
    if ends and args.variants == VARIANTS:
        variants.append("adapters_kernels_ends_composed")
    models, toks = {}, {}
    for name in variants:
        m = build_model(cfgd, dev).eval()
        m.add_lora(args.lora, float(args.lora), target_modules=args.lora_targets, seed=1)
        gen = torch.Generator(device="cpu").manual_seed(2)
        with torch.no_grad():
            for _, lin in m._lora_linears():  # a trained adapter: B away from its zero initialisation
                lin.lora.B.copy_((torch.randn(lin.lora.B.shape, generator=gen) * 0.01).to(torch.bfloat16))
            if ends:  # the Embedding adapter starts at A = 0, the lm_head adapter at B = 0
                ad = m.spatial_embed_tokens.lora
                ad.A.copy_((torch.randn(ad.A.shape, generator=gen) * 0.01).to(torch.bfloat16))
                ad = getattr(m.language_model.lm_head, "lora", None)
                if ad is not None:
                    ad.B.copy_((torch.randn(ad.B.shape, generator=gen) * 0.01).to(torch.bfloat16))
        if name == "merged":
            m.merge_lora()
        else:
            m.enable_lora_decode(True, emb_head=ends)
        Fn.LORA_DECODE_KERNELS[0] = name != "adapters_composed"
        Fn.LORA_DECODE_EMB_HEAD_KERNELS[0] = name != "adapters_kernels_ends_composed"
        with torch.no_grad():  # warm-up under the variant's setting: every graph this model replays is captured here
            m.predict_action(inputs, max_new_tokens=1, eos_token_id=-1)
            toks[name] = m.predict_action(inputs, max_new_tokens=n_long, eos_token_id=-1)
        models[name] = m
    Fn.LORA_DECODE_KERNELS[0] = Fn.LORA_DECODE_EMB_HEAD_KERNELS[0] = True
    rounds = []
    with torch.no_grad():
        for _ in range(args.rounds):
            row = {}
            for name, m in models.items():
                t1, _ = timed(lambda: m.predict_action(inputs, max_new_tokens=1, eos_token_id=-1), args.reps)
                tl, _ = timed(lambda: m.predict_action(inputs, max_new_tokens=n_long, eos_token_id=-1),
                              max(3, args.reps // 2))
                row[name] = {"ms_prefill_plus_first": round(t1, 2), "ms_per_decode_token": round((tl - t1) / (n_long - 1), 4)}
            rounds.append(row)
    per = {n: [r[n]["ms_per_decode_token"] for r in rounds] for n in models}
    print(json.dumps({
        "metric": "SpatialVLA-4B greedy decode latency with LoRA adapters", "unit": "ms", "batch": args.batch, "r": args.lora,
        "lora_targets": args.lora_targets,
        "prompt_tokens": P, "decode_tokens_timed": n_long - 1, "rounds": rounds,
        "ms_per_decode_token_min_max": {n: [min(v), max(v)] for n, v in per.items()},
        "kernels_tokens_equal_composed": (bool(torch.equal(toks["adapters_kernels"], toks["adapters_composed"]))
                                          if "adapters_kernels" in toks and "adapters_composed" in toks else None),
        "kernels_tokens_equal_ends_composed": (bool(torch.equal(toks["adapters_kernels"],
                                                                toks["adapters_kernels_ends_composed"]))
                                               if "adapters_kernels_ends_composed" in toks and "adapters_kernels" in toks
                                               else None),
        "decode_graphs": bool(next(iter(models.values())).decode_graphs), "dtype": "bf16",
        "data": "synthetic OXE-shaped prompt, random-init weights and adapters"}), flush=True)


VARIANTS = "merged,adapters_kernels,adapters_composed"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--new-tokens", type=int, default=4)
    ap.add_argument("--long", type=int, default=36, help="extra tokens for the per-token slope")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-uncached", action="store_true")
    ap.add_argument("--lora", type=int, default=0, metavar="R",
                    help="rank-R adapters: merged vs unmerged (adapter GEMVs) vs unmerged (composed), three rounds")
    ap.add_argument("--lora-targets", default="gemma2-linear",
                    help="--lora: the target set (gemma2-linear, spatialvla-linear, spatialvla-linear+emb, "
                         "spatialvla-linear+emb+h)")
    ap.add_argument("--variants", default=VARIANTS,
                    help="--lora: which of merged, adapters_kernels, adapters_composed (with an +emb set also "
                         "adapters_kernels_ends_composed, added by default) to run (a kernel trace takes one)")
    ap.add_argument("--rounds", type=int, default=3, help="--lora: alternating rounds")
    args = ap.parse_args()
    if args.lora:
        return lora_main(args)
    from bench import build_model, make_batch
    from spatialvla_amd import presets
    dev = torch.device("cuda:0")
    cfgd = json.loads(json.dumps(presets.spatialvla_4b()))
    model = build_model(cfgd, dev).eval()
    b = make_batch(cfgd, args.batch, 4321, dev)
    P = int((b["token_type_ids"][0] == 0).sum())  # prompt = image tokens + bos + prompt ids + "\n"
    inputs = {"input_ids": b["input_ids"][:, :P], "pixel_values": b["pixel_values"], "intrinsic": b["intrinsic"]}

    n_new, n_long = args.new_tokens, args.new_tokens + args.long
    pa = lambda n: model.predict_action(inputs, max_new_tokens=n, eos_token_id=-1)  # noqa: E731
    with torch.no_grad():
        pa(n_long)  # warm-up: kernel loads, hipBLASLt plans, and the decode-step graphs of every position
        t1, _ = timed(lambda: pa(1), args.reps)
        tn, toks = timed(lambda: pa(n_new), args.reps)
        tl, _ = timed(lambda: pa(n_long), max(3, args.reps // 2))
        per_tok = (tl - t1) / (n_long - 1)
        graphs_on = model.decode_graphs
        model.decode_graphs = False
        toks_eager = pa(n_new)
        model.decode_graphs = graphs_on
        res_unc = None
        if not args.no_uncached:
            tu, toks_u = timed(lambda: model.predict_action_uncached(inputs, max_new_tokens=n_new, eos_token_id=-1),
                               max(2, args.reps // 2))
            res_unc = {"ms": round(tu, 2), "tokens_equal": bool(torch.equal(toks, toks_u))}
    lm = model.language_model
    wbytes = sum(p.numel() * p.element_size() for p in lm.model.layers.parameters())
    wbytes += lm.lm_head.weight.numel() * lm.lm_head.weight.element_size()
    wbytes += lm.model.norm.weight.numel() * lm.model.norm.weight.element_size()
    gbs = wbytes / (per_tok * 1e-3) / 1e9
    graphs = bool(model.decode_graphs)
    print(json.dumps({
        "metric": "SpatialVLA-4B greedy decode latency (BASELINE configs[1])", "unit": "ms", "batch": args.batch,
        "prompt_tokens": P, "new_tokens": n_new, "ms_total": round(tn, 2), "ms_prefill_plus_first": round(t1, 2),
        "ms_per_decode_token": round(per_tok, 3), "tokens_per_s_decode": round(1000.0 * args.batch / per_tok, 1),
        "uncached": res_unc, "decode_graphs": graphs, "graph_tokens_equal_eager": bool(torch.equal(toks, toks_eager)),
        "decode_roofline": {"bound": "hbm", "algorithmic_bytes_per_token_step": wbytes, "achieved": round(gbs, 1),
                            "peak": 8000.0, "unit": "GB/s", "frac": round(gbs / 8000.0, 4)},
        "dtype": "bf16", "data": "synthetic OXE-shaped prompt, random-init weights"}), flush=True)


if __name__ == "__main__":
    main()
