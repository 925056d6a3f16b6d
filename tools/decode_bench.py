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


def algorithmic_bytes_per_token_step(lm):
    """The bf16 bytes a decode step streams: every Gemma2 layer weight, the final norm and lm_head once (the
    decode_roofline.algorithmic_bytes_per_token_step of the default mode's JSON line)."""
    n = sum(p.numel() * p.element_size() for p in lm.model.layers.parameters())
    n += lm.lm_head.weight.numel() * lm.lm_head.weight.element_size()
    return n + lm.model.norm.weight.numel() * lm.model.norm.weight.element_size()


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


def fp8_main(args):
    """--fp8: ms per decode token of the bf16 decode and of the weight-only MX fp8 decode (enable_fp8_decode) in one
    process, alternating rounds (one model each, warmed up and captured under its own setting, so the rounds only
    replay), the bytes a token streams in each, the achieved GB/s against the 8 TB/s spec and the 6.3 TB/s measured copy
    rate, the share of the greedy tokens on which the two agree, and a per-kernel table of the step: every projection
    kernel of both paths timed over the 26 layers' own weights back to back (cold weights, as in the step)."""
    from bench import build_model, make_batch
    from spatialvla_amd import functional as Fn, kernels as K, presets
    dev = torch.device("cuda:0")
    cfgd = json.loads(json.dumps(presets.spatialvla_4b()))
    b = make_batch(cfgd, args.batch, 4321, dev)
    P = int((b["token_type_ids"][0] == 0).sum())
    inputs = {"input_ids": b["input_ids"][:, :P], "pixel_values": b["pixel_values"], "intrinsic": b["intrinsic"]}
    n_long = args.new_tokens + args.long
    models, toks = {}, {}
    for name in ("bf16", "fp8"):
        m = build_model(cfgd, dev).eval()
        if name == "fp8":
            m.enable_fp8_decode()
        with torch.no_grad():
            m.predict_action(inputs, max_new_tokens=1, eos_token_id=-1)
            toks[name] = m.predict_action(inputs, max_new_tokens=n_long, eos_token_id=-1)
        models[name] = m
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
    lm = models["bf16"].language_model
    norms = sum(p.numel() * p.element_size() for n, p in lm.model.named_parameters() if "norm" in n)
    nbytes = {"bf16": sum(p.numel() * p.element_size() for p in lm.model.layers.parameters())
              + lm.lm_head.weight.numel() * lm.lm_head.weight.element_size()
              + lm.model.norm.weight.numel() * lm.model.norm.weight.element_size(),
              "fp8": sum(h.nbytes() for h in models["fp8"].language_model.fp8_decode_holders()) + norms}
    best = {n: min(v) for n, v in per.items()}
    gbs = {n: nbytes[n] / (best[n] * 1e-3) / 1e9 for n in models}

    # per-kernel table: one launch per layer over that layer's own weights, the median of `reps` such sweeps; every row
    # calls the kernel bindings directly on preallocated outputs, so the rows carry the same host cost per launch
    tc = lm.config
    H, I = tc.hidden_size, tc.intermediate_size
    qd = tc.num_attention_heads * tc.head_dim
    kd = tc.num_key_value_heads * tc.head_dim
    M = args.batch
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(dev)  # noqa: E731
    res, y, attn, hout = rnd(M, H), rnd(M, H), rnd(M, qd), torch.empty(M, H, dtype=torch.bfloat16, device=dev)
    qkv, out = (torch.empty(M, n, dtype=torch.bfloat16, device=dev) for n in (qd + 2 * kd, H))
    hact, gbuf, ubuf = (torch.empty(M, I, dtype=torch.bfloat16, device=dev) for _ in range(3))
    tgt = torch.full((M,), -1, dtype=torch.int64, device=dev)

    def sweep(fn, layers):
        def run():
            for l in layers:
                fn(l)
        with torch.no_grad():
            run()
            t, _ = timed(run, args.reps)
        return t * 1e3 / len(layers)

    table = {}
    for name, m in models.items():
        layers = list(m.language_model.model.layers)
        f8 = name == "fp8"

        def pre(l):
            pa, pf = l.post_attention_layernorm, l.pre_feedforward_layernorm
            return (res, y, pa.weight, pf.weight, pa.eps, pf.eps, hout)

        def k_qkv(l):
            ws = [l.self_attn.q_proj.weight, l.self_attn.k_proj.weight, l.self_attn.v_proj.weight]
            if f8:
                K.gemv_mxfp8(None, *l._svla_fp8_decode.get("qkv", ws), qkv, norm=pre(l))
            else:
                K.gemv_rmsnorm2(*pre(l), ws, qkv)

        def k_o(l):
            if f8:
                K.gemv_mxfp8(attn, *l._svla_fp8_decode.get("o", [l.self_attn.o_proj.weight]), out)
            else:
                K.linear_fwd(attn, [l.self_attn.o_proj.weight], out)

        def k_mlp(l):
            wg, wu, wd = l.mlp.gate_proj.weight, l.mlp.up_proj.weight, l.mlp.down_proj.weight
            if f8:  # the two launches of Fn.gemma_mlp_decode(f8d=...)
                K.gemv_mxfp8(None, *l._svla_fp8_decode.get("gate_up", [wg, wu]), hact, geglu_out=(gbuf, ubuf),
                             norm=pre(l))
                K.gemv_mxfp8(hact, *l._svla_fp8_decode.get("down", [wd]), out)
            elif Fn.persist_ok(y, wg, wu, wd):  # the one persistent launch of Fn.gemma_mlp_decode
                K.decode_mlp(*pre(l), wg, wu, wd, hact, out)
            else:
                K.gemv_rmsnorm2(*pre(l), [wg, wu], hact, geglu_out=(gbuf, ubuf))
                K.linear_fwd(hact, [wd], out)

        hrow = rnd(M, 1, H)
        table[name] = {"qkv_with_norm_pair_us": round(sweep(k_qkv, layers), 2), "o_us": round(sweep(k_o, layers), 2),
                       "mlp_with_norm_pair_us": round(sweep(k_mlp, layers), 2),
                       "head_us": round(sweep(lambda _l: m.language_model.head(hrow, tgt, {}, decode=True), [None]), 2)}
        table[name]["sum_per_step_us"] = round(sum(table[name][k] * (1 if k == "head_us" else len(layers))
                                                   for k in list(table[name])), 1)
    agree = float((toks["bf16"] == toks["fp8"]).float().mean())
    print(json.dumps({
        "metric": "SpatialVLA-4B greedy decode latency, bf16 against weight-only MX fp8 decode", "unit": "ms",
        "batch": args.batch, "prompt_tokens": P, "decode_tokens_timed": n_long - 1, "rounds": rounds,
        "ms_per_decode_token_min_max": {n: [min(v), max(v)] for n, v in per.items()},
        "bytes_per_token": nbytes,
        "achieved_GBps": {n: round(v, 1) for n, v in gbs.items()},
        "frac_of_8TBps_spec": {n: round(v / 8000.0, 4) for n, v in gbs.items()},
        "frac_of_6p3TBps_copy": {n: round(v / 6300.0, 4) for n, v in gbs.items()},
        "greedy_tokens": n_long, "tokens_agree_share": round(agree, 4),
        "kernels": table,
        "kernels_note": "wall us per eager launch (host launch cost included: an upper bound of the kernel time, not a "
                        "kernel trace), one launch per layer over that layer's weights, kernel bindings on preallocated "
                        "outputs (head: the model's head() on lm_head, warm, with its allocations); the bf16 mlp is the "
                        "persistent svla_decode_mlp, the fp8 mlp the norm-prologue gate|up GEMV + the down GEMV",
        "decode_graphs": bool(models["bf16"].decode_graphs),
        "data": "synthetic OXE-shaped prompt, random-init weights"}), flush=True)


def lora_fp8_main(args):
    """--lora R --fp8: ms per decode token of three variants in one process, alternating rounds (one model each, warmed
    up and captured under its own setting, so the rounds only replay): the adapters merged into the bf16 weights, the
    adapters unmerged on the bf16 adapter GEMVs (enable_lora_decode: the yardstick), and unmerged over the e4m3 copies
    of the frozen base weights (enable_fp8_lora_decode).  Also the bytes a token streams in each, the share of the
    greedy tokens on which the two unmerged legs agree (and, beside it, the two bf16 legs: random-init weights leave
    small margins, so a greedy sequence rarely survives its first differing token), and the rel-L2 between the two
    unmerged legs' logits of one teacher-forced decode step -- the quantisation error of the e4m3 base weights."""
    from bench import build_model, make_batch
    from spatialvla_amd import presets
    dev = torch.device("cuda:0")
    cfgd = json.loads(json.dumps(presets.spatialvla_4b()))
    b = make_batch(cfgd, args.batch, 4321, dev)
    P = int((b["token_type_ids"][0] == 0).sum())
    inputs = {"input_ids": b["input_ids"][:, :P], "pixel_values": b["pixel_values"], "intrinsic": b["intrinsic"]}
    n_long = args.new_tokens + args.long
    ends = "+emb" in args.lora_targets
    models, toks, nbytes = {}, {}, {}
    for name in ("merged", "adapters_bf16", "adapters_fp8"):
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
        lm = m.language_model
        ads = [lin.lora for _, lin in m._lora_linears()] + [a for a in (getattr(lm.lm_head, "lora", None),) if a]
        adapters = sum(t.numel() * t.element_size() for ad in ads for t in (ad.A, ad.B))
        norms = sum(p.numel() * p.element_size() for n, p in lm.model.named_parameters() if "norm" in n)
        base = (sum(lin.weight.numel() * lin.weight.element_size() for _, lin in m._lora_linears())
                + lm.lm_head.weight.numel() * lm.lm_head.weight.element_size())
        if name == "merged":
            m.merge_lora()
            adapters = 0
        else:
            m.enable_lora_decode(True, emb_head=ends)
            if name == "adapters_fp8":
                m.enable_fp8_lora_decode()
        with torch.no_grad():  # warm-up under the variant's setting: every graph this model replays is captured here
            m.predict_action(inputs, max_new_tokens=1, eos_token_id=-1)
            toks[name] = m.predict_action(inputs, max_new_tokens=n_long, eos_token_id=-1)
        if name == "adapters_fp8":
            base = sum(h.nbytes() for h in lm.fp8_lora_decode_holders())
        nbytes[name] = base + norms + adapters
        models[name] = m
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
    best = {n: min(v) for n, v in per.items()}
    agree = float((toks["adapters_bf16"] == toks["adapters_fp8"]).float().mean())
    agree_bf16 = float((toks["adapters_bf16"] == toks["merged"]).float().mean())

    def step_logits(m):  # the prompt, then the bf16 leg's first token through the KV-cached step
        with torch.no_grad():
            cache = m(**inputs, use_cache=True).past_key_values
            return m(input_ids=toks["adapters_bf16"][:, :1], past_key_values=cache).logits.float()

    lb, lf = step_logits(models["adapters_bf16"]), step_logits(models["adapters_fp8"])
    step_rel = float((lf - lb).norm() / lb.norm())
    print(json.dumps({
        "metric": "SpatialVLA-4B greedy decode latency with unmerged LoRA adapters, bf16 against e4m3 base weights",
        "unit": "ms", "batch": args.batch, "r": args.lora, "lora_targets": args.lora_targets, "prompt_tokens": P,
        "decode_tokens_timed": n_long - 1, "rounds": rounds,
        "ms_per_decode_token_min_max": {n: [min(v), max(v)] for n, v in per.items()},
        "bytes_per_token": nbytes,
        "achieved_GBps": {n: round(nbytes[n] / (best[n] * 1e-3) / 1e9, 1) for n in models},
        "e4m3_copies_bytes": sum(h.nbytes() for h in models["adapters_fp8"].language_model.fp8_lora_decode_holders()),
        "greedy_tokens": n_long, "unmerged_tokens_agree_share": round(agree, 4),
        "bf16_unmerged_vs_merged_tokens_agree_share": round(agree_bf16, 4),
        "decode_step_logits_rel_l2_fp8_vs_bf16_unmerged": round(step_rel, 5),
        "decode_graphs": bool(models["merged"].decode_graphs),
        "data": "synthetic OXE-shaped prompt, random-init weights and adapters"}), flush=True)


def batched_main(args):
    """--batched: ms per decode step with the batched-decode switch off and on (enable_batched_decode) in one process,
    graph replay, alternating rounds (one model each, warmed up and captured under its own setting, so the rounds only
    replay) at every batch of --batches; a batch of at most 8 rows runs the switch-off model only (the GEMV path, which
    the switch does not touch: the neighbouring point).  Reports ms per step, tokens/s, achieved GB/s against the bf16
    bytes a step streams (algorithmic_bytes_per_token_step) and the rounds' spread, and, at --table-rows rows, the
    time per launch of the five projections of a step on the general GEMM and, for the two the switch routes (q|k|v,
    o), on svla_gemm_skinny, each swept over the 26 layers' own weights inside one captured graph (device time, cold
    weights as in the step)."""
    from bench import build_model, make_batch
    from spatialvla_amd import functional as Fn, kernels as K, presets
    dev = torch.device("cuda:0")
    cfgd = json.loads(json.dumps(presets.spatialvla_4b()))
    n_long = args.new_tokens + args.long
    models = {"off": build_model(cfgd, dev).eval(), "on": build_model(cfgd, dev).eval()}
    models["on"].enable_batched_decode()
    for m in models.values():  # the depth estimator's convolutions take at most 2 GiB of input: 8 images a call
        m.predict_depth = lambda pv, _f=m.predict_depth: torch.cat([_f(pv[i:i + 8]) for i in range(0, pv.shape[0], 8)], 0)
    lm = models["off"].language_model
    wbytes = algorithmic_bytes_per_token_step(lm)
    results = []
    for batch in [int(v) for v in args.batches.split(",") if v and v != "none"]:
        b = make_batch(cfgd, batch, 4321, dev)
        P = int((b["token_type_ids"][0] == 0).sum())
        inputs = {"input_ids": b["input_ids"][:, :P], "pixel_values": b["pixel_values"], "intrinsic": b["intrinsic"]}
        names = ["off", "on"] if batch >= Fn.BATCHED_DECODE_MIN_ROWS else ["off"]
        toks, rounds = {}, []
        with torch.no_grad():
            for name in names:  # warm-up: every graph the rounds replay is captured here
                models[name].predict_action(inputs, max_new_tokens=1, eos_token_id=-1)
                toks[name] = models[name].predict_action(inputs, max_new_tokens=n_long, eos_token_id=-1)
            for _ in range(args.rounds):
                row = {}
                for name in names:
                    m = models[name]
                    t1, _ = timed(lambda: m.predict_action(inputs, max_new_tokens=1, eos_token_id=-1), args.reps)
                    tl, _ = timed(lambda: m.predict_action(inputs, max_new_tokens=n_long, eos_token_id=-1), args.reps)
                    row[name] = round((tl - t1) / (n_long - 1), 4)
                rounds.append(row)
        per = {n: [r[n] for r in rounds] for n in names}
        med = {n: sorted(v)[len(v) // 2] for n, v in per.items()}
        res = {"batch": batch, "prompt_tokens": P, "decode_steps_timed": n_long - 1, "rounds_ms_per_step": rounds,
               "ms_per_step_median": med, "ms_per_step_min_max": {n: [min(v), max(v)] for n, v in per.items()},
               "tokens_per_s": {n: round(1000.0 * batch / v, 1) for n, v in med.items()},
               "achieved_GBps": {n: round(wbytes / (v * 1e-3) / 1e9, 1) for n, v in med.items()}}
        if "on" in names:
            spread = max(max(v) - min(v) for v in per.values())
            res["spread_ms"] = round(spread, 4)
            res["on_minus_off_ms"] = round(med["on"] - med["off"], 4)
            res["on_beats_off_by_more_than_spread"] = bool(med["off"] - med["on"] > spread)
            res["tokens_agree_share"] = round(float((toks["on"] == toks["off"]).float().mean()), 4)
        results.append(res)
        for m in models.values():
            m.clear_decode_cache()
        print(json.dumps(res), file=sys.stderr, flush=True)

    # per-launch table: the five routed projections at --table-rows rows, one launch per layer inside one graph
    tables = {}
    for M in [int(v) for v in str(args.table_rows).split(",")]:
        tables[str(M)] = _batched_table(args, K, lm, M, dev)
    print(json.dumps({
        "metric": "SpatialVLA-4B batched greedy decode, enable_batched_decode off against on", "unit": "ms per decode step",
        "algorithmic_bytes_per_token_step": wbytes, "window_rows": [Fn.BATCHED_DECODE_MIN_ROWS, Fn.BATCHED_DECODE_MAX_ROWS],
        "batches": results, "per_launch_us_by_rows": tables,
        "per_launch_note": "device time per launch: one launch per layer over that layer's own weights (lm_head: one "
                           "launch), the sweep captured in one graph and replayed; general_gemm = svla_gemm_bf16 "
                           "through linear_fwd / linear_geglu_fwd, gemm_skinny = the two projections the switch routes",
        "decode_graphs": bool(models["off"].decode_graphs), "dtype": "bf16",
        "data": "synthetic OXE-shaped prompt, random-init weights"}), flush=True)


def _batched_table(args, K, lm, M, dev):
    """The five projections of a step at M rows on the general GEMM, q|k|v and o also on svla_gemm_skinny: us per launch."""
    tc = lm.config
    H, I, V = tc.hidden_size, tc.intermediate_size, lm.lm_head.weight.shape[0]
    qd, kd = tc.num_attention_heads * tc.head_dim, tc.num_key_value_heads * tc.head_dim
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(dev)  # noqa: E731
    x, attn, hin = rnd(M, H), rnd(M, qd), rnd(M, I)
    qkv, out = (torch.empty(M, n, dtype=torch.bfloat16, device=dev) for n in (qd + 2 * kd, H))
    hact, gbuf, ubuf = (torch.empty(M, I, dtype=torch.bfloat16, device=dev) for _ in range(3))
    logits = torch.empty(M, K.round_up(V, 64), dtype=torch.bfloat16, device=dev)
    layers = list(lm.model.layers)

    def sweep(fn, over):
        def run():
            for l in over:
                fn(l)
        with torch.no_grad():
            run()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                run()
            gr.replay()
            t, _ = timed(gr.replay, max(5, args.reps))
        return round(t * 1e3 / len(over), 2)

    att = lambda l: l.self_attn  # noqa: E731
    table = {
        "general_gemm": {
            "qkv_us": sweep(lambda l: K.linear_fwd(x, [att(l).q_proj.weight, att(l).k_proj.weight, att(l).v_proj.weight],
                                                   qkv), layers),
            "o_us": sweep(lambda l: K.linear_fwd(attn, [att(l).o_proj.weight], out), layers),
            "gate_up_geglu_us": sweep(lambda l: K.linear_geglu_fwd(x, l.mlp.gate_proj.weight, l.mlp.up_proj.weight, hact,
                                                                   gbuf, ubuf), layers),
            "down_us": sweep(lambda l: K.linear_fwd(hin, [l.mlp.down_proj.weight], out), layers),
            "lm_head_us": sweep(lambda _l: K.linear_fwd(x, [lm.lm_head.weight], logits[:, :V]), [None])},
        "gemm_skinny": {
            "qkv_us": sweep(lambda l: K.gemm_skinny(x, [att(l).q_proj.weight, att(l).k_proj.weight, att(l).v_proj.weight],
                                                    qkv), layers),
            "o_us": sweep(lambda l: K.gemm_skinny(attn, [att(l).o_proj.weight], out), layers)}}
    return table


def sample_main(args):
    """--sample (with --batched and / or --fp8 applied to both models): ms per decode step of greedy decoding with
    enable_sampled_decode off, and with it on for the greedy form and three sampling settings -- the full vocabulary
    (temperature 1, no filter), top_k 50 / top_p 0.95 at temperature 0.7, and temperature 1 inside the action-token
    ranges -- in one process, graph replay, alternating rounds, at every batch of --batches (default 1,16).  The
    settings live in the device block, so the four switch-on legs replay the same graphs.  Also svla_sample_rows
    alone at the model's vocabulary for M = 1, 16, 64 rows: device time per launch inside one captured graph."""
    from bench import build_model, make_batch
    from spatialvla_amd import kernels as K, presets
    dev = torch.device("cuda:0")
    cfgd = json.loads(json.dumps(presets.spatialvla_4b()))
    n_long = args.new_tokens + args.long
    n_long += (-n_long) % 3  # whole actions under the range constraint
    models = {"off": build_model(cfgd, dev).eval(), "on": build_model(cfgd, dev).eval()}
    models["on"].enable_sampled_decode()
    for m in models.values():
        if args.batched:
            m.enable_batched_decode()
        if args.fp8:
            m.enable_fp8_decode()
        m.predict_depth = lambda pv, _f=m.predict_depth: torch.cat([_f(pv[i:i + 8]) for i in range(0, pv.shape[0], 8)], 0)
    r = models["on"].action_token_ranges()
    ranges = [(r[0], r[1] + 1), (r[2], r[3] + 1), (r[4], r[5] + 1)]
    legs = {"off_greedy": ("off", {}), "on_greedy": ("on", {}),
            "on_full_vocab_T1": ("on", dict(do_sample=True, seed=1)),
            "on_T0.7_k50_p0.95": ("on", dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.95, seed=1)),
            "on_action_ranges_T1": ("on", dict(do_sample=True, seed=1, allowed_ranges=ranges))}
    results = []
    for batch in [int(v) for v in (args.batches or "1,16").split(",")]:
        b = make_batch(cfgd, batch, 4321, dev)
        P = int((b["token_type_ids"][0] == 0).sum())
        inputs = {"input_ids": b["input_ids"][:, :P], "pixel_values": b["pixel_values"], "intrinsic": b["intrinsic"]}
        run = lambda leg, n: models[legs[leg][0]].predict_action(  # noqa: E731
            inputs, max_new_tokens=n, eos_token_id=-1, **legs[leg][1])
        toks, rounds = {}, []
        with torch.no_grad():
            for leg in legs:  # warm-up: every graph the rounds replay is captured here
                run(leg, 1)
                toks[leg] = run(leg, n_long)
            for _ in range(args.rounds):
                row = {}
                for leg in legs:
                    t1, _ = timed(lambda: run(leg, 1), args.reps)
                    tl, _ = timed(lambda: run(leg, n_long), args.reps)
                    row[leg] = round((tl - t1) / (n_long - 1), 4)
                rounds.append(row)
        per = {n: [r_[n] for r_ in rounds] for n in legs}
        med = {n: sorted(v)[len(v) // 2] for n, v in per.items()}
        res = {"batch": batch, "prompt_tokens": P, "decode_steps_timed": n_long - 1, "rounds_ms_per_step": rounds,
               "ms_per_step_median": med, "ms_per_step_min_max": {n: [min(v), max(v)] for n, v in per.items()},
               "spread_ms": round(max(max(v) - min(v) for v in per.values()), 4),
               "minus_off_greedy_ms": {n: round(med[n] - med["off_greedy"], 4) for n in legs if n != "off_greedy"},
               "on_greedy_tokens_equal_off": bool(torch.equal(toks["on_greedy"], toks["off_greedy"]))}
        results.append(res)
        for m in models.values():
            m.clear_decode_cache()
        print(json.dumps(res), file=sys.stderr, flush=True)

    # the kernel alone: 20 launches over the same logits in one captured graph, device time per launch
    V = models["on"].language_model.lm_head.weight.shape[0]
    ld = K.round_up(V, 64)
    g = torch.Generator(device="cpu").manual_seed(3)
    rtab = torch.tensor(ranges, dtype=torch.int32, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    kernel = {}
    for M in (1, 16, 64):
        x = torch.randn(M, ld, generator=g) * 4.0
        logits = (30.0 * torch.tanh(x / 30.0)).to(torch.bfloat16).to(dev)
        out = (torch.empty(M, dtype=torch.int64, device=dev), torch.empty(M, dtype=torch.float32, device=dev),
               torch.empty(M, dtype=torch.float32, device=dev))
        row = {}
        for name, (T, k, p, nr) in {"greedy": (0.0, 0, 1.0, 0), "full_vocab_T1": (1.0, 0, 1.0, 0),
                                    "T1_p0.9": (1.0, 0, 0.9, 0), "T0.7_k50_p0.95": (0.7, 50, 0.95, 0),
                                    "action_ranges_T1": (1.0, 0, 1.0, 3)}.items():
            params = K.pack_sample_params(T, p, k, 1, 0, nr).to(dev)

            def launches():
                for i in range(20):
                    K.sample_rows(logits, V, params, 300 + i, None, rtab, step, out=out)
            launches()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                launches()
            gr.replay()
            t, _ = timed(gr.replay, max(5, args.reps))
            row[name] = round(t * 1e3 / 20, 2)
        kernel[str(M)] = row
    print(json.dumps({
        "metric": "SpatialVLA-4B decode, greedy against sampled (enable_sampled_decode)", "unit": "ms per decode step",
        "batched_decode": bool(args.batched), "fp8_decode": bool(args.fp8), "batches": results,
        "sample_rows_us_per_launch_by_rows": kernel, "vocabulary": V,
        "kernel_note": "device time per launch, 20 launches over the same (cache-resident) logits in one captured graph",
        "decode_graphs": bool(models["off"].decode_graphs), "dtype": "bf16",
        "data": "synthetic OXE-shaped prompt, random-init weights"}), flush=True)


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
    ap.add_argument("--rounds", type=int, default=3, help="--lora / --fp8: alternating rounds")
    ap.add_argument("--fp8", action="store_true",
                    help="bf16 against the weight-only MX fp8 decode (enable_fp8_decode), alternating rounds, bytes per "
                         "token, token agreement and a per-kernel table; with --lora R: merged bf16, unmerged on the "
                         "bf16 adapter GEMVs and unmerged over the e4m3 copies (enable_fp8_lora_decode)")
    ap.add_argument("--batched", action="store_true",
                    help="the batched-decode switch (enable_batched_decode) off against on, alternating rounds at every "
                         "batch of --batches, and a per-launch table of the routed projections at --table-rows rows")
    ap.add_argument("--batches", default=None, help="--batched: the batch sizes (default: 8,16,32,48,64; --batch N: 8,N)")
    ap.add_argument("--table-rows", default="16", help="--batched: token rows of the per-launch table (a,b,...)")
    ap.add_argument("--sample", action="store_true",
                    help="greedy against sampled decode (enable_sampled_decode) at every batch of --batches (default "
                         "1,16), alternating rounds, and svla_sample_rows alone; --batched / --fp8 apply to both models")
    args = ap.parse_args()
    if args.sample:
        return sample_main(args)
    if args.batched:
        if args.batches is None:
            args.batches = "8,16,32,48,64" if args.batch == 1 else (f"8,{args.batch}" if args.batch != 8 else "8")
        return batched_main(args)
    if args.lora and args.fp8:
        return lora_fp8_main(args)
    if args.lora:
        return lora_main(args)
    if args.fp8:
        return fp8_main(args)
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
    wbytes = algorithmic_bytes_per_token_step(lm)
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
