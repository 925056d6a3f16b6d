"""ms/step of a SpatialVLA-4B train step (B = 32 by default) through TrainEngine: full fine-tune, LoRA r = 32 on the
kernels of csrc/lora.hip with the adapter gradients on the main stream (SVLA_LORA_WGRAD_STREAM=0) and on the side
stream (the default), LoRA r = 32 on the unfused composition (SVLA_LORA_KERNELS=0's path), and the side-stream LoRA
step with the frozen base projections in fp8 (enable_fp8_lora) -- with the flat-buffer and optimizer-state bytes of
each and, for the fp8 leg, the bytes of the e4m3 weight copies.  --targets picks the adapter set of the LoRA legs:
gemma2-linear (the seven Gemma2 projections, the default), spatialvla-linear (those plus SigLIP, projector and Ego3D:
the reference's default recipe), spatialvla-linear+emb (plus the Embedding adapter on spatial_embed_tokens) or
spatialvla-linear+emb+h (plus lm_head); several = every LoRA leg once per set in one process, alternating.
--modules-to-save spatial_embed_tokens trains the spatial table in full beside the adapters (the reference's
--adapt_emb --adpt_feature recipe; sets without the Embedding adapter only).  The model and batches are bench.py's
(same random init, same synthetic OXE batches)."""
import argparse
import gc
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
from spatialvla_amd import functional as Fn, presets
from spatialvla_amd.engine import TrainEngine


def run(name, cfgd, args, lora, kernels, side=False, fp8=False, targets="gemma2-linear"):
    dev = torch.device("cuda", 0)
    saved = (Fn.LORA_KERNELS[0], Fn.LORA_WGRAD_STREAM[0])
    model = bench.build_model(cfgd, dev)
    if lora:
        mts = args.modules_to_save if "+emb" not in targets else None
        model.add_lora(args.rank, float(args.rank), target_modules=targets, seed=0, modules_to_save=mts)
    if fp8:
        model.enable_fp8_lora()
    Fn.LORA_KERNELS[0] = kernels
    Fn.LORA_WGRAD_STREAM[0] = side
    total = args.warmup + args.steps
    eng = TrainEngine(model, lr=2e-5, weight_decay=0.0, max_grad_norm=1.0, warmup_ratio=0.005,
                      total_steps=max(total, 10), defer_host_checks=True)
    batches = [bench.make_batch(cfgd, args.batch, 1 + s, dev) for s in range(total)]
    for s in range(args.warmup):
        eng.train_step(batches[s])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = None
    for s in range(args.steps):
        loss = eng.train_step(batches[args.warmup + s])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    flat = eng.flat_param.numel() * 2 + eng.flat_grad.numel() * 2
    opt = (eng.master.numel() + eng.m.numel() + eng.v.numel()) * 4
    copies = 0
    for layer in model.language_model.model.layers:
        f8 = getattr(layer.mlp, "_svla_fp8_lora", None)
        for e in (f8.mats.values() if f8 is not None else ()):
            if isinstance(e, dict):
                copies += sum(e[k].numel() for k in ("q", "qt") if k in e)
                copies += sum(e[k].buf.numel() for k in ("s", "st") if k in e and hasattr(e[k], "buf"))
    print(f"{name:42s} {ms:8.2f} ms/step  loss {float(loss):.4f}  trainable {len(eng.params)} tensors "
          f"{eng.numel / 1e6:9.2f} M elems  flat param+grad {flat / 2**20:9.1f} MiB  optimizer state "
          f"{opt / 2**20:9.1f} MiB  peak alloc {torch.cuda.max_memory_allocated() / 2**30:6.1f} GiB"
          + (f"  e4m3 weight copies {copies / 2**20:7.1f} MiB" if fp8 else ""), flush=True)
    Fn.LORA_KERNELS[0], Fn.LORA_WGRAD_STREAM[0] = saved
    del eng, model, batches
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return ms


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="spatialvla_4b", choices=["spatialvla_4b", "tiny"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=1,
                    help="repeat the list of configurations this many times, alternating them; prints min / median / max")
    ap.add_argument("--only", default="", help="comma list of: full, lora, lora-sidestream, lora-composed, lora-fp8")
    ap.add_argument("--targets", nargs="+", default=["gemma2-linear"],
                    choices=["gemma2-linear", "spatialvla-linear", "spatialvla-linear+emb", "spatialvla-linear+emb+h"],
                    help="adapter set(s) of the LoRA legs; several values run every LoRA leg once per set")
    ap.add_argument("--modules-to-save", default=None, choices=["spatial_embed_tokens"],
                    help="train the spatial table in full beside the adapters (sets without the Embedding adapter)")
    a = ap.parse_args()
    import json
    cfgd = json.loads(json.dumps(getattr(presets, a.config)()))
    only = set(a.only.split(",")) if a.only else None
    cfgs = [c for c in (("full", False, True, False), ("lora", True, True, False),
                        ("lora-sidestream", True, True, True), ("lora-composed", True, False, False),
                        ("lora-fp8", True, True, True, True))
            if only is None or c[0] in only]
    # one leg per adapter set for the LoRA configurations (the name carries the set when there are two)
    legs = []
    for name, lora, kern, side, *fp8 in cfgs:
        for tg in (a.targets if lora else a.targets[:1]):
            legs.append((f"{name}/{tg}" if lora and len(a.targets) > 1 else name, lora, kern, side, bool(fp8), tg))
    times = {c[0]: [] for c in legs}
    for rnd in range(a.rounds):
        for name, lora, kern, side, fp8, tg in legs:
            times[name].append(run(f"{name} (r={a.rank})" if lora else name, cfgd, a, lora, kern, side, fp8, tg))
    if a.rounds > 1:
        for name, v in times.items():
            v = sorted(v)
            print(f"{name:42s} over {len(v)} alternating rounds: min {v[0]:.2f}  median {v[len(v) // 2]:.2f}  "
                  f"max {v[-1]:.2f} ms/step", flush=True)
