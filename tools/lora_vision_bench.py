"""What the GELU / RESID / SCALE epilogues of svla_lora_up buy on the SigLIP layer of SpatialVLA-4B (hidden 1152,
I 4304, 16 heads, 256 patches; B images, r = 32): the layer forward under no_grad with the adapters on the fused
epilogues, with fc1's GELU as its own pass (SVLA_LORA_GELU_FUSED=0's path), on the unfused composition
(SVLA_LORA_KERNELS=0's path) and without adapters, and each rank-r pass alone against its two-pass form (lora_up
without an epilogue, then svla_gelu_rows / the bf16 add / the bf16 multiply).  Device events around `iters` calls,
alternating rounds, all in one process; prints min / median / max per leg."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from spatialvla_amd import SpatialVLAConfig, functional as Fn, kernels as Kn, presets
from spatialvla_amd.modeling_gemma2 import LoRAAdapter
from spatialvla_amd.modeling_siglip import SiglipEncoderLayer

BF = torch.bfloat16


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = SpatialVLAConfig(**json.loads(json.dumps(presets.spatialvla_4b(use_vision_zoe=False))))
    vc = cfg.vision_config
    layer = SiglipEncoderLayer(vc).to(BF).to(dev)
    r, Lq = a.rank, (vc.image_size // vc.patch_size) ** 2
    M, H, I = a.batch * Lq, vc.hidden_size, vc.intermediate_size
    lins = [getattr(layer.self_attn, n) for n in ("q_proj", "k_proj", "v_proj", "out_proj")] + [layer.mlp.fc1, layer.mlp.fc2]
    with torch.no_grad():
        for p in layer.parameters():
            p.normal_(0, 0.02) if p.dim() == 2 else p.normal_(0, 0.1)
            p.requires_grad_(False)
    ads = [LoRAAdapter((torch.randn(r, l.in_features, device=dev) / r).to(BF),
                       (torch.randn(l.out_features, r, device=dev) * 0.02).to(BF), r, float(r)) for l in lins]
    x = torch.randn(M, H, device=dev).to(BF)

    def attach(on):
        for l, ad in zip(lins, ads):
            if on:
                l.lora = ad
            elif hasattr(l, "lora"):
                del l.lora

    def layer_fwd():
        with torch.no_grad():
            return layer(x, a.batch, Lq)

    def leg(adapters, kernels=True, gelu_fused=True):
        def run():
            attach(adapters)
            Fn.LORA_KERNELS[0], Fn.LORA_GELU_FUSED[0] = kernels, gelu_fused
            try:
                return timed(layer_fwd, a.iters)
            finally:
                Fn.LORA_KERNELS[0], Fn.LORA_GELU_FUSED[0] = True, True
                attach(False)
        return run

    # the rank-r passes alone, at the layer's shapes
    R = Kn.lora_R(r)
    t = torch.randn(M, R, device=dev).to(BF)
    B1, B2 = ads[4].B.data, ads[5].B.data
    cI, hI = torch.randn(M, I, device=dev).to(BF), torch.empty(M, I, dtype=BF, device=dev)
    cH, resH = torch.randn(M, H, device=dev).to(BF), torch.randn(M, H, device=dev).to(BF)
    post = 1.0 / (2304 ** 0.5)

    def two_gelu():
        Kn.lora_up(cI, t, [B1], r)
        Kn.gelu_rows(Kn.GELU_TANH, cI, hI)

    def two_resid():
        Kn.lora_up(cH, t, [B2], r)
        cH.add_(resH)

    def two_scale():
        Kn.lora_up(cH, t, [B2], r)
        cH.mul_(post)

    legs = {
        "layer fwd, no adapters": leg(False),
        "layer fwd, fused epilogues": leg(True),
        "layer fwd, GELU as its own pass": leg(True, gelu_fused=False),
        "layer fwd, composition": leg(True, kernels=False),
        f"lora_up GELU [{M}x{I}] fused": lambda: timed(lambda: Kn.lora_up(cI, t, [B1], r, gelu_out=hI), a.iters),
        f"lora_up + gelu_rows [{M}x{I}]": lambda: timed(two_gelu, a.iters),
        f"lora_up RESID [{M}x{H}] fused": lambda: timed(lambda: Kn.lora_up(cH, t, [B2], r, resid=resH), a.iters),
        f"lora_up + add [{M}x{H}]": lambda: timed(two_resid, a.iters),
        f"lora_up SCALE [{M}x{H}] fused": lambda: timed(lambda: Kn.lora_up(cH, t, [B2], r, post_scale=post), a.iters),
        f"lora_up + mul [{M}x{H}]": lambda: timed(two_scale, a.iters),
    }
    times = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, f in legs.items():
            times[k].append(f())
    print(f"SigLIP layer of SpatialVLA-4B, B = {a.batch} ({M} rows), r = {r}, {a.iters} calls per timing, "
          f"{a.rounds} alternating rounds; us per call")
    for k, v in times.items():
        v = sorted(v)
        print(f"{k:44s} min {v[0]:9.1f}  median {v[len(v) // 2]:9.1f}  max {v[-1]:9.1f}", flush=True)


if __name__ == "__main__":
    main()
