"""Isolated times of the LoRA kernels (csrc/lora.hip) at the SpatialVLA-4B shapes (B = 32: M = 9984 rows, r = 32),
beside the unfused composition the same Functions run with SVLA_LORA_KERNELS=0 (svla_gemm_bf16 wrappers + torch
elementwise ops) and beside the byte floor (bytes moved / 8 TB/s).  Each arm is captured into a graph of REPS calls
and replayed (no host launch gaps); best of 3 interleaved rounds.  The operands of consecutive calls are the same
buffers (46-370 MB), so part of them is served from the last-level cache: the fraction of the HBM byte floor printed
here is an upper bound.  One line per (site, product); for gate|up one more: the GeGLU pass that also writes the MX
e4m3 copy of h (enable_fp8_lora) against the pass followed by svla_quant_mx_rows."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from spatialvla_amd import functional as Fn, kernels as K

BF = torch.bfloat16
M, R_, REPS, HBM = 9984, 32, 10, 8e12
# site: (K, [N_s], epilogue)
SITES = {"q|k|v": (2304, [2048, 1024, 1024], "rope"), "o": (2048, [2304], None),
         "gate|up": (2304, [9216, 9216], "geglu"), "down": (9216, [2304], None)}


def _r(*s, scale=1.0):
    return (torch.randn(*s, device="cuda") * scale).to(BF)


def _time(fns):
    """{name: ms per call}: each fn captured REPS times into a graph, replayed; best of 3 interleaved rounds."""
    graphs = {}
    for n, f in fns.items():
        f()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(REPS):
                f()
        graphs[n] = g
    best = {}
    for _ in range(3):
        for n, g in graphs.items():
            g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            best[n] = min(best.get(n, 1e30), e0.elapsed_time(e1) / REPS)
    return best


def bench_site(name, Kd, sizes, epi, r=R_):
    N, ns, R = sum(sizes), len(sizes), K.lora_R(r)
    x, dy, c = _r(M, Kd), _r(M, N, scale=0.1), _r(M, N)
    As = [_r(r, Kd, scale=1.0 / r) for _ in sizes]
    Bs = [_r(n, r, scale=0.02) for n in sizes]
    t = _r(M, ns * R)
    dA = [torch.empty(r, Kd, dtype=BF, device="cuda") for _ in sizes]
    dB = [torch.empty(n, r, dtype=BF, device="cuda") for n in sizes]
    starts = [0]
    for n in sizes:
        starts.append(starts[-1] + n)
    dx = _r(M, Kd)
    kw = {}
    if epi == "rope":
        L, D = 312, 256
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, device="cuda").float() / D))
        fr = (torch.arange(L, device="cuda").float() + 1)[:, None] * inv[None]
        kw["rope"] = (fr.cos().to(BF).contiguous(), fr.sin().to(BF).contiguous(), L, D, sizes[0] + sizes[1])
    elif epi == "geglu":
        kw["geglu_h"] = torch.empty(M, N // 2, dtype=BF, device="cuda")
    small = 2 * ns * r * Kd + 2 * N * r
    rows = []
    for prod, byts, call in (
            ("down fwd  t = x A^T", 2 * M * Kd + 2 * M * ns * R + small, lambda o: o.down(x, As, r)),
            (f"up fwd    y += s t B^T ({epi or 'none'})", 4 * M * N + 2 * M * ns * R + small
             + (M * N if epi == "geglu" else 0), lambda o: o.up(c, t, Bs, r, 1.0, **kw)),
            ("down bwd  dt = s dy B", 2 * M * N + 2 * M * ns * R + small, lambda o: o.down_t(dy, Bs, r, 1.0)),
            ("up bwd    dx += dt A", 4 * M * Kd + 2 * M * ns * R + small, lambda o: o.up_t(dx, t, As, r)),
            ("wgrad dA  = dt^T x", 2 * M * Kd + 2 * M * ns * R + small,
             lambda o: o.wgrad(x, t, [(g, False, None) for g in dA], r, False, 1.0, starts)),
            ("wgrad dB  = s dy^T t", 2 * M * N + 2 * M * ns * R + small,
             lambda o: o.wgrad(dy, t, [(g, False, None) for g in dB], r, True, 1.0, starts))):
        ms = _time({"kernel": lambda: call(Fn._LoraKernelOps), "composed": lambda: call(Fn._LoraComposedOps)})
        floor = byts / HBM * 1e3
        rows.append((prod, ms["kernel"], ms["composed"], floor))
        print(f"{name:8s} K={Kd:5d} N={N:5d} {prod:36s} kernel {ms['kernel'] * 1e3:8.1f} us  composed "
              f"{ms['composed'] * 1e3:8.1f} us  ({ms['composed'] / ms['kernel']:5.2f}x)  floor {floor * 1e3:6.1f} us "
              f"({100 * floor / ms['kernel']:5.1f} % of it)", flush=True)
    if epi == "geglu":  # enable_fp8_lora: the MX e4m3 copy of h from the same pass, against the pass + svla_quant_mx_rows
        h, I = kw["geglu_h"], N // 2
        mx = (torch.empty(M, I, dtype=torch.float8_e4m3fn, device="cuda"), K.MXScales(M, I, "cuda"))
        up = Fn._LoraKernelOps.up

        def two_passes():
            up(c, t, Bs, r, 1.0, **kw)
            K.quant_mx_rows(h, *mx)
        ms = _time({"fused": lambda: up(c, t, Bs, r, 1.0, mx_out=mx, **kw), "plain": lambda: up(c, t, Bs, r, 1.0, **kw),
                    "two": two_passes})
        print(f"{name:8s} K={Kd:5d} N={N:5d} up fwd (geglu) + MX copy of h: one pass {ms['fused'] * 1e3:8.1f} us  "
              f"pass + quant_mx_rows {ms['two'] * 1e3:8.1f} us  pass without the copy {ms['plain'] * 1e3:8.1f} us", flush=True)
    return rows


if __name__ == "__main__":
    torch.manual_seed(0)
    sel = sys.argv[1:]
    tot_k = tot_c = 0.0
    for name, (Kd, sizes, epi) in SITES.items():
        if sel and not any(s in name for s in sel):
            continue
        for _, k, c, _ in bench_site(name, Kd, sizes, epi):
            tot_k += k
            tot_c += c
    print(f"sum over the listed products of one layer: kernel {tot_k:.3f} ms, composed {tot_c:.3f} ms")
