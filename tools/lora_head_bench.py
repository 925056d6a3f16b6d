"""The lm_head adapter's forward pass at SpatialVLA-4B widths (V = 265347, row stride round_up(V, 64), H = 2304,
r = 32): svla_lora_softcap_ce_rows (adapter term + softcap + statistics in one trip over the raw logits) against its
composed form (plain-store GEMM t B^T into a second [rows, ld] buffer, a bf16 add, svla_softcap_ce_rows) and against
svla_softcap_ce_rows alone (what the pass costs without an adapter), over the label rows of a B = 32 step (416) and over
all rows (9984).  Device events around --calls calls per timing, --rounds alternating rounds; the raw logits are
restored from a pristine copy before every timed group (the copy is outside the events).  Also prints the bytes each
form moves, computed from the shapes."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from spatialvla_amd import kernels as K

BF = torch.bfloat16


def timed(fn, reset, calls):
    reset()
    fn()  # warm-up of this shape
    torch.cuda.synchronize()
    tot = 0.0
    for _ in range(calls):
        reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        tot += e0.elapsed_time(e1)
    return tot / calls * 1e3  # us


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=265347)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--rows", type=int, nargs="+", default=[416, 9984])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    V, r, cap = a.vocab, a.rank, 30.0
    ld, R = K.round_up(V, 64), K.lora_R(r)
    gen = torch.Generator(device=dev).manual_seed(0)
    B = (torch.randn(V, r, device=dev, generator=gen) * 0.02).to(BF)
    for rows in a.rows:
        raw0 = (torch.randn(rows, ld, device=dev, generator=gen) * 8).to(BF)
        t = torch.zeros(rows, R, dtype=BF, device=dev)
        t[:, :r] = (torch.randn(rows, r, device=dev, generator=gen) * 0.5).to(BF)
        buf, u = torch.empty_like(raw0), torch.empty_like(raw0)
        stats = torch.empty(rows, K.ceil_div(V, 128), 3, dtype=torch.float32, device=dev)

        def reset():
            buf.copy_(raw0)

        def fused():
            K.lora_softcap_ce_rows(buf, V, t, B, r, 1.0, stats, cap)

        def composed():
            K.linear_fwd(t[:, :r], [B], u[:, :V], alpha=1.0)
            buf[:, :V] += u[:, :V]
            K.softcap_ce_rows(buf, V, stats, cap)

        def plain():
            K.softcap_ce_rows(buf, V, stats, cap)

        # the two forms compute the same values at the timed size (they differ in fp32 summation order only)
        reset(); fused(); f = buf.clone(); sf = stats.clone()
        reset(); composed()
        torch.cuda.synchronize()
        rel = float((f[:, :V].float() - buf[:, :V].float()).norm() / buf[:, :V].float().norm())
        print(f"rows {rows}: fused vs composed logits rel-L2 {rel:.3e}, bit-identical logits "
              f"{torch.equal(f[:, :V], buf[:, :V])}, statistics {torch.equal(sf, stats)}", flush=True)
        legs = (("fused  svla_lora_softcap_ce_rows", fused), ("composed  GEMM + add + softcap_ce_rows", composed),
                ("no adapter  svla_softcap_ce_rows", plain))
        res = {n: [] for n, _ in legs}
        for _ in range(a.rounds):
            for n, fn in legs:
                res[n].append(timed(fn, reset, a.calls))
        lg = rows * ld * 2
        moved = {legs[0][0]: 2 * lg + V * r * 2, legs[1][0]: 6 * lg + V * r * 2, legs[2][0]: 2 * lg}
        for n, v in res.items():
            v = sorted(v)
            print(f"rows {rows:5d}  {n:42s} min {v[0]:9.1f}  median {v[len(v) // 2]:9.1f}  max {v[-1]:9.1f} us   "
                  f"logits + B bytes by shape {moved[n] / 2**20:8.1f} MiB", flush=True)
        del raw0, buf, u, stats, t
        torch.cuda.empty_cache()
