"""float64 reference of the masked attention of include/svla.h (key classes, sliding window, softcap, RoPE) with the
reference's additive-mask gradient, the mask mutations the attention mask tests must tell apart, and the cases they run.
Torch only: tests/test_attention_masks_cpu.py checks the discriminating-power condition of every case without a GPU,
tests/test_attention_masks_gpu.py compares the HIP kernels with the same reference on the same data.

Masked scores take finfo(bf16).min exactly and keep their gradient (where(vis, s, s - s.detach() + MIN)): a row with
no visible key is then exactly uniform over all L keys and its gradient reaches the scores, as through the additive
mask of eager_attention_forward (fp32 s + MIN rounds to MIN; a plain fp64 s + MIN would keep s).
"""
import functools
import math

import torch

BF = torch.bfloat16
MIN = float(torch.finfo(BF).min)
TOL_OUT, TOL_LSE, TOL_GRAD = 1e-2, 1e-4, 2e-2  # the project's own (tests/test_kernels_gpu.py)
MUTANTS = ("w+1", "w-1", "strict", "c2vis", "nowin0")
QUANT = ("out", "dq", "dk", "dv")
TOLS = {"out": TOL_OUT, "dq": TOL_GRAD, "dk": TOL_GRAD, "dv": TOL_GRAD}


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def layout(name, B, L, device="cpu"):
    """Key classes [B, L] uint8 (None: no kv_class); B = 2 gets a different layout per batch element."""
    if name == "none":
        return None
    c = torch.ones(B, L, dtype=torch.uint8)
    if name == "mix":  # class 0 up to L/2, class 1 after, class 2 at 5:9 and on the last 4 keys
        c[:, :L // 2] = 0
        c[0, 5:9] = 2
        c[-1, L - 4:] = 2
    elif name == "few-prefix":  # 3 class-0 keys, the rest class 1, the last 3 class 2
        c[:, :3] = 0
        c[-1, L - 3:] = 2
        c[0, 2] = 1
    elif name == "left-pad":  # all class 1 with the first 6 class 2: rows 0..5 are fully masked
        c[:, :6] = 2
        c[0, 6] = 2 if B > 1 else 1
    elif name == "tile-dead":  # class 2 on one whole 64-key tile between class-1 keys
        c[:, 64:128] = 2
        c[0, 0] = 0
    elif name == "sparse":  # class 1 with class 2 on keys 8..L-9: few keys per row, so a single score weighs
        c[:, 8:L - 8] = 2
        c[0, 8] = 1
    else:
        raise ValueError(name)
    return c.to(device)


def visibility(cls, B, L, window, mut=None, device="cpu"):
    """[B, L(query), L(key)] bool as include/svla.h: class 0 visible, class 1 when j <= i, class 2 never; with a
    window, key j is masked for query i when i - j >= window, for every class.  mut: one of MUTANTS."""
    i = torch.arange(L, device=device)[:, None]
    j = torch.arange(L, device=device)[None, :]
    c = (cls.long() if cls is not None else torch.zeros(B, L, dtype=torch.long, device=device))[:, None, :]
    causal = (j < i) if mut == "strict" else (j <= i)
    vis = (c == 0) | ((c == 1) & causal)
    if mut == "c2vis":
        vis = vis | (c == 2)
    w = window + {"w+1": 1, "w-1": -1}.get(mut, 0) if window > 0 else 0
    if window > 0:
        win = (i - j) < w
        if mut == "nowin0":
            win = win | (c == 0)
        vis = vis & win
    return vis.expand(B, L, L)


def rope_tables(L, D, device="cpu"):
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D))
    f = (torch.arange(L).float() + 1)[:, None] * inv[None]
    return f.cos().to(BF).contiguous().to(device), f.sin().to(BF).contiguous().to(device)


def rope_bf16(x, cos, sin):
    """Gemma2 apply_rotary_pos_emb in bf16 (what the QKV GEMM epilogue hands the kernels): x [B, L, H, D]."""
    c = torch.cat([cos, cos], -1)[None, :, None, :]
    s = torch.cat([sin, sin], -1)[None, :, None, :]
    h = x.shape[-1] // 2
    return (x * c) + (torch.cat([-x[..., h:], x[..., :h]], -1) * s)


def ref_attn(q, k, v, scale, cap, vis, cos=None, sin=None):
    """q [B, L, Hq, D], k / v [B, L, Hkv, D] (any float dtype, computed in float64) -> out [B, L, Hq, D] and
    lse [B, Hq, L], differentiable in q / k / v (the pre-rotation q / k when given the RoPE tables)."""
    B, L, Hq, D = q.shape
    Hkv = k.shape[2]
    q, k, v = (t.double().transpose(1, 2) for t in (q, k, v))
    if cos is not None:
        c, s = torch.cat([cos, cos], -1).double(), torch.cat([sin, sin], -1).double()
        rh = lambda t: torch.cat((-t[..., D // 2:], t[..., :D // 2]), -1)  # noqa: E731
        q, k = q * c + rh(q) * s, k * c + rh(k) * s
    k, v = k.repeat_interleave(Hq // Hkv, 1), v.repeat_interleave(Hq // Hkv, 1)
    s_ = q @ k.transpose(-1, -2) * scale
    if cap:
        s_ = cap * torch.tanh(s_ / cap)
    s_ = torch.where(vis[:, None], s_, s_ - s_.detach() + MIN)
    return (torch.softmax(s_, -1) @ v).transpose(1, 2), torch.logsumexp(s_, -1)


class Case:
    """One attention problem: data drawn on the CPU from a seeded generator (unit-variance q / k / v / dO), so the CPU
    and the GPU tests see the same numbers."""

    def __init__(self, D, Hq, Hkv, L, lay, window, rope=False, cap=50.0, B=2, seed=0):
        self.D, self.Hq, self.Hkv, self.L, self.lay, self.window = D, Hq, Hkv, L, lay, window
        self.rope, self.cap, self.B, self.seed = rope, cap, B, seed
        self.scale = 1 / 16 if D == 256 else D ** -0.5

    def __repr__(self):
        return (f"D{self.D}-H{self.Hq}x{self.Hkv}-L{self.L}-{self.lay}-w{self.window}-"
                f"{'rope' if self.rope else 'norope'}-cap{self.cap:g}")

    def data(self, device="cpu"):
        g = torch.Generator().manual_seed(1000 + self.seed)
        r = lambda H: torch.randn(self.B, self.L, H, self.D, generator=g).to(BF).to(device)  # noqa: E731
        d = dict(q=r(self.Hq), k=r(self.Hkv), v=r(self.Hkv), do=r(self.Hq), cls=layout(self.lay, self.B, self.L, device),
                 cos=None, sin=None)
        if self.rope:
            d["cos"], d["sin"] = rope_tables(self.L, self.D, device)
        return d

    def vis(self, d, mut=None):
        return visibility(d["cls"], self.B, self.L, self.window, mut, d["q"].device)

    def reference(self, d, mut=None, do=None):
        """out, lse, dq, dk, dv (float64) under the true mask or a mutant, for the upstream gradient do."""
        q, k, v = (d[n].double().requires_grad_(True) for n in "qkv")
        out, lse = ref_attn(q, k, v, self.scale, self.cap, self.vis(d, mut), d["cos"], d["sin"])
        out.backward((d["do"] if do is None else do).double())
        return dict(out=out.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def row_mask(rows, like):
    """[B, L] bool -> a factor broadcasting over [B, L, H, D]."""
    return rows[:, :, None, None].to(like.dtype)


def mutant_plan(case, d, ref=None):
    """For every mutation that changes the mask, where the case tells it from the truth by at least 3x the tolerance
    on out, dq, dk and dv: "global" (the whole tensors, upstream gradient dO), or "rows" (out on the query rows whose
    mask the mutation changes, and the gradients of dO zeroed outside those rows, as the fully masked rows are
    compared).  Returns {mut: (where, rows [B, L] bool or None, {quantity: distance})}; raises AssertionError when a
    mutant is told apart in neither way: the case then proves nothing about that edge and its layout must change."""
    ref = ref or case.reference(d)
    vt = case.vis(d)
    plan = {}
    for m in MUTANTS:
        vm = case.vis(d, m)
        if torch.equal(vm, vt):
            continue
        mu = case.reference(d, m)
        dist = {n: rel(mu[n], ref[n]) for n in QUANT}
        if all(dist[n] >= 3 * TOLS[n] for n in QUANT):
            plan[m] = ("global", None, dist)
            continue
        rows = (vm != vt).any(-1)
        do = d["do"] * row_mask(rows, d["do"])
        rt, rm = case.reference(d, None, do), case.reference(d, m, do)
        dist2 = {n: rel(rm[n], rt[n]) for n in ("dq", "dk", "dv")}
        dist2["out"] = rel(mu["out"][rows], ref["out"][rows])
        assert all(dist2[n] >= 3 * TOLS[n] for n in QUANT), (case, m, dist, dist2)
        plan[m] = ("rows", rows, dist2)
    return plan


def dead_rows(case, d):
    """[B, L] bool: the query rows with no visible key."""
    return ~case.vis(d).any(-1)


def dead_lse_cap(L):
    """lse the softcap path returns for a fully masked row: L keys at 2^-120 each."""
    return math.log(L) - 120 * math.log(2)


# ---------------------------------------------------------------------------------------------------- cases
def _A():
    """Case A: backward under a window at head_dim 256.  Every window value, every layout and both head kinds at
    least twice; w = 140 / 145 at L = 140 make the window ineffective (the kernels' window_free switch)."""
    C = Case
    return [
        C(256, 2, 1, 140, "mix", 1, rope=True), C(256, 3, 3, 140, "none", 1, cap=0.0),
        C(256, 8, 4, 140, "mix", 8, rope=True), C(256, 2, 1, 140, "few-prefix", 8, cap=0.0),
        C(256, 2, 1, 140, "mix", 48, rope=True), C(256, 3, 3, 140, "left-pad", 48), C(256, 8, 4, 140, "none", 48, cap=0.0),
        C(256, 3, 3, 140, "mix", 63), C(256, 2, 1, 140, "tile-dead", 63, rope=True, cap=0.0),
        C(256, 8, 4, 140, "mix", 64, rope=True), C(256, 2, 1, 140, "left-pad", 64, cap=0.0),
        C(256, 2, 1, 140, "tile-dead", 65), C(256, 3, 3, 140, "few-prefix", 65, rope=True),
        C(256, 2, 1, 140, "sparse", 139, rope=True), C(256, 3, 3, 140, "sparse", 139, cap=0.0),
        C(256, 8, 4, 140, "sparse", 140), C(256, 2, 1, 140, "sparse", 140, rope=True, cap=0.0),
        C(256, 2, 1, 140, "mix", 145, rope=True), C(256, 3, 3, 140, "few-prefix", 145, cap=0.0),
        C(256, 2, 1, 64, "mix", 16, rope=True), C(256, 3, 3, 65, "sparse", 64),
        C(256, 8, 4, 97, "left-pad", 33, rope=True, cap=0.0), C(256, 2, 1, 200, "tile-dead", 100, rope=True),
        C(256, 3, 3, 140, "few-prefix", 0, rope=True), C(256, 2, 1, 140, "none", 8, rope=True),
    ]


CASES_A = _A()
# Case C: head_dim 72 (SigLIP's kernels) with key classes and a window
CASES_C = [Case(72, 2, 2, L, lay, 48, cap=0.0) for L in (70, 256) for lay in ("mix", "left-pad")]
# Case B: fully masked rows (left padding), compared on their own
CASES_B = [Case(D, H, H // g, 140, "left-pad", 48, cap=cap, rope=(D == 256 and cap > 0))
           for D, H, g in ((256, 2, 2), (72, 2, 1)) for cap in (50.0, 0.0)]
# Case F: the autograd plug-in
CASES_F = [Case(256, 2, 1, 140, "mix", 48), Case(256, 2, 1, 140, "left-pad", 0, cap=0.0)]
# Case D: the stored-dS workspace; L % 64 in 1..32 (columns left unwritten) and above
CASES_D = [Case(256, 2, 1, L, "mix", 0 if L < 100 else 48, rope=(L % 2 == 0)) for L in (65, 70, 96, 140, 161)]
# Case E: distinct leading dimensions
CASES_E = [Case(256, 2, 1, 97, "mix", 33, rope=True), Case(72, 2, 2, 97, "mix", 33, cap=0.0)]
ALL_CASES = CASES_A + CASES_B + CASES_C + CASES_D + CASES_E + CASES_F


@functools.lru_cache(maxsize=None)
def _cached(idx, device):
    case = ALL_CASES[idx]
    d = case.data(device)
    ref = case.reference(d)
    return d, ref, mutant_plan(case, d, ref)


def prepared(case, device="cpu"):
    """(data, true reference, mutant plan) of a case, computed once per device and shared (never modified)."""
    return _cached(ALL_CASES.index(case), str(device))


# ------------------------------------------------------------------------------------------- model level
# The presets' sliding_window is 4096 with L <= 312, so the sliding layers' mask never bites; 16 does (layer 0 of the
# tiny config is a sliding layer, layer 1 a global one).
WINDOW16 = {"text_config": {"sliding_window": 16}}
MODEL_SEED = 7


def model_depth(batch=2):
    """A fixed depth map for both sides (the frozen depth estimator is not what these runs are about)."""
    return torch.rand(batch, 1, 224, 224, generator=torch.Generator().manual_seed(3)).mul(3).add(0.5)
