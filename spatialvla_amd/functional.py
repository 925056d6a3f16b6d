"""autograd Functions of the SpatialVLA hot path, each a thin shell over libsvla kernels.

Every Function documents the reference op(s) it replaces.  All tensors are bf16, 2-D row-major
[rows, features] on the GPU.  Weight gradients go either to freshly allocated tensors returned to
autograd (standard HF/torch semantics) or — when the training engine has attached a flat-buffer
view as `param._svla_grad` — straight into that view (accumulating when `param._svla_accum`),
in which case autograd receives None for that parameter (no extra copy, no autograd add).
"""
import math
import os
import weakref
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib as L
from . import kernels as K

BF16 = torch.bfloat16
F32 = torch.float32


# ------------------------------------------------------------------------------------ helpers
def _empty(*shape, dtype=BF16, like=None, device=None):
    return torch.empty(*shape, dtype=dtype, device=like.device if like is not None else device)


# Parameters whose gradients go to a TrainEngine's flat buffer, by (data_ptr, shape): a Function's saved weight can
# come back from ctx.saved_tensors as an alias without the Parameter's attributes -- torch.utils.checkpoint's
# recompute (gradient checkpointing) returns the recomputed saved tensors -- and its gradient must still land in the
# flat buffer, not in a fresh tensor autograd would put in .grad.
_FLAT_PARAMS: "weakref.WeakValueDictionary" = weakref.WeakValueDictionary()


def register_flat_param(p: torch.Tensor):
    _FLAT_PARAMS[(p.data_ptr(), tuple(p.shape))] = p


def _grad_dest(p: torch.Tensor, needed: bool):
    """(buffer, accumulate, value returned to autograd) for the gradient of parameter p."""
    if not needed:
        return None, False, None
    if not hasattr(p, "_svla_grad"):
        p = _FLAT_PARAMS.get((p.data_ptr(), tuple(p.shape)), p)
    g = getattr(p, "_svla_grad", None)
    if g is not None:
        return g, bool(getattr(p, "_svla_accum", False)), None
    buf = torch.empty_like(p)
    return buf, False, buf


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# Weight gradients on a side stream (SVLA_WGRAD_STREAM=0: all on the current stream).  A projection's weight-gradient
# GEMM reads only dY and X, so it can run beside the input-gradient GEMM and whatever follows that on the main stream
# (the attention backward, the GeGLU derivative pass).  The GEMMs run one workgroup per CU with a tile count that
# rarely divides 256 (o dgrad: 312 tiles, the last round fills 56 CUs), so the second kernel takes the CUs the first
# leaves idle.  Outputs are independent and every kernel's reduction order is fixed by its own tiling, so results are
# bitwise those of the serial order.
# When every weight gradient of a Function goes to the engine's flat buffer (nothing returned to autograd), the main
# stream does not wait for the side stream at the Function's end (SVLA_WGRAD_DEFER=0: it does): the side work keeps
# overlapping the next layers' backward.  The tensors it reads are marked with record_stream, so the caching allocator
# does not hand their memory out again before the side stream has read them, and the main stream waits for the side
# stream at the end of the backward pass (an autograd engine callback) and wherever the engine hands gradients to
# a collective (join_side_work, TrainEngine's bucket hooks).
WGRAD_STREAM = [os.environ.get("SVLA_WGRAD_STREAM", "1") != "0"]
# CUs the side-stream weight-gradient GEMMs leave to the main stream (their stream-K persistent grid is capped at
# num_cus - reserve, svla_gemm_set_cu_cap); 0 = they may take every CU.  Without it a persistent weight-gradient grid
# holds every CU until it is done and the main stream's next kernel (the norm-pair backward, 69 us alone) waits
# ~600 us for a CU (profiles/r7a_block_breakdown.txt).  8: step 216.4-216.8 -> 214.3-214.4 ms, block 4.65-4.67 ->
# 4.61 ms (16: the same within noise); 4: 214.1-214.3 (8) -> 212.4-212.8 ms, 2: 212.9-213.0 (profiles/
# r8q_side_cu_reserve_ab.txt); a CU reserve for the Zoe forward beside SigLIP (64, 128) measured no gain
SIDE_CU_RESERVE = [int(os.environ.get("SVLA_SIDE_CU_RESERVE", "4"))]
WGRAD_DEFER = [os.environ.get("SVLA_WGRAD_DEFER", "1") != "0"]
_side_streams: dict = {}
_join_queued: dict = {}  # device -> main stream the end-of-backward callback will make wait


def side_stream(device) -> "torch.cuda.Stream":
    """The per-device side stream (_SideWork's; the forward also runs the frozen Zoe estimator on it)."""
    s = _side_streams.get(device)
    if s is None:
        s = _side_streams[device] = torch.cuda.Stream(device)
    return s


def join_side_work():
    """Make the stream that queued side-stream weight gradients wait for all of them."""
    for dev, main in list(_join_queued.items()):
        main.wait_stream(_side_streams[dev])
        del _join_queued[dev]


_NUM_CUS: dict = {}


def _num_cus(device) -> int:
    n = _NUM_CUS.get(device)
    if n is None:
        n = _NUM_CUS[device] = torch.cuda.get_device_properties(device).multi_processor_count
    return n


class _SideWork:
    """run(fn, *reads): fn on the side stream, after everything issued on the main stream so far (reads: the tensors
    fn reads); join(*returned): the main stream waits for the side stream now, or -- when no returned gradient buffer
    is given and deferral is on -- at the end of the backward pass."""
    __slots__ = ("on", "main", "side", "reads")

    def __init__(self, like: torch.Tensor):
        self.on = WGRAD_STREAM[0] and like.is_cuda and not torch.cuda.is_current_stream_capturing()
        self.reads = []
        if self.on:
            dev = like.device
            self.main = torch.cuda.current_stream(dev)
            self.side = side_stream(dev)

    def run(self, fn, *reads):
        if not self.on:
            return fn()
        self.side.wait_stream(self.main)
        self.reads.extend(reads)
        res = SIDE_CU_RESERVE[0]
        with torch.cuda.stream(self.side):
            if res <= 0:
                return fn()
            lib = L.lib()
            lib.svla_gemm_set_cu_cap(max(1, _num_cus(self.side.device) - res))
            try:
                return fn()
            finally:
                lib.svla_gemm_set_cu_cap(0)

    def join(self, *returned):
        if not self.on:
            return
        if not WGRAD_DEFER[0] or any(r is not None for r in returned):
            self.main.wait_stream(self.side)
            return
        for t in self.reads:
            if t is not None:
                t.record_stream(self.side)
        dev = self.main.device
        if dev not in _join_queued:
            _join_queued[dev] = self.main
            torch.autograd.Variable._execution_engine.queue_callback(join_side_work)


class ResidualSlot:
    """Hand-off of a residual-stream gradient between the two consumers of one tensor: the residual branch
    (add + post-norm, or a GEMM epilogue's residual input) and the pre-norm that reads the same tensor.  The
    residual branch's backward always runs first (the pre-norm feeds it), so it parks its gradient here instead
    of returning it, and the pre-norm's backward adds it inside the norm-backward kernel (dres) -- the sum
    autograd would otherwise form with a separate elementwise add over the residual stream."""
    __slots__ = ("g",)

    def __init__(self):
        self.g = None

    def put(self, g):
        self.g = g

    def take(self):
        g, self.g = self.g, None
        return g


class MXSlot:
    """Hand-off of an activation's OCP MX e4m3 copy from the kernel that produced the bf16 tensor (a norm forward) to
    the fp8 projection that reads it (configs[4]): the producer writes both in one pass, the consumer takes the copy
    instead of quantising the tensor again.  `ptr` ties the copy to the bf16 tensor it was made from."""
    __slots__ = ("val", "ptr")

    def __init__(self):
        self.val, self.ptr = None, None

    def put(self, t, val):
        self.val, self.ptr = val, t.data_ptr()

    def take(self, t):
        """The copy of t if this slot holds one (else None); the slot is emptied either way."""
        v, p = self.val, self.ptr
        self.val, self.ptr = None, None
        return v if v is not None and p == t.data_ptr() else None


def mx_slot_for(f8, site) -> Optional[MXSlot]:
    """An MXSlot when projection `site` runs in fp8 with MX scales (producers then emit the copy), else None."""
    return MXSlot() if f8 is not None and site in FP8_SITES[0] and FP8_SCALING[0] == "mx" else None


# ------------------------------------------------------------------------------------ norms
class RMSNormFn(torch.autograd.Function):
    """Gemma2RMSNorm.forward (reference model/modeling_gemma2.py:69-74).  mx: an MXSlot that receives the MX e4m3
    copy of y, made by the same launch (the fp8 q|k|v operand)."""

    @staticmethod
    def forward(ctx, x, w, eps, slot=None, mx=None):
        x = _c(x)
        y = torch.empty_like(x)
        rstd = _empty(x.shape[0], dtype=F32, like=x)
        if mx is not None and x.shape[1] % 128 == 0:
            mx.put(y, K.rmsnorm_fwd_mx(x, w, eps, y, rstd))
        else:
            K.rmsnorm_fwd(x, w, eps, y, rstd)
        ctx.save_for_backward(x, w, rstd)
        ctx.slot = slot
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, rstd = ctx.saved_tensors
        dx = torch.empty_like(x)
        dw, acc, ret = _grad_dest(w, ctx.needs_input_grad[1])
        dres = ctx.slot.take() if ctx.slot is not None else None
        K.rmsnorm_bwd(x, w, rstd, _c(dy), None if dres is None else _c(dres), dx, dw, dw_accumulate=acc)
        return dx, ret, None, None, None


class AddRMSNormFn(torch.autograd.Function):
    """h = res + Gemma2RMSNorm(y)  (decoder-layer sandwich norm + residual, modeling_gemma2.py:489-496)."""

    @staticmethod
    def forward(ctx, res, y, w, eps, slot=None, mx_grad=None):
        res, y = _c(res), _c(y)
        h = torch.empty_like(y)
        rstd = _empty(y.shape[0], dtype=F32, like=y)
        K.add_rmsnorm_fwd(res, y, w, eps, h, rstd)
        ctx.save_for_backward(y, w, rstd)
        ctx.slot = slot
        ctx.mx_grad = mx_grad
        return h

    @staticmethod
    def backward(ctx, dh):
        y, w, rstd = ctx.saved_tensors
        dh = _c(dh)
        dy = torch.empty_like(y)
        dw, acc, ret = _grad_dest(w, ctx.needs_input_grad[2])
        N = y.shape[1]
        mx = ctx.mx_grad is not None and N % 128 == 0 and N > 1536
        dy_mx = K.rmsnorm_bwd(y, w, rstd, dh, None, dy, dw, dw_accumulate=acc, mx=mx)
        if dy_mx is not None:  # the MX copy of dy for the fp8 dgrad of the projection that produced y
            ctx.mx_grad.put(dy, dy_mx)
        if ctx.slot is not None:  # the pre-norm reading `res` adds dh in its backward kernel
            ctx.slot.put(dh)
            return None, dy, ret, None, None, None
        return dh, dy, ret, None, None, None


class AddRMSNorm2Fn(torch.autograd.Function):
    """(h, x) = (res + Gemma2RMSNorm_1(y), Gemma2RMSNorm_2(h)): the decoder layer's post-attention norm + residual
    and its pre-feedforward norm (modeling_gemma2.py:487-490) in one forward launch (svla_add_rmsnorm2_fwd_train,
    bitwise AddRMSNormFn then RMSNormFn).  Backward (one launch, svla_rmsnorm2_bwd): dh_total = rms_bwd_2(dx) + dh
    (dh: h's residual-branch gradient, from slot_h when its consumer parks it there), then dy = rms_bwd_1(dh_total);
    dh_total is the gradient of res (parked in slot_res for the pre-norm that also reads res, as AddRMSNormFn does)."""

    @staticmethod
    def forward(ctx, res, y, w1, w2, eps1, eps2, slot_res=None, slot_h=None, mx=None, mx_grad=None):
        res, y = _c(res), _c(y)
        h, x = torch.empty_like(y), torch.empty_like(y)
        r1 = _empty(y.shape[0], dtype=F32, like=y)
        r2 = _empty(y.shape[0], dtype=F32, like=y)
        if mx is not None and y.shape[1] % 128 == 0:  # + the MX copy of x (the fp8 gate|up operand)
            mx.put(x, K.add_rmsnorm2_fwd_train_mx(res, y, w1, w2, eps1, eps2, h, x, r1, r2))
        else:
            K.add_rmsnorm2_fwd_train(res, y, w1, w2, eps1, eps2, h, x, r1, r2)
        ctx.save_for_backward(y, h, w1, w2, r1, r2)
        ctx.slots = (slot_res, slot_h)
        ctx.mx_grad = mx_grad
        ctx.set_materialize_grads(False)  # h's residual gradient usually arrives through slot_h: no zero tensor
        return h, x

    @staticmethod
    def backward(ctx, dh, dx):
        y, h, w1, w2, r1, r2 = ctx.saved_tensors
        slot_res, slot_h = ctx.slots
        if slot_h is not None:
            parked = slot_h.take()
            if parked is not None:
                dh = parked if dh is None else dh + parked
        dw2, acc2, ret2 = _grad_dest(w2, ctx.needs_input_grad[3])
        dw1, acc1, ret1 = _grad_dest(w1, ctx.needs_input_grad[2])
        dht = torch.empty_like(h)
        dy = torch.empty_like(y)
        if dx is None:
            dx = torch.zeros_like(h)
        # both norms' backward in one pass (bitwise the two svla_rmsnorm_bwd calls)
        mx = ctx.mx_grad is not None and y.shape[1] % 128 == 0
        dy_mx = K.rmsnorm2_bwd(h, w2, r2, _c(dx), None if dh is None else _c(dh), y, w1, r1, dht, dy, dw2, dw1, acc2,
                               acc1, mx=mx)
        if dy_mx is not None:  # the MX copy of dy (the attention output's gradient) for the fp8 o dgrad
            ctx.mx_grad.put(dy, dy_mx)
        if slot_res is not None:
            slot_res.put(dht)
            return None, dy, ret1, ret2, None, None, None, None, None, None
        return dht, dy, ret1, ret2, None, None, None, None, None, None


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm (SigLIP layer_norm1/2/post_layernorm [3p]; Ego3D head.1, modeling_spatialvla.py:61)."""

    @staticmethod
    def forward(ctx, x, w, b, eps, slot=None):
        x = _c(x)
        y = torch.empty_like(x)
        mean = _empty(x.shape[0], dtype=F32, like=x)
        rstd = _empty(x.shape[0], dtype=F32, like=x)
        K.layernorm_fwd(x, w, b, eps, y, mean, rstd)
        ctx.save_for_backward(x, w, b, mean, rstd)
        ctx.slot = slot
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, mean, rstd = ctx.saved_tensors
        dx = torch.empty_like(x)
        dw, accw, retw = _grad_dest(w, ctx.needs_input_grad[1])
        db, accb, retb = _grad_dest(b, ctx.needs_input_grad[2])
        if dw is not None and db is not None and accw != accb:
            raise RuntimeError("LayerNorm weight/bias grads must share accumulate mode")
        dres = ctx.slot.take() if ctx.slot is not None else None
        K.layernorm_bwd(x, w, mean, rstd, _c(dy), None if dres is None else _c(dres), dx, dw, db, accumulate=accw)
        return dx, retw, retb, None, None


class ReLUFn(torch.autograd.Function):
    """nn.ReLU (Ego3D position_embedding_head.2, modeling_spatialvla.py:62)."""

    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        y = torch.empty_like(x)
        K.relu_fwd(x, y)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        K.relu_bwd(x, _c(dy), dx)
        return dx


# ------------------------------------------------------------------------------------ linear
def _cat_views(ts):
    """torch.cat of 1-D tensors that already sit back to back in one storage (the engine's flat buffer) as a
    view; otherwise a copy."""
    nxt, st = ts[0].data_ptr(), ts[0].untyped_storage().data_ptr()
    for t in ts:
        if t.dim() != 1 or not t.is_contiguous() or t.data_ptr() != nxt or t.untyped_storage().data_ptr() != st:
            return torch.cat(ts)
        nxt += t.numel() * t.element_size()
    return torch.as_strided(ts[0], (sum(t.numel() for t in ts),), (1,))


def _bias_grad(dy, b, needed):
    db, acc, ret = _grad_dest(b, needed)
    if db is not None:
        K.colsum_bf16(dy, db, accumulate=acc)
    return ret


class LinearFn(torch.autograd.Function):
    """y = bf16(bf16(x W^T + b) * post_scale) — nn.Linear (+ the projector's / sqrt(H),
    modeling_spatialvla.py:124,331-332).  With `res`, y = bf16(bf16(x W^T + b) + res): the residual add
    fused in the epilogue (SigLIP encoder residuals; Ego3D + vision features, modeling_spatialvla.py:328).
    K may be padded (`k_pad`): the weight is zero-padded per call (patchify, Ego3D 204-wide input)."""

    @staticmethod
    def forward(ctx, x, w, b, res, post_scale):
        x = _c(x)
        M = x.shape[0]
        N, Kw = w.shape
        wk = w
        if x.shape[1] != Kw:  # zero-padded reduction dim (ld must be a multiple of 8)
            wk = torch.zeros(N, x.shape[1], dtype=BF16, device=w.device)
            wk[:, :Kw] = w
        y = _empty(M, N, like=x)
        if res is not None:
            K.linear_fwd(x, [wk], y, kind=L.EPI_BIAS_RESID, bias=b, in0=_c(res))
        elif b is not None:
            K.linear_fwd(x, [wk], y, kind=L.EPI_BIAS, bias=b, alpha=post_scale)
        else:
            K.linear_fwd(x, [wk], y, kind=L.EPI_STORE, alpha=post_scale)
        ctx.save_for_backward(x, w, b)
        ctx.post_scale = post_scale
        ctx.has_res = res is not None
        ctx.wk = wk if wk is not w else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        dy = _c(dy)
        if ctx.post_scale != 1.0:
            # y = bf16(z * s): dz = bf16(dy * s) (autograd of the reference's division)
            dy = (dy * ctx.post_scale).to(BF16)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _empty(*x.shape, like=x)
            K.linear_dgrad(dy, [ctx.wk if ctx.wk is not None else w], dx)
        retw = None
        if ctx.needs_input_grad[1]:
            if x.shape[1] != w.shape[1]:
                tmp = _empty(w.shape[0], x.shape[1], like=x)
                K.linear_wgrad(dy, x, [tmp])
                dw, acc, retw = _grad_dest(w, True)
                if acc:
                    dw.add_(tmp[:, :w.shape[1]])
                else:
                    dw.copy_(tmp[:, :w.shape[1]])
            else:
                dw, acc, retw = _grad_dest(w, True)
                K.linear_wgrad(dy, x, [dw], accumulate=acc)
        retb = _bias_grad(dy, b, b is not None and ctx.needs_input_grad[2])
        dres = dy if ctx.has_res else None
        return dx, retw, retb, dres, None


# ------------------------------------------------------------------------------------ fp8 projections
# Bumped by TrainEngine.optimizer_step: AdamW rewrites the bf16 weights through the C-ABI, which torch's version
# counters do not see, so the fp8 weight copies compare this epoch as well.
WEIGHT_EPOCH = [0]
# fp8 projections: the input-gradient (dgrad) GEMMs run in e4m3 too (the weight-gradient GEMMs stay bf16)
FP8_DGRAD = [True]
# scaling of the fp8 operands: "mx" = OCP MX block scales (one E8M0 scale per 32 k, applied by the MFMA; the product
# path), "row" = one fp32 scale per row applied in the epilogue (round 2-4)
FP8_SCALING = [os.environ.get("SVLA_FP8_SCALING", "mx")]
# which Gemma2 projections run in fp8 when a layer has fp8 weights (configs[4]): any of "qkv", "o", "gate_up", "down"
# (SVLA_FP8_SITES, comma-separated); the others stay on the bf16 GEMM.  tests/test_fp8_ablation_gpu.py measures each
# site's share of the logit error and of the action-row flips.
FP8_SITES = [set(os.environ.get("SVLA_FP8_SITES", "qkv,o,gate_up,down").split(","))]


def _fp8_site(f8, name):
    """f8 if projection `name` runs in fp8 (FP8_SITES), else None (the bf16 GEMM)."""
    return f8 if f8 is not None and name in FP8_SITES[0] else None


class FP8Weights:
    """e4m3 copies of one Gemma2 layer's projection weights (BASELINE configs[4]): q|k|v [4096, H], o [H, 2048],
    gate|up [2I, H], down [H, I].  MX scaling: the forward copy W (MX blocks along the input dim K) and, for dgrad,
    W^T (blocks along the output dim N: the dgrad GEMM's reduction) each quantised from bf16 (svla_quant_mx_rows);
    row scaling: per-row fp32 scales, W^T the byte transpose of the forward copy.  Rebuilt lazily when a weight
    moved, was modified in place, or the optimizer stepped (WEIGHT_EPOCH).
    frozen: the weights are the frozen base of LoRA adapters (enable_fp8_lora), which no optimizer step rewrites, so
    the copies do not follow WEIGHT_EPOCH -- unless a weight sits in a TrainEngine's flat buffers (an engine built
    while it was trainable steps it still); a move or an in-place change rebuilds them as always, and merge_lora()
    drops the whole object."""

    def __init__(self, frozen: bool = False):
        self._key = None
        self.mats = {}
        self.frozen = frozen

    def _epoch(self, mats):
        if self.frozen and not any((m.data_ptr(), tuple(m.shape)) in _FLAT_PARAMS for m in mats):
            return -1
        return WEIGHT_EPOCH[0]

    @staticmethod
    def _rows(mats):
        mats = K._merge_rows(list(mats))
        return mats[0] if len(mats) == 1 else torch.cat(mats, 0)

    def _entry(self, name, mats):
        key = (self._epoch(mats), FP8_SCALING[0]) + tuple((m.data_ptr(), m._version) for m in mats)
        hit = self.mats.get(name)
        if hit is None or hit["key"] != key:
            w = self._rows(mats)
            if FP8_SCALING[0] == "mx" and w.shape[0] % 128 == 0 and w.shape[1] % 128 == 0:
                # both layouts from one read of the bf16 weight (the forward copy and the dgrad copy W^T)
                (q, s), (qt, st) = K.quant_mx_both(w)
                hit = self.mats[name] = {"key": key, "q": q, "s": s, "qt": qt, "st": st}
            else:
                q, s = K.quant_mx_rows(w) if FP8_SCALING[0] == "mx" else K.quant_fp8_rows(w)
                hit = self.mats[name] = {"key": key, "q": q, "s": s}
        return hit

    def get(self, name, mats):
        e = self._entry(name, mats)
        return e["q"], e["s"]

    def get_t(self, name, mats):
        """The dgrad operand: MX -- (e4m3 W^T [K, N], its MX scales); row -- (the byte transpose of the forward copy,
        the forward copy's row scales s [N])."""
        e = self._entry(name, mats)
        if "qt" not in e:
            if FP8_SCALING[0] == "mx":
                e["qt"], e["st"] = K.quant_mx_cols(self._rows(mats))  # W^T's rows, no transposed copy
            else:
                e["qt"], e["st"] = K.transpose_u8(e["q"]), e["s"]
        return e["qt"], e["st"]

    def ones(self, n, device):
        o = self.mats.get(("ones", n))
        if o is None:
            o = self.mats[("ones", n)] = torch.ones(n, dtype=torch.float32, device=device)
        return o


class FP8DecodeWeights:
    """Weight-only OCP MX e4m3 copies for the KV-cached decode step (enable_fp8_decode): of one Gemma2 layer's q|k|v
    [4096, H], o [H, 2048], gate|up [2I, H] and down [H, I], or of lm_head [V, H].  A copy is svla_quant_mx_rows(W) --
    the tested quantiser defines the numbers -- with the exponents repacked row-major (svla_mx_scales_rowmajor), the
    layout the GEMVs of csrc/fp8_decode.hip read.  Built lazily by the first fp8 decode step and rebuilt when a weight
    moved, was modified in place (tensor version), or the optimizer stepped (WEIGHT_EPOCH).  `builds` counts this
    holder's (re)builds: the captured decode graphs hold raw pointers into the copies, so the decode state compares the
    model's sum of them (SpatialVLAForConditionalGeneration._fp8_decode_key); BUILDS counts those of every holder
    (tests, tools).
    frozen: the weights are the frozen base of unmerged LoRA adapters (enable_fp8_lora_decode), which no optimizer step
    on A and B rewrites, so the copies do not follow WEIGHT_EPOCH (FP8Weights' rule: unless a weight sits in a
    TrainEngine's flat buffers); a move or an in-place change rebuilds them as always."""

    BUILDS = [0]

    def __init__(self, frozen: bool = False):
        self.mats = {}
        self.builds = 0
        self.frozen = frozen

    _epoch = FP8Weights._epoch

    def get(self, name, mats):
        """([q segments e4m3 [N_i, K]], [exponent segments uint8 [N_i, K/32]]) of cat(mats, 0): one segment, or for
        name == "gate_up" the gate rows and the up rows (the GEGLU pair)."""
        key = (self._epoch(mats),) + tuple((m.data_ptr(), m._version) for m in mats)
        hit = self.mats.get(name)
        if hit is None or hit["key"] != key:
            q, sc = K.quant_mx_rows(FP8Weights._rows(mats))
            s = K.mx_scales_rowmajor(sc)
            if name == "gate_up":
                I = mats[0].shape[0]
                qs, ss = [q[:I], q[I:]], [s[:I], s[I:]]
            else:
                qs, ss = [q], [s]
            hit = self.mats[name] = {"key": key, "q": qs, "s": ss}
            self.builds += 1
            FP8DecodeWeights.BUILDS[0] += 1
        return hit["q"], hit["s"]

    def nbytes(self) -> int:
        return sum(t.numel() for e in self.mats.values() for t in e["q"] + e["s"])


def fp8_decode_ok(M: int, k: int, weights, norm: bool = False) -> bool:
    """Whether a decode-step projection runs on its e4m3 copy: shapes svla_gemv_mxfp8 takes (else the bf16 path)."""
    return all(w.dim() == 2 and w.shape[1] == k for w in weights) and K.gemv_mxfp8_ok(M, k, norm)


def _fp8_linear(x, f8, name, mats, out, x_mx=None, **kw):
    """out = epi(x @ cat(mats)^T) with both operands quantised to e4m3 (x per call -- or x_mx, the MX copy x's
    producer already made -- weights cached)."""
    wq, ws = f8.get(name, mats)
    if FP8_SCALING[0] == "mx":
        xq, xs = x_mx if x_mx is not None else K.quant_mx_rows(x)
        K.gemm_mxfp8(xq, xs, wq, ws, out, **kw)
    else:
        xq, xs = K.quant_fp8_rows(x)
        K.gemm_fp8(xq, xs, wq, ws, out, **kw)


def _fp8_dgrad(dy, f8, name, mats, out, dy_mx=None):
    """out[M, K] = dy[M, N] @ cat(mats)[N, K] on the fp8 GEMM.  MX: dy quantised with blocks along N against the
    MX copy of W^T (dy_mx: that quantisation already made by dy's producer).  Row scaling: the forward's e4m3 weight
    W ~ diag(s_w) W_q reused transposed -- dy's columns are scaled by s_w before dy is quantised per row, so
    out = s_dy[m] * sum_n q_dy[m, n] W_q[n, k]."""
    wt, st = f8.get_t(name, mats)
    if FP8_SCALING[0] == "mx":
        dq, ds = dy_mx if dy_mx is not None else K.quant_mx_rows(dy)
        K.gemm_mxfp8(dq, ds, wt, st, out)
    else:
        dq, ds = K.quant_fp8_rows(dy, colscale=st)
        K.gemm_fp8(dq, ds, wt, f8.ones(wt.shape[0], dy.device), out)


# ------------------------------------------------------------------------------------ Gemma2 blocks
@dataclass
class GemmaAttnCfg:
    B: int
    L: int
    Hq: int
    Hkv: int
    D: int
    scale: float
    softcap: float
    window: int


class GemmaAttentionFn(torch.autograd.Function):
    """Gemma2Attention.forward (modeling_gemma2.py:364-413): q/k/v projections, rotary embedding
    (:95-154), eager prefix-LM GQA attention with logit softcap (:169-195), o_proj — as one fused
    QKV GEMM whose epilogue applies RoPE to q/k (bf16 rounding of the reference), one attention kernel,
    one O GEMM.  The saved qkv holds the rotated q/k; the attention backward returns dq/dk w.r.t. the
    pre-rotation q/k (RoPE transpose), which is what the projection backward needs."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv, wo, cos, sin, kv_class, cfg: GemmaAttnCfg, f8: Optional[FP8Weights] = None,
                capture: Optional[dict] = None, mx_in: Optional[MXSlot] = None, mx_dout: Optional[MXSlot] = None):
        x = _c(x)
        x_mx = mx_in.take(x) if mx_in is not None else None
        M, H = x.shape
        qd, kd = cfg.Hq * cfg.D, cfg.Hkv * cfg.D
        qkv = _empty(M, qd + 2 * kd, like=x)
        rope = (cos, sin, cos.shape[0], cfg.D, qd + kd)
        if _fp8_site(f8, "qkv") is not None:
            _fp8_linear(x, f8, "qkv", (wq, wk, wv), qkv, x_mx=x_mx, kind=L.EPI_ROPE, rope=rope)
        else:
            K.linear_fwd(x, [wq, wk, wv], qkv, kind=L.EPI_ROPE, rope=rope)
        attn = _empty(M, qd, like=x)
        lse = _empty(cfg.B, cfg.Hq, cfg.L, dtype=F32, like=x)
        a = K.attn_args(cfg.B, cfg.L, cfg.Hq, cfg.Hkv, cfg.D, qkv[:, :qd], qkv.stride(0), qkv[:, qd:qd + kd],
                        qkv.stride(0), qkv[:, qd + kd:], qkv.stride(0), cfg.scale, cfg.softcap, kv_class, cfg.window)
        K.attn_fwd(a, attn, lse)
        if capture is not None:  # output_attentions: the rotated q|k|v rows (no copy)
            capture["qkv"] = qkv
        out = _empty(M, wo.shape[0], like=x)
        if _fp8_site(f8, "o") is not None:
            _fp8_linear(attn, f8, "o", (wo,), out)
        else:
            K.linear_fwd(attn, [wo], out)
        ctx.save_for_backward(x, wq, wk, wv, wo, qkv, attn, lse, cos, sin, kv_class)
        ctx.cfg = cfg
        ctx.f8 = f8
        ctx.mx_dout = mx_dout
        return out

    @staticmethod
    def backward(ctx, dout):
        x, wq, wk, wv, wo, qkv, attn, lse, cos, sin, kv_class = ctx.saved_tensors
        cfg = ctx.cfg
        if cos.shape[0] != cfg.L:  # Gemma2Attention.forward refuses this case up front (check_rope_for_grad)
            raise NotImplementedError("GemmaAttentionFn.backward: per-sequence RoPE tables (the backward's RoPE "
                                      "transpose reads table row = position in the sequence)")
        dout = _c(dout)
        M = x.shape[0]
        qd, kd = cfg.Hq * cfg.D, cfg.Hkv * cfg.D
        dattn = _empty(M, qd, like=x)
        f8 = ctx.f8 if FP8_DGRAD[0] else None
        # each weight gradient is queued on the side stream before the main-stream work it may overlap
        side = _SideWork(x)
        dwo, acc, ret_wo = _grad_dest(wo, ctx.needs_input_grad[4])
        if dwo is not None:
            side.run(lambda: K.linear_wgrad(dout, attn, [dwo], accumulate=acc), dout, attn)
        if _fp8_site(f8, "o") is not None:
            _fp8_dgrad(dout, f8, "o", (wo,), dattn, dy_mx=ctx.mx_dout.take(dout) if ctx.mx_dout is not None else None)
        else:
            K.linear_dgrad(dout, [wo], dattn)
        dqkv = torch.empty_like(qkv)
        a = K.attn_args(cfg.B, cfg.L, cfg.Hq, cfg.Hkv, cfg.D, qkv[:, :qd], qkv.stride(0), qkv[:, qd:qd + kd],
                        qkv.stride(0), qkv[:, qd + kd:], qkv.stride(0), cfg.scale, cfg.softcap, kv_class, cfg.window,
                        cos, sin)
        ld = dqkv.stride(0)
        K.attn_bwd(a, attn, dattn, lse, dqkv[:, :qd], ld, dqkv[:, qd:qd + kd], ld, dqkv[:, qd + kd:], ld)
        dx = None
        dests = [_grad_dest(w, ctx.needs_input_grad[1 + i]) for i, w in enumerate((wq, wk, wv))]

        def qkv_wgrad():
            if all(d[0] is not None for d in dests) and len({d[1] for d in dests}) == 1:
                K.linear_wgrad(dqkv, x, [d[0] for d in dests], accumulate=dests[0][1])
            else:
                off = 0
                for (dw, acc_i, _), w in zip(dests, (wq, wk, wv)):
                    n = w.shape[0]
                    if dw is not None:
                        K.linear_wgrad(_c(dqkv[:, off:off + n]), x, [dw], accumulate=acc_i)
                    off += n
        side.run(qkv_wgrad, dqkv, x)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if _fp8_site(f8, "qkv") is not None:
                _fp8_dgrad(dqkv, f8, "qkv", (wq, wk, wv), dx)
            else:
                K.linear_dgrad(dqkv, [wq, wk, wv], dx)
        rets = [d[2] for d in dests]
        side.join(*rets, ret_wo)
        return (dx, *rets, ret_wo, None, None, None, None, None, None, None, None)


@torch.no_grad()
def gemma_attention_weights(qkv, kv_class, cfg: GemmaAttnCfg) -> torch.Tensor:
    """output_attentions of the reference eager attention (modeling_gemma2.py:169-195): softmax probabilities
    [B, Hq, L, L] in bf16, from the rotated q / k rows the fused projection wrote.  The attention OUTPUT always comes
    from the HIP kernel, which never materialises these L x L maps; this is an introspection path (torch ops, the
    reference's op order and bf16 roundings: bf16 scores * scale, bf16 softcap, + additive mask, fp32 softmax)."""
    B, L, Hq, Hkv, D = cfg.B, cfg.L, cfg.Hq, cfg.Hkv, cfg.D
    qd, kd = Hq * D, Hkv * D
    q = qkv[:, :qd].reshape(B, L, Hq, D).transpose(1, 2)
    k = qkv[:, qd:qd + kd].reshape(B, L, Hkv, D).transpose(1, 2)
    k = k.repeat_interleave(Hq // Hkv, dim=1)                                   # repeat_kv (:157-166)
    w = torch.matmul(q, k.transpose(2, 3)) * cfg.scale
    if cfg.softcap:
        w = torch.tanh(w / cfg.softcap) * cfg.softcap
    mn = torch.finfo(w.dtype).min
    i = torch.arange(L, device=qkv.device)
    cls = (kv_class if kv_class is not None else torch.zeros(B, L, dtype=torch.uint8, device=qkv.device))[:, :L]
    vis = (cls[:, None, :] == 0) | ((cls[:, None, :] == 1) & (i[None, :, None] >= i[None, None, :]))
    if cfg.window:  # sliding layers (:461-473): keys at distance >= window are masked
        vis = vis & ((i[:, None] - i[None, :]) < cfg.window)[None]
    w = w + torch.where(vis, 0.0, mn).to(w.dtype)[:, None]
    return torch.softmax(w, dim=-1, dtype=torch.float32).to(qkv.dtype)


# decode steps run RoPE + cache append + attention as one launch (svla_attn_decode_rope); False = the two-launch
# form (svla_qkv_rope_append, then svla_attn_decode), kept for the bitwise A/B test
DECODE_FUSED = [os.environ.get("SVLA_DECODE_FUSED", "1") != "0"]


# decode steps fold the two norms between sublayers into the next projection's prologue (svla_gemv_rmsnorm2)
DECODE_NORM_FUSED = [os.environ.get("SVLA_DECODE_NORM_FUSED", "1") != "0"]


# decode steps with unmerged LoRA adapters run each projection as svla_lora_gemv_down + svla_lora_gemv (9 launches per
# layer); SVLA_LORA_DECODE_KERNELS=0 (and M > 8, or a shape those kernels refuse): the composition from the training
# path's kernels (norm pair, then projection + lora_down + lora_up per projection: 15 launches) -- the A/B partner, the
# second reference of the tests and the general fallback
LORA_DECODE_KERNELS = [os.environ.get("SVLA_LORA_DECODE_KERNELS", "1") != "0"]
# ... and, under enable_lora_decode(emb_head=True), embed the step's token with svla_lora_embed_decode and run the head
# as svla_lora_gemv_down + svla_lora_head_gemv; SVLA_LORA_DECODE_EMB_HEAD_KERNELS=0 keeps the layers' GEMVs and takes
# EmbedMergeLoRAFn / LMHeadCEFn at the two ends (tools/decode_bench.py times the two ends on their own with it)
LORA_DECODE_EMB_HEAD_KERNELS = [os.environ.get("SVLA_LORA_DECODE_EMB_HEAD_KERNELS", "1") != "0"]


def decode_proj_ok(form: str, M: int, k: int, weights, norm: bool = False, geglu: bool = False) -> bool:
    """Whether a decode step's projection of M rows over `weights` [N_i, k] runs on the kernel of `form` (decode_proj's
    rules 2 and 4; False: the next rule down).  norm: the norm pair runs in the prologue; geglu: a gate|up pair.
    "lora": the adapter GEMV pair (SVLA_LORA_DECODE_KERNELS, shapes svla_lora_gemv_down / svla_lora_gemv take).
    "fp8": svla_gemv_mxfp8 on the e4m3 copy (fp8_decode_ok; the GeGLU pair splits the copy into two equal halves).
    "lora_fp8": the adapter pair's projection half on the e4m3 copy (svla_lora_gemv_mxfp8, which has no prologue),
    else svla_lora_gemv on the bf16 weights."""
    sizes = [w.shape[0] for w in weights]
    if form == "lora":
        return (LORA_DECODE_KERNELS[0] and all(w.stride(1) == 1 for w in weights)
                and K.lora_gemv_ok(M, k, sizes, norm))
    halves = not geglu or sizes[0] == sizes[1]
    if form == "lora_fp8":
        return fp8_decode_ok(M, k, weights) and K.lora_gemv_mxfp8_ok(M, k, sizes) and halves
    return fp8_decode_ok(M, k, weights, norm=norm) and halves


def _adapters(lora, lo, hi):
    """Projections lo..hi-1 of lora = (r, scaling, (A, B) per projection) as decode_proj takes them, or None."""
    return None if lora is None else (lora[0], lora[1], [A for A, _ in lora[2 + lo:2 + hi]],
                                      [B for _, B in lora[2 + lo:2 + hi]])


def decode_proj(x, weights, out, geglu_out=None, lora=None, f8d=None, site=None, batched=False, decode=True):
    """out = x @ cat(weights)^T for one projection of a KV-cached step, on the first of these that applies:
      1. batched: svla_gemm_skinny.
      2. adapters, a decode step, decode_proj_ok("lora"): svla_lora_gemv_down (norm pair in its prologue), then
         svla_lora_gemv_mxfp8 on f8d.get(site, weights) if a holder is given and decode_proj_ok("lora_fp8"), else
         svla_lora_gemv.
      3. adapters otherwise: the composition (add_rmsnorm2_fwd, then _lora_ops().down, linear_fwd, .up).
      4. a holder, a decode step, decode_proj_ok("fp8"): svla_gemv_mxfp8 (norm pair in its prologue).
      5. a norm prologue: svla_gemv_rmsnorm2.
      6. linear_fwd.
    x: the input rows, or pre = (res, y, w1, w2, eps1, eps2, h_out) when the norm pair rms(res + rms(y; w1); w2) is
    formed in the prologue.  geglu_out = (g, u): weights is a gate|up pair and out its GeGLU.  lora = (r, scaling, As,
    Bs); f8d: an FP8DecodeWeights and the `site` its copy is kept under ("qkv", "o", "gate_up", "down"); decode: p0 > 0.
    Returns the x the adapter rules worked on (under pre they store it), else None."""
    pre = x if isinstance(x, tuple) else None
    like = pre[1] if pre is not None else x
    M, k = like.shape
    norm, geglu = pre is not None, geglu_out is not None
    if batched:
        K.gemm_skinny(x, weights, out)
    elif lora is not None:
        r, s, As, Bs = lora
        if decode and decode_proj_ok("lora", M, k, weights, norm):
            t = _empty(M, len(As) * K.lora_R(r), like=like)
            if norm:  # the norm pair in the prologue of the rank-r GEMV, which also stores x for the projection
                x = _empty(M, k, like=like)
            K.lora_gemv_down(x, As, r, t, norm=pre)
            if f8d is not None and decode_proj_ok("lora_fp8", M, k, weights, geglu=geglu):
                K.lora_gemv_mxfp8(x, *f8d.get(site, weights), t, Bs, r, s, out, geglu_out=geglu_out)
            else:
                K.lora_gemv(x, weights, t, Bs, r, s, out, geglu_out=geglu_out)
        else:
            if geglu:
                raise ValueError("decode_proj: the composed adapter form has no GeGLU (GemmaMLPLoRAFn runs that MLP)")
            ops = _lora_ops()
            if norm:
                x = _empty(M, k, like=like)
                K.add_rmsnorm2_fwd(*pre, x)
            t = ops.down(x, As, r)
            K.linear_fwd(x, weights, out)
            ops.up(out, t, Bs, r, s)
        return x
    elif f8d is not None and decode and decode_proj_ok("fp8", M, k, weights, norm, geglu):
        K.gemv_mxfp8(None if norm else x, *f8d.get(site, weights), out, geglu_out=geglu_out, norm=pre)
    elif norm:
        K.gemv_rmsnorm2(*pre, weights, out, geglu_out=geglu_out)
    else:
        K.linear_fwd(x, weights, out)
    return None


# Batched decode (enable_batched_decode): the window of new token rows B * Lq of a KV-cached step whose q|k|v and o
# projections run on svla_gemm_skinny.  Below it the GEMVs run (<= 8 rows); 64 is the kernel's limit.  The same-process
# A/B at 4B (tools/decode_bench.py --batched, profiles/batched_decode_ab.txt) has the switch ahead by more than the
# rounds' spread at 16, 32, 48 and 64 rows, one point per count of 16-row tiles, so the whole range is routed.
BATCHED_DECODE_MIN_ROWS = 9
BATCHED_DECODE_MAX_ROWS = 64


def batched_decode_ok(enabled: bool, rows: int, seen_tokens: int, grad_enabled: bool, bf16: bool = True,
                      adapters: bool = False, fp8_decode: bool = False, fp8_projections: bool = False,
                      widths=()) -> bool:
    """Whether a KV-cached step takes the batched decode path (q|k|v and o on svla_gemm_skinny), and the one place
    that states its exclusions: the switch is on, the step is a decode step (seen_tokens > 0) without grad, it adds
    BATCHED_DECODE_MIN_ROWS..BATCHED_DECODE_MAX_ROWS token rows, the base weights are bf16, no adapters are attached
    and no fp8 switch (enable_fp8_decode, enable_fp8_lora_decode, enable_fp8_projections) is on; `widths`: the
    reduction widths of the two projections, each a multiple of 32.  Everything else keeps the path it had.  Pure
    Python: nothing here touches a device."""
    return bool(enabled and seen_tokens > 0 and not grad_enabled
                and BATCHED_DECODE_MIN_ROWS <= rows <= BATCHED_DECODE_MAX_ROWS
                and bf16 and not adapters and not fp8_decode and not fp8_projections
                and all(k >= 32 and k % 32 == 0 for k in widths))


@torch.no_grad()
def gemma_attention_cached(x, wq, wk, wv, wo, cos, sin, k_cache, v_cache, kv_class, p0, cfg: GemmaAttnCfg,
                           pre=None, skip_o=False, lora=None, f8d=None, batched=False):
    """Gemma2Attention.forward with a KV cache (modeling_gemma2.py:364-413, cache update :387-395), inference
    only.  x holds the cfg.L new tokens of each of the cfg.B sequences, at absolute positions p0 .. p0+L-1;
    their rotated k and v are written into rows p0.. of k_cache/v_cache ([B, capacity, Hkv*D]).  The prefill
    (p0 == 0) runs the flash kernel of the uncached forward over the prompt, so it is bit-identical to it;
    later steps run the decode kernel over the first p0+L cache rows.  pre = (res, y, w1, w2, eps1, eps2, h_out): a
    decode step whose input x = rms(res + rms(y; w1); w2) is formed inside the q|k|v GEMV (h_out the new residual).
    lora = (r, scaling, (Aq, Bq), (Ak, Bk), (Av, Bv), (Ao, Bo)): unmerged adapters on the four projections; their
    prefill is the uncached adapter forward's kernels (GemmaAttentionLoRAFn) with the RoPE + cache fill launch.
    f8d: the layer's FP8DecodeWeights (enable_fp8_decode; with lora: enable_fp8_lora_decode), read by decode steps
    only.  batched (enable_batched_decode, batched_decode_ok): never with pre, lora or f8d.
    decode_proj states which kernel runs q|k|v and o under each of these."""
    if batched and (p0 == 0 or pre is not None or lora is not None or f8d is not None):
        raise ValueError("gemma_attention_cached: batched is a plain bf16 decode step (p0 > 0, no pre / lora / f8d)")
    if pre is not None:
        if p0 == 0:
            raise ValueError("gemma_attention_cached: the fused norm prologue is a decode-step path (p0 > 0)")
        like = pre[1]
    else:
        x = like = _c(x)
    M = like.shape[0]
    B, Lq = cfg.B, cfg.L
    qd, kd = cfg.Hq * cfg.D, cfg.Hkv * cfg.D
    qkv = _empty(M, qd + 2 * kd, like=like)
    attn = _empty(M, qd, like=like)
    # the prefill's RoPE in the q|k|v GEMM's epilogue (the base path with SVLA_PREFILL_ROPE_FILL=0; the adapter term
    # is added after the projection, so the adapter prefill always rotates afterwards)
    rope_epilogue = p0 == 0 and lora is None and not PREFILL_ROPE_FILL[0]
    if rope_epilogue:
        K.linear_fwd(x, [wq, wk, wv], qkv, kind=L.EPI_ROPE, rope=(cos, sin, cos.shape[0], cfg.D, qd + kd))
    else:
        # the RoPE / cache kernels read table row b*Lq+t (per-sequence positions): a shared table is repeated
        if cos.shape[0] != B * Lq:
            cos, sin = cos.repeat(B, 1), sin.repeat(B, 1)
        decode_proj(pre if pre is not None else x, [wq, wk, wv], qkv, lora=_adapters(lora, 0, 3), f8d=f8d, site="qkv",
                    batched=batched, decode=p0 > 0)
    if p0 > 0:
        _decode_attention(qkv, attn, cos, sin, k_cache, v_cache, kv_class, p0, cfg)
    else:
        _prefill_attention(qkv, attn, cos, sin, k_cache, v_cache, kv_class, cfg, rotated=rope_epilogue)
    # with adapters the o projection stays its own GEMV pair (skip_o / DECODE_O_FUSED do not apply): its adapter term
    # needs T complete before the projection starts, which inside one launch would take a grid barrier
    if skip_o and lora is None:  # the caller runs the o projection (gemma_mlp_decode with o=(attn, wo))
        return attn
    out = _empty(M, wo.shape[0], like=like)
    decode_proj(attn, [wo], out, lora=_adapters(lora, 3, 4), f8d=f8d, site="o", batched=batched, decode=p0 > 0)
    return out


def _decode_attention(qkv, attn, cos, sin, k_cache, v_cache, kv_class, p0, cfg):
    """A decode step's attention over the projected rows: one launch rotates q / k, appends k / v to the cache at
    rows p0.. and attends (DECODE_FUSED), or the two-launch form."""
    Lq = cfg.L
    if DECODE_FUSED[0]:
        K.attn_decode_rope(qkv, Lq, cos, sin, k_cache, v_cache, p0 + Lq, cfg.Hq, cfg.Hkv, cfg.D, cfg.scale,
                           cfg.softcap, kv_class, cfg.window, attn)
    else:
        K.qkv_rope_append(qkv, cfg.B, Lq, cfg.Hq, cfg.Hkv, cfg.D, cos, sin, k_cache, v_cache, p0)
        K.attn_decode(qkv[:, :cfg.Hq * cfg.D], Lq, k_cache, v_cache, p0 + Lq, cfg.Hq, cfg.Hkv, cfg.D, cfg.scale,
                      cfg.softcap, kv_class, cfg.window, attn)


def _prefill_attention(qkv, attn, cos, sin, k_cache, v_cache, kv_class, cfg, rotated):
    """The prefill's RoPE, cache fill and flash attention over the projected rows.  One launch rotates q and k in
    place and fills cache rows 0.. with k and v (svla_qkv_rope_fill: the ROPE epilogue's rounding, bitwise); rotated:
    the projection's epilogue did the RoPE, two copies fill the cache."""
    B, Lq = cfg.B, cfg.L
    qd, kd = cfg.Hq * cfg.D, cfg.Hkv * cfg.D
    if rotated:
        k_cache[:, :Lq].copy_(qkv[:, qd:qd + kd].view(B, Lq, kd))
        v_cache[:, :Lq].copy_(qkv[:, qd + kd:].view(B, Lq, kd))
    else:
        K.qkv_rope_append(qkv, B, Lq, cfg.Hq, cfg.Hkv, cfg.D, cos, sin, k_cache, v_cache, 0, k_back=True)
    lse = _empty(B, cfg.Hq, Lq, dtype=F32, like=qkv)
    cls = kv_class[:, :Lq].contiguous()  # held until the launch: attn_args keeps only its pointer
    a = K.attn_args(B, Lq, cfg.Hq, cfg.Hkv, cfg.D, qkv[:, :qd], qkv.stride(0), qkv[:, qd:qd + kd],
                    qkv.stride(0), qkv[:, qd + kd:], qkv.stride(0), cfg.scale, cfg.softcap, cls, cfg.window)
    K.attn_fwd(a, attn, lse)


# the prefill's q|k|v: plain GEMM + svla_qkv_rope_fill (one launch: RoPE of q and k, cache rows of k and v) instead
# of the RoPE epilogue + two cache copies; SVLA_PREFILL_ROPE_FILL=0: the latter
PREFILL_ROPE_FILL = [os.environ.get("SVLA_PREFILL_ROPE_FILL", "1") != "0"]


# ... with the o projection inside the same launch (a second grid barrier) instead of its own GEMV: opt-in, measured
# slower (1.97 vs 1.84 ms per token: 2304 rows over 2048 waves leave one row in flight a wave; profiles/r7b_*)
DECODE_O_FUSED = [os.environ.get("SVLA_DECODE_O_FUSED", "0") != "0"]


def persist_ok(y, wg, wu, wd) -> bool:
    return (DECODE_MLP_PERSIST[0] and y.shape[1] <= 2560 and wg.shape[0] <= 10240 and y.shape[0] <= 8
            and wg.stride(1) == wu.stride(1) == wd.stride(1) == 1
            and K.decode_mlp_grid(y.shape[0], y.shape[1], wg.shape[0]) > 0)


# the decode MLP as one persistent launch (svla_decode_mlp) instead of the norm-GEMV + down-GEMV pair: 1.80 vs
# 1.95 ms per decode token (profiles/r6z_decode_mlp_persist_ab.txt); SVLA_DECODE_MLP_PERSIST=0: the pair
DECODE_MLP_PERSIST = [os.environ.get("SVLA_DECODE_MLP_PERSIST", "1") != "0"]


@torch.no_grad()
def gemma_mlp_decode(res, y, w1, w2, eps1, eps2, h_out, wg, wu, wd, o=None, lora=None, f8d=None):
    """Decode-step Gemma2 MLP (modeling_gemma2.py:91-92) whose input is the post-attention + pre-feedforward norm pair
    (:487-490), formed inside the gate|up GEMV: h_out = res + rms(y; w1) (the residual stream), returns
    down(gelu_tanh(gate x) * up x) with x = rms(h_out; w2).
    lora = (r, scaling, (Ag, Bg), (Au, Bu), (Ad, Bd)): unmerged adapters on the three projections.
    f8d: the layer's FP8DecodeWeights (enable_fp8_decode): the two-launch form on the e4m3 copies -- the norm-prologue
    gate|up GeGLU GEMV, then the (split-K) down GEMV, both svla_gemv_mxfp8; not combined with `o`.  With `lora`
    (enable_fp8_lora_decode) the adapter form keeps its four launches and svla_lora_gemv_mxfp8 streams the e4m3 copies
    of gate|up and down."""
    I = wg.shape[0]

    def both(form):  # a joint choice: gate|up and down both run on the form's kernels, or the form is not taken
        return (decode_proj_ok(form, y.shape[0], y.shape[1], [wg, wu], norm=True, geglu=True)
                and decode_proj_ok(form, y.shape[0], I, [wd]))

    if lora is not None:
        # With adapters neither the persistent svla_decode_mlp nor DECODE_O_FUSED is used: each adapter term needs T
        # (a reduction over the whole input row) complete between the rank-r GEMV and the projection that adds it,
        # which inside the persistent launch would mean a second grid barrier per projection; a launch boundary is
        # the cheaper barrier (the persistent kernel's one barrier already costs what it saves on the o projection).
        if o is not None:
            raise ValueError("gemma_mlp_decode: the o projection inside the MLP launch is not built with adapters")
        if not both("lora"):  # the norm pair, then the uncached adapter forward's kernels
            r, s, (Ag, Bg), (Au, Bu), (Ad, Bd) = lora
            x = torch.empty_like(y)
            K.add_rmsnorm2_fwd(res, y, w1, w2, eps1, eps2, h_out, x)
            return GemmaMLPLoRAFn.apply(x, wg, wu, wd, s, r, Ag, Bg, Au, Bu, Ad, Bd)
    elif f8d is None or o is not None or not both("fp8"):
        f8d = None  # the bf16 forms: the persistent launch (with or without o), else the pair below
        if o is not None:  # y = attn @ wo^T (the o projection), in the persistent launch or as its own GEMV
            attn, wo = o
            y = _empty(attn.shape[0], wo.shape[0], like=attn)
            if (not persist_ok(y, wg, wu, wd) or attn.shape[1] > 2048 or wo.stride(1) != 1
                    or y.shape[1] > 8 * K.decode_mlp_grid(y.shape[0], y.shape[1], wg.shape[0])):
                decode_proj(attn, [wo], y)
                o = None
        if persist_ok(y, wg, wu, wd):
            out = _empty(y.shape[0], wd.shape[0], like=y)
            hact = _empty(y.shape[0], I, like=y)
            K.decode_mlp(res, y, w1, w2, eps1, eps2, h_out, wg, wu, wd, hact, out, o=o)  # one launch, bitwise
            return out
    # two projections: the norm-prologue gate|up GeGLU, then down -- adapter GEMV pairs (four launches), svla_gemv_mxfp8
    # on the e4m3 copies, or svla_gemv_rmsnorm2 + the bf16 GEMV
    M = y.shape[0]
    hact, g, u = (_empty(M, I, like=y) for _ in range(3))
    decode_proj((res, y, w1, w2, eps1, eps2, h_out), [wg, wu], hact, geglu_out=(g, u), lora=_adapters(lora, 0, 2),
                f8d=f8d, site="gate_up")
    out = _empty(M, wd.shape[0], like=y)
    decode_proj(hact, [wd], out, lora=_adapters(lora, 2, 3), f8d=f8d, site="down")
    return out


class GemmaMLPFn(torch.autograd.Function):
    """Gemma2MLP.forward (modeling_gemma2.py:91-92): down(gelu_tanh(gate x) * up x) — gate/up as one
    GEMM with the GeGLU in its epilogue; backward: dH GEMM, then the GeGLU derivative in one elementwise pass."""

    @staticmethod
    def forward(ctx, x, wg, wu, wd, f8: Optional[FP8Weights] = None, mx_in: Optional[MXSlot] = None,
                mx_dout: Optional[MXSlot] = None):
        x = _c(x)
        x_mx = mx_in.take(x) if mx_in is not None else None
        M = x.shape[0]
        I = wg.shape[0]
        h = _empty(M, I, like=x)
        g = _empty(M, I, like=x)
        u = _empty(M, I, like=x)
        out = _empty(M, wd.shape[0], like=x)
        h_mx = None
        if _fp8_site(f8, "gate_up") is not None:
            kw = {}
            if _fp8_site(f8, "down") is not None and FP8_SCALING[0] == "mx" and I % 128 == 0:
                # the GeGLU epilogue also writes the MX copy of h, the fp8 down operand (no quantisation pass)
                h_mx = (torch.empty(M, I, dtype=torch.float8_e4m3fn, device=x.device), K.MXScales(M, I, x.device))
                kw["mx_out"] = h_mx
            _fp8_linear(x, f8, "gate_up", (wg, wu), h, x_mx=x_mx, kind=L.EPI_GEGLU, geglu_I=I, out1=g, out2=u, **kw)
        else:
            K.linear_geglu_fwd(x, wg, wu, h, g, u)
        if _fp8_site(f8, "down") is not None:
            _fp8_linear(h, f8, "down", (wd,), out, x_mx=h_mx)
        else:
            K.linear_fwd(h, [wd], out)
        ctx.save_for_backward(x, wg, wu, wd, g, u, h)
        ctx.f8 = f8
        ctx.mx_dout = mx_dout
        return out

    @staticmethod
    def backward(ctx, dout):
        x, wg, wu, wd, g, u, h = ctx.saved_tensors
        dout = _c(dout)
        M, I = g.shape
        side = _SideWork(x)
        dwd, acc, ret_wd = _grad_dest(wd, ctx.needs_input_grad[3])
        if dwd is not None:
            side.run(lambda: K.linear_wgrad(dout, h, [dwd], accumulate=acc), dout, h)
        dgu = _empty(M, 2 * I, like=x)
        f8 = ctx.f8 if FP8_DGRAD[0] else None
        # dH by a plain-store GEMM, then the GeGLU derivative as one HBM pass in place (in the down dgrad's epilogue
        # it cost more than the pass: +60 % on the 8-phase kernel's LDS image, +0.11 ms per layer from the 4-wave
        # kernel's accumulators with the g / u loads one row block ahead, r4)
        if _fp8_site(f8, "down") is not None:
            _fp8_dgrad(dout, f8, "down", (wd,), dgu[:, :I],
                       dy_mx=ctx.mx_dout.take(dout) if ctx.mx_dout is not None else None)
        else:
            K.linear_dgrad(dout, [wd], dgu[:, :I])
        f8gu = _fp8_site(f8, "gate_up")
        dgu_mx = None
        if f8gu is not None and FP8_SCALING[0] == "mx" and I % 128 == 0 and ctx.needs_input_grad[0]:
            # the MX copy of [dg | du] for the fp8 dgrad comes out of the same pass (no quantisation pass over dgu)
            dgu_mx = K.geglu_bwd_mx(dgu[:, :I], g, u, dgu[:, :I], dgu[:, I:])
        else:
            K.geglu_bwd(dgu[:, :I], g, u, dgu[:, :I], dgu[:, I:])
        dg_, accg, retg = _grad_dest(wg, ctx.needs_input_grad[1])
        du_, accu, retu = _grad_dest(wu, ctx.needs_input_grad[2])

        def gate_up_wgrad():
            if dg_ is not None and du_ is not None and accg == accu:
                K.linear_wgrad(dgu, x, [dg_, du_], accumulate=accg)
            else:
                if dg_ is not None:
                    K.linear_wgrad(_c(dgu[:, :I]), x, [dg_], accumulate=accg)
                if du_ is not None:
                    K.linear_wgrad(_c(dgu[:, I:]), x, [du_], accumulate=accu)
        side.run(gate_up_wgrad, dgu, x)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if f8gu is not None:
                _fp8_dgrad(dgu, f8, "gate_up", (wg, wu), dx, dy_mx=dgu_mx)
            else:
                K.linear_dgrad(dgu, [wg, wu], dx)
        side.join(retg, retu, ret_wd)
        return dx, retg, retu, ret_wd, None, None, None


# ------------------------------------------------------------------------------------ Gemma2 blocks with LoRA adapters
# The rank-r products of the adapters on the kernels of csrc/lora.hip (SVLA_LORA_KERNELS=0: the same Functions run
# them as an unfused composition of svla_gemm_bf16 calls and torch elementwise ops -- the A/B partner and a second
# reference in the tests).
LORA_KERNELS = [os.environ.get("SVLA_LORA_KERNELS", "1") != "0"]
# the adapter gradients (svla_lora_wgrad) on the side stream beside the input-gradient chain, as the base weight
# gradients of the full fine-tune are (_SideWork; results are bitwise the serial order's).  B = 32 4B LoRA step, r = 32,
# three alternating rounds: 219.4-220.0 ms on the main stream, 212.3-212.8 ms on the side stream
# (profiles/lora_step.txt); SVLA_LORA_WGRAD_STREAM=0 keeps them on the main stream
LORA_WGRAD_STREAM = [os.environ.get("SVLA_LORA_WGRAD_STREAM", "1") != "0"]


def _rope_torch(c, rope):
    """In-place rotate_half RoPE of the composition path, the rounding points of SVLA_EPI_ROPE."""
    cos, sin, Lr, D, cols = rope
    M = c.shape[0]
    pos = torch.arange(M, device=c.device) % Lr
    cs, sn = cos[pos][:, None, :D // 2], sin[pos][:, None, :D // 2]
    x = c[:, :cols].reshape(M, cols // D, D)
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    lo = x1 * cs + (-x2) * sn  # bf16 tensors: every product and the sum round to bf16
    hi = x2 * cs + x1 * sn
    c[:, :cols] = torch.cat([lo, hi], -1).reshape(M, cols)


class _LoraKernelOps:
    """The adapter products on svla_lora_down / svla_lora_up / svla_lora_wgrad."""

    # Two products of a single adapter go to the library's bf16 GEMM instead (a documented choice between two HIP
    # kernels, DESIGN.md section 4 "LoRA"): t = x A^T with one segment (o: 21.5 us vs 24.5 us on svla_lora_down, down
    # K = 9216: 70 vs 87 us) and dA = dt^T x with one segment and >= 8192 columns (down: 85 vs 121 us on
    # svla_lora_wgrad; at 2048 columns the rank-r kernel wins, 46 vs 146 us).  With q|k|v or gate|up sharing the
    # large matrix the rank-r kernels read it once and win everywhere (profiles/lora_kernels_ab.txt).
    WGRAD_GEMM_MIN_COLS = 8192

    @staticmethod
    def down(x, As, r):
        R = K.lora_R(r)
        if len(As) == 1:
            t = _empty(x.shape[0], R, like=x) if r == R else torch.zeros(x.shape[0], R, dtype=BF16, device=x.device)
            K.linear_fwd(x, [As[0]], t[:, :r])
            return t
        t = _empty(x.shape[0], len(As) * R, like=x)
        K.lora_down(x, As, r, t)
        return t

    @staticmethod
    def up(c, t, Bs, r, s, rope=None, geglu_h=None, mx_out=None, gelu_out=None, resid=None, post_scale=None):
        if gelu_out is not None and not LORA_GELU_FUSED[0]:  # plain adapter add, then the GELU as its own pass
            K.lora_up(c, t, Bs, r, alpha=s)
            K.gelu_rows(K.GELU_TANH, c, gelu_out)
            return
        K.lora_up(c, t, Bs, r, alpha=s, rope=rope, geglu_h=geglu_h, mx_out=mx_out, gelu_out=gelu_out, resid=resid,
                  post_scale=post_scale)

    @staticmethod
    def down_t(dy, Bs, r, s):
        dt = _empty(dy.shape[0], len(Bs) * K.lora_R(r), like=dy)
        K.lora_down(dy, Bs, r, dt, sliced=True, alpha=s)
        return dt

    @staticmethod
    def up_t(dx, dt, As, r):
        K.lora_up(dx, dt, As, r, summed=True)

    @staticmethod
    def wgrad(y, t, dests, r, sliced, alpha, starts):
        R = K.lora_R(r)
        if (not sliced and len(dests) == 1 and dests[0][0] is not None and alpha == 1.0
                and y.shape[1] >= _LoraKernelOps.WGRAD_GEMM_MIN_COLS):
            K.linear_wgrad(_c(t[:, :r]), y, [dests[0][0]], accumulate=dests[0][1])
            return
        if all(d[0] is not None for d in dests) and len({d[1] for d in dests}) == 1:
            K.lora_wgrad(y, t, [d[0] for d in dests], r, sliced=sliced, alpha=alpha, accumulate=dests[0][1])
            return
        for i, (g, acc, _) in enumerate(dests):
            if g is not None:
                ys = y[:, starts[i]:starts[i + 1]] if sliced else y
                K.lora_wgrad(ys, t[:, i * R:(i + 1) * R], [g], r, sliced=sliced, alpha=alpha, accumulate=acc)


class _LoraComposedOps:
    """The same products as an unfused composition: svla_gemm_bf16 wrappers plus torch elementwise ops."""

    @staticmethod
    def down(x, As, r):
        R = K.lora_R(r)
        t = torch.zeros(x.shape[0], len(As) * R, dtype=BF16, device=x.device)
        for i, a in enumerate(As):
            K.linear_fwd(x, [a], t[:, i * R:i * R + r])
        return t

    @staticmethod
    def up(c, t, Bs, r, s, rope=None, geglu_h=None, mx_out=None, gelu_out=None, resid=None, post_scale=None):
        R = K.lora_R(r)
        off = 0
        for i, b in enumerate(Bs):
            u = _empty(c.shape[0], b.shape[0], like=c)
            K.linear_fwd(t[:, i * R:i * R + r], [b], u, alpha=s)
            c[:, off:off + b.shape[0]] += u
            off += b.shape[0]
        if rope is not None:
            _rope_torch(c, rope)
        if geglu_h is not None:
            I = c.shape[1] // 2
            torch.mul(torch.nn.functional.gelu(c[:, :I], approximate="tanh"), c[:, I:], out=geglu_h)
            if mx_out is not None:
                K.quant_mx_rows(geglu_h, *mx_out)
        if gelu_out is not None:
            gelu_out.copy_(torch.nn.functional.gelu(c, approximate="tanh"))
        if resid is not None:
            c += resid
        if post_scale is not None:
            c *= post_scale

    @staticmethod
    def down_t(dy, Bs, r, s):
        R = K.lora_R(r)
        dt = torch.zeros(dy.shape[0], len(Bs) * R, dtype=BF16, device=dy.device)
        off = 0
        for i, b in enumerate(Bs):
            K.linear_dgrad(dy[:, off:off + b.shape[0]], [b], dt[:, i * R:i * R + r])
            off += b.shape[0]
        if s != 1.0:
            dt *= s
        return dt

    @staticmethod
    def up_t(dx, dt, As, r):
        R = K.lora_R(r)
        for i, a in enumerate(As):
            K.linear_dgrad(dt[:, i * R:i * R + r], [a], dx, accumulate=True)

    @staticmethod
    def wgrad(y, t, dests, r, sliced, alpha, starts):
        R = K.lora_R(r)
        for i, (g, acc, _) in enumerate(dests):
            if g is None:
                continue
            tmp = torch.empty_like(g)
            ti = _c(t[:, i * R:i * R + r])
            if sliced:   # dB_i [N_i, r] = alpha y_i^T t_i
                K.linear_wgrad(_c(y[:, starts[i]:starts[i + 1]]), ti, [tmp])
            else:        # dA_i [r, W] = alpha t_i^T y
                K.linear_wgrad(ti, y, [tmp])
            if alpha != 1.0:
                tmp *= alpha
            if acc:
                g += tmp
            else:
                g.copy_(tmp)


def _lora_ops():
    return _LoraKernelOps if LORA_KERNELS[0] else _LoraComposedOps


def _lora_grads(ops, dy, t, x, r, s, Bs, As, needs):
    """dt = s dy B (returned), and the adapter gradients dB = s dy^T t, dA = dt^T x written to their destinations;
    returns (dt, [values for autograd: dA_0, dB_0, dA_1, dB_1, ...])."""
    sizes = [b.shape[0] for b in Bs]
    starts = [0]
    for n in sizes:
        starts.append(starts[-1] + n)
    dt = ops.down_t(dy, Bs, r, s)
    dB = [_grad_dest(b, needs[2 * i + 1]) for i, b in enumerate(Bs)]
    dA = [_grad_dest(a, needs[2 * i]) for i, a in enumerate(As)]
    rets = []
    for a, b in zip(dA, dB):
        rets += [a[2], b[2]]

    def wgrads():
        ops.wgrad(dy, t, dB, r, True, s, starts)
        ops.wgrad(x, dt, dA, r, False, 1.0, starts)
    if LORA_WGRAD_STREAM[0]:
        side = _SideWork(x)
        side.run(wgrads, dy, t, x, dt)
        side.join(*rets)
    else:
        wgrads()
    return dt, rets


def _frozen(ctx, idx, what):
    if any(ctx.needs_input_grad[i] for i in idx):
        raise RuntimeError(f"{what}: the base weights of a LoRA-adapted projection must be frozen "
                           "(requires_grad=False); no base weight gradient is computed")


class GemmaAttentionLoRAFn(torch.autograd.Function):
    """GemmaAttentionFn with a LoRA adapter on each of q, k, v, o (reference train/spatialvla_finetune.py:262-300,
    peft Linear.forward: base(x) + lora_B(lora_A(x)) * scaling): the base q|k|v GEMM stores plainly, one rank-r pass
    adds s t B^T and applies RoPE in place; the backward computes the adapter and input gradients only (frozen base).
    f8 (enable_fp8_lora): the base forward and input-gradient GEMMs of the sites in FP8_SITES run in e4m3 as in
    GemmaAttentionFn (mx_in / mx_dout: the MX copies of x and dout from the norms); the rank-r products, the
    attention and the adapter gradients read the bf16 tensors."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv, wo, cos, sin, kv_class, cfg: GemmaAttnCfg, scaling: float, r: int,
                Aq, Bq, Ak, Bk, Av, Bv, Ao, Bo, f8: Optional[FP8Weights] = None, mx_in: Optional[MXSlot] = None,
                mx_dout: Optional[MXSlot] = None):
        _frozen(ctx, (1, 2, 3, 4), "GemmaAttentionLoRAFn")
        ops = _lora_ops()
        x = _c(x)
        x_mx = mx_in.take(x) if mx_in is not None else None
        M = x.shape[0]
        qd, kd = cfg.Hq * cfg.D, cfg.Hkv * cfg.D
        t = ops.down(x, [Aq, Ak, Av], r)
        qkv = _empty(M, qd + 2 * kd, like=x)
        if _fp8_site(f8, "qkv") is not None:
            _fp8_linear(x, f8, "qkv", (wq, wk, wv), qkv, x_mx=x_mx)
        else:
            K.linear_fwd(x, [wq, wk, wv], qkv)
        ops.up(qkv, t, [Bq, Bk, Bv], r, scaling, rope=(cos, sin, cos.shape[0], cfg.D, qd + kd))
        attn = _empty(M, qd, like=x)
        lse = _empty(cfg.B, cfg.Hq, cfg.L, dtype=F32, like=x)
        a = K.attn_args(cfg.B, cfg.L, cfg.Hq, cfg.Hkv, cfg.D, qkv[:, :qd], qkv.stride(0), qkv[:, qd:qd + kd],
                        qkv.stride(0), qkv[:, qd + kd:], qkv.stride(0), cfg.scale, cfg.softcap, kv_class, cfg.window)
        K.attn_fwd(a, attn, lse)
        t_o = ops.down(attn, [Ao], r)
        out = _empty(M, wo.shape[0], like=x)
        if _fp8_site(f8, "o") is not None:
            _fp8_linear(attn, f8, "o", (wo,), out)
        else:
            K.linear_fwd(attn, [wo], out)
        ops.up(out, t_o, [Bo], r, scaling)
        ctx.save_for_backward(x, wq, wk, wv, wo, qkv, attn, lse, cos, sin, kv_class, t, t_o,
                              Aq, Bq, Ak, Bk, Av, Bv, Ao, Bo)
        ctx.cfg, ctx.scaling, ctx.r = cfg, scaling, r
        ctx.f8, ctx.mx_dout = f8, mx_dout
        return out

    @staticmethod
    def backward(ctx, dout):
        (x, wq, wk, wv, wo, qkv, attn, lse, cos, sin, kv_class, t, t_o,
         Aq, Bq, Ak, Bk, Av, Bv, Ao, Bo) = ctx.saved_tensors
        cfg, s, r = ctx.cfg, ctx.scaling, ctx.r
        if cos.shape[0] != cfg.L:
            raise NotImplementedError("GemmaAttentionLoRAFn.backward: per-sequence RoPE tables")
        ops = _lora_ops()
        dout = _c(dout)
        M = x.shape[0]
        qd, kd = cfg.Hq * cfg.D, cfg.Hkv * cfg.D
        nig = ctx.needs_input_grad
        dt_o, g_o = _lora_grads(ops, dout, t_o, attn, r, s, [Bo], [Ao], nig[17:19])
        dattn = _empty(M, qd, like=x)
        f8 = ctx.f8 if FP8_DGRAD[0] else None
        if _fp8_site(f8, "o") is not None:
            _fp8_dgrad(dout, f8, "o", (wo,), dattn, dy_mx=ctx.mx_dout.take(dout) if ctx.mx_dout is not None else None)
        else:
            K.linear_dgrad(dout, [wo], dattn)
        ops.up_t(dattn, dt_o, [Ao], r)
        dqkv = torch.empty_like(qkv)
        a = K.attn_args(cfg.B, cfg.L, cfg.Hq, cfg.Hkv, cfg.D, qkv[:, :qd], qkv.stride(0), qkv[:, qd:qd + kd],
                        qkv.stride(0), qkv[:, qd + kd:], qkv.stride(0), cfg.scale, cfg.softcap, kv_class, cfg.window,
                        cos, sin)
        ld = dqkv.stride(0)
        K.attn_bwd(a, attn, dattn, lse, dqkv[:, :qd], ld, dqkv[:, qd:qd + kd], ld, dqkv[:, qd + kd:], ld)
        dt, g_qkv = _lora_grads(ops, dqkv, t, x, r, s, [Bq, Bk, Bv], [Aq, Ak, Av], nig[11:17])
        dx = None
        if nig[0]:
            dx = torch.empty_like(x)
            if _fp8_site(f8, "qkv") is not None:
                _fp8_dgrad(dqkv, f8, "qkv", (wq, wk, wv), dx)
            else:
                K.linear_dgrad(dqkv, [wq, wk, wv], dx)
            ops.up_t(dx, dt, [Aq, Ak, Av], r)
        return (dx, None, None, None, None, None, None, None, None, None, None, *g_qkv, *g_o, None, None, None)


class GemmaMLPLoRAFn(torch.autograd.Function):
    """GemmaMLPFn with a LoRA adapter on each of gate, up, down (reference train/spatialvla_finetune.py:262-300): the
    base gate|up GEMM stores g | u plainly into one [M, 2I] buffer, one rank-r pass adds the adapters and writes
    h = gelu_tanh(g) u; the down adapter's gradient contribution enters dH before the GeGLU derivative pass.
    f8 (enable_fp8_lora): as GemmaAttentionLoRAFn; the rank-r GeGLU pass also writes the MX copy of h, the fp8 down
    operand (svla_lora_epilogue.mx_q), and svla_geglu_bwd_mx that of [dg | du]."""

    @staticmethod
    def forward(ctx, x, wg, wu, wd, scaling: float, r: int, Ag, Bg, Au, Bu, Ad, Bd, f8: Optional[FP8Weights] = None,
                mx_in: Optional[MXSlot] = None, mx_dout: Optional[MXSlot] = None):
        _frozen(ctx, (1, 2, 3), "GemmaMLPLoRAFn")
        ops = _lora_ops()
        x = _c(x)
        x_mx = mx_in.take(x) if mx_in is not None else None
        M = x.shape[0]
        I = wg.shape[0]
        t = ops.down(x, [Ag, Au], r)
        gu = _empty(M, 2 * I, like=x)
        if _fp8_site(f8, "gate_up") is not None:
            _fp8_linear(x, f8, "gate_up", (wg, wu), gu, x_mx=x_mx)
        else:
            K.linear_fwd(x, [wg, wu], gu)
        h = _empty(M, I, like=x)
        h_mx = None
        if _fp8_site(f8, "down") is not None and FP8_SCALING[0] == "mx" and I % 128 == 0:
            h_mx = (torch.empty(M, I, dtype=torch.float8_e4m3fn, device=x.device), K.MXScales(M, I, x.device))
        ops.up(gu, t, [Bg, Bu], r, scaling, geglu_h=h, mx_out=h_mx)
        t_d = ops.down(h, [Ad], r)
        out = _empty(M, wd.shape[0], like=x)
        if _fp8_site(f8, "down") is not None:
            _fp8_linear(h, f8, "down", (wd,), out, x_mx=h_mx)
        else:
            K.linear_fwd(h, [wd], out)
        ops.up(out, t_d, [Bd], r, scaling)
        ctx.save_for_backward(x, wg, wu, wd, gu, h, t, t_d, Ag, Bg, Au, Bu, Ad, Bd)
        ctx.scaling, ctx.r = scaling, r
        ctx.f8, ctx.mx_dout = f8, mx_dout
        return out

    @staticmethod
    def backward(ctx, dout):
        x, wg, wu, wd, gu, h, t, t_d, Ag, Bg, Au, Bu, Ad, Bd = ctx.saved_tensors
        s, r = ctx.scaling, ctx.r
        ops = _lora_ops()
        dout = _c(dout)
        M = x.shape[0]
        I = wg.shape[0]
        nig = ctx.needs_input_grad
        dt_d, g_d = _lora_grads(ops, dout, t_d, h, r, s, [Bd], [Ad], nig[10:12])
        dgu = _empty(M, 2 * I, like=x)
        f8 = ctx.f8 if FP8_DGRAD[0] else None
        if _fp8_site(f8, "down") is not None:
            _fp8_dgrad(dout, f8, "down", (wd,), dgu[:, :I],
                       dy_mx=ctx.mx_dout.take(dout) if ctx.mx_dout is not None else None)
        else:
            K.linear_dgrad(dout, [wd], dgu[:, :I])
        ops.up_t(dgu[:, :I], dt_d, [Ad], r)
        f8gu = _fp8_site(f8, "gate_up")
        dgu_mx = None
        if f8gu is not None and FP8_SCALING[0] == "mx" and I % 128 == 0 and nig[0]:
            dgu_mx = K.geglu_bwd_mx(dgu[:, :I], gu[:, :I], gu[:, I:], dgu[:, :I], dgu[:, I:])
        else:
            K.geglu_bwd(dgu[:, :I], gu[:, :I], gu[:, I:], dgu[:, :I], dgu[:, I:])
        dt, g_gu = _lora_grads(ops, dgu, t, x, r, s, [Bg, Bu], [Ag, Au], nig[6:10])
        dx = None
        if nig[0]:
            dx = torch.empty_like(x)
            if f8gu is not None:
                _fp8_dgrad(dgu, f8, "gate_up", (wg, wu), dx, dy_mx=dgu_mx)
            else:
                K.linear_dgrad(dgu, [wg, wu], dx)
            ops.up_t(dx, dt, [Ag, Au], r)
        return (dx, None, None, None, None, None, *g_gu, *g_d, None, None, None)


# ------------------------------------------------------------------------------------ SigLIP blocks
@dataclass
class SiglipAttnCfg:
    B: int
    L: int
    H: int
    D: int
    scale: float


class SiglipAttentionFn(torch.autograd.Function):
    """SiglipAttention.forward + encoder residual (transformers siglip [3p], called from
    modeling_spatialvla.py:310): q/k/v (bias) as one GEMM, bidirectional softmax attention
    (head_dim 72), out_proj with bias and the residual add fused in its epilogue."""

    @staticmethod
    def forward(ctx, x, res, wq, bq, wk, bk, wv, bv, wo, bo, cfg: SiglipAttnCfg, slot=None):
        ctx.slot = slot
        x, res = _c(x), _c(res)
        M, Hd = x.shape
        bqkv = _cat_views([bq, bk, bv])
        qkv = _empty(M, 3 * Hd, like=x)
        K.linear_fwd(x, [wq, wk, wv], qkv, kind=L.EPI_BIAS, bias=bqkv)
        attn = _empty(M, Hd, like=x)
        lse = _empty(cfg.B, cfg.H, cfg.L, dtype=F32, like=x)
        a = K.attn_args(cfg.B, cfg.L, cfg.H, cfg.H, cfg.D, qkv[:, :Hd], qkv.stride(0), qkv[:, Hd:2 * Hd],
                        qkv.stride(0), qkv[:, 2 * Hd:], qkv.stride(0), cfg.scale)
        K.attn_fwd(a, attn, lse)
        out = _empty(M, Hd, like=x)
        K.linear_fwd(attn, [wo], out, kind=L.EPI_BIAS_RESID, bias=bo, in0=res)
        ctx.save_for_backward(x, wq, bq, wk, bk, wv, bv, wo, bo, qkv, attn, lse)
        ctx.cfg = cfg
        return out

    @staticmethod
    def backward(ctx, dout):
        x, wq, bq, wk, bk, wv, bv, wo, bo, qkv, attn, lse = ctx.saved_tensors
        cfg = ctx.cfg
        dout = _c(dout)
        M, Hd = x.shape
        nig = ctx.needs_input_grad
        dattn = torch.empty_like(attn)
        # weight and bias gradients on the side stream (_SideWork), each queued before the main-stream work it may
        # overlap; every gradient buffer is allocated here, on the main stream
        side = _SideWork(x)
        dwo, acc, ret_wo = _grad_dest(wo, nig[8])
        dbo, accbo, ret_bo = _grad_dest(bo, nig[9])

        def o_grads():
            if dwo is not None:
                K.linear_wgrad(dout, attn, [dwo], accumulate=acc)
            if dbo is not None:
                K.colsum_bf16(dout, dbo, accumulate=accbo)
        side.run(o_grads, dout, attn)
        K.linear_dgrad(dout, [wo], dattn)
        dqkv = torch.empty_like(qkv)
        a = K.attn_args(cfg.B, cfg.L, cfg.H, cfg.H, cfg.D, qkv[:, :Hd], qkv.stride(0), qkv[:, Hd:2 * Hd],
                        qkv.stride(0), qkv[:, 2 * Hd:], qkv.stride(0), cfg.scale)
        ld = dqkv.stride(0)
        K.attn_bwd(a, attn, dattn, lse, dqkv[:, :Hd], ld, dqkv[:, Hd:2 * Hd], ld, dqkv[:, 2 * Hd:], ld)
        rets = []
        dws = [_grad_dest(w, nig[2 + 2 * i]) for i, w in enumerate((wq, wk, wv))]
        bds = [_grad_dest(b, nig[3 + 2 * i]) for i, b in enumerate((bq, bk, bv))]
        cat = None
        if all(d[0] is not None for d in bds) and len({d[1] for d in bds}) == 1:
            cat = _cat_views([d[0] for d in bds])
            if cat.data_ptr() != bds[0][0].data_ptr():  # not back to back (no engine flat buffer): a copy, unusable
                cat = None

        def qkv_grads():
            if all(d[0] is not None for d in dws) and len({d[1] for d in dws}) == 1:
                # q, k and v weight gradients in one GEMM (C row segments): three 1152x1152 wgrads launched
                # separately filled ~20 of the 256 CUs each
                K.linear_wgrad(dqkv, x, [d[0] for d in dws], accumulate=dws[0][1])
            else:
                for i, (dw, accw, _r) in enumerate(dws):
                    if dw is not None:
                        K.linear_wgrad(_c(dqkv[:, i * Hd:(i + 1) * Hd]), x, [dw], accumulate=accw)
            if cat is not None:  # the q|k|v bias gradients in one column sum over dqkv (engine: adjacent in the flat grad)
                K.colsum_bf16(dqkv, cat, accumulate=bds[0][1])
            else:
                for i, (db, accb, _r) in enumerate(bds):
                    if db is not None:
                        K.colsum_bf16(dqkv[:, i * Hd:(i + 1) * Hd], db, accumulate=accb)  # strided view, no copy
        side.run(qkv_grads, dqkv, x)
        dx = torch.empty_like(x) if nig[0] else None
        if dx is not None:
            K.linear_dgrad(dqkv, [wq, wk, wv], dx)
        for i in range(3):
            rets += [dws[i][2], bds[i][2]]
        side.join(*rets, ret_wo, ret_bo)
        dres = dout
        if ctx.slot is not None:  # handed to layer_norm1's backward (ResidualSlot)
            ctx.slot.put(dout)
            dres = None
        return (dx, dres, *rets, ret_wo, ret_bo, None, None)


# SigLIP fc1 / BEiT fc1: bias GEMM + GELU pass (svla_gelu_rows) instead of the VALU-heavy GELU GEMM epilogues, which
# ran slower inside the tile loop (profiles/r3l_epi_ab.txt); bitwise the same values (test_gelu_rows_matches_epilogues)
GELU_PASS = [os.environ.get("SVLA_GELU_PASS", "1") != "0"]


class SiglipMLPFn(torch.autograd.Function):
    """SiglipMLP + residual: res + fc2(gelu_tanh(fc1 x)) (transformers siglip [3p]); fc1 bias+GELU and
    fc2 bias+residual fused in GEMM epilogues, GELU derivative fused into the fc2 dgrad epilogue."""

    @staticmethod
    def forward(ctx, x, res, w1, b1, w2, b2, slot=None):
        ctx.slot = slot
        x, res = _c(x), _c(res)
        M = x.shape[0]
        I = w1.shape[0]
        pre = _empty(M, I, like=x)
        act = _empty(M, I, like=x)
        if GELU_PASS[0]:  # bias GEMM (the 4-wave kernel's direct epilogue), then the GELU as an HBM pass
            K.linear_fwd(x, [w1], pre, kind=L.EPI_BIAS, bias=b1)
            K.gelu_rows(K.GELU_TANH, pre, act)
        else:
            K.linear_fwd(x, [w1], act, kind=L.EPI_BIAS_GELU, bias=b1, out1=pre)
        out = _empty(M, w2.shape[0], like=x)
        K.linear_fwd(act, [w2], out, kind=L.EPI_BIAS_RESID, bias=b2, in0=res)
        ctx.save_for_backward(x, w1, b1, w2, b2, pre, act)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w1, b1, w2, b2, pre, act = ctx.saved_tensors
        dout = _c(dout)
        nig = ctx.needs_input_grad
        side = _SideWork(x)  # weight / bias gradients beside the input-gradient chain (as SiglipAttentionFn)
        dw2, acc2, ret_w2 = _grad_dest(w2, nig[4])
        db2, accb2, ret_b2 = _grad_dest(b2, nig[5])

        def fc2_grads():
            if dw2 is not None:
                K.linear_wgrad(dout, act, [dw2], accumulate=acc2)
            if db2 is not None:
                K.colsum_bf16(dout, db2, accumulate=accb2)
        side.run(fc2_grads, dout, act)
        dpre = torch.empty_like(pre)
        if GELU_PASS[0]:
            K.linear_dgrad(dout, [w2], dpre)
            K.gelu_rows(K.GELU_TANH_BWD, dpre, dpre, pre=pre)
        else:
            K.linear_dgrad(dout, [w2], dpre, kind=L.EPI_GELU_BWD, in0=pre)
        dw1, acc1, ret_w1 = _grad_dest(w1, nig[2])
        db1, accb1, ret_b1 = _grad_dest(b1, nig[3])

        def fc1_grads():
            if dw1 is not None:
                K.linear_wgrad(dpre, x, [dw1], accumulate=acc1)
            if db1 is not None:
                K.colsum_bf16(dpre, db1, accumulate=accb1)
        side.run(fc1_grads, dpre, x)
        dx = torch.empty_like(x) if nig[0] else None
        if dx is not None:
            K.linear_dgrad(dpre, [w1], dx)
        side.join(ret_w1, ret_b1, ret_w2, ret_b2)
        dres = dout
        if ctx.slot is not None:  # handed to layer_norm2's backward (ResidualSlot)
            ctx.slot.put(dout)
            dres = None
        return dx, dres, ret_w1, ret_b1, ret_w2, ret_b2, None


# ------------------------------------------------------------------------------------ vision-side blocks with LoRA adapters
# The reference's default lora_target="linear" (train/spatialvla_finetune.py:264-270) also wraps the SigLIP q/k/v/
# out_proj/fc1/fc2, the projector and both Ego3D linears.  Each base GEMM keeps its bias store (SVLA_EPI_BIAS), one
# rank-r pass adds the adapter term and applies what the base epilogue would have applied after it (GELU, residual,
# post-scale: svla_lora_up's GELU / RESID / SCALE); peft's bias="none" freezes weights and biases, so the backward
# computes the adapter and input gradients only.  SVLA_LORA_KERNELS=0 runs the same Functions on the composition.
# SVLA_LORA_GELU_FUSED=0: fc1's adapter add stores plainly and svla_gelu_rows makes the activation (two passes).
LORA_GELU_FUSED = [os.environ.get("SVLA_LORA_GELU_FUSED", "1") != "0"]


class SiglipAttentionLoRAFn(torch.autograd.Function):
    """SiglipAttentionFn with a LoRA adapter on each of q, k, v, out_proj: q|k|v share one t (three segments of H
    columns, plain adapter add after the bias GEMM), out_proj's rank-r pass adds the encoder residual (RESID)."""

    @staticmethod
    def forward(ctx, x, res, wq, bq, wk, bk, wv, bv, wo, bo, cfg: SiglipAttnCfg, scaling: float, r: int,
                Aq, Bq, Ak, Bk, Av, Bv, Ao, Bo, slot=None):
        _frozen(ctx, tuple(range(2, 10)), "SiglipAttentionLoRAFn")
        ctx.slot = slot
        ops = _lora_ops()
        x, res = _c(x), _c(res)
        M, Hd = x.shape
        t = ops.down(x, [Aq, Ak, Av], r)
        qkv = _empty(M, 3 * Hd, like=x)
        K.linear_fwd(x, [wq, wk, wv], qkv, kind=L.EPI_BIAS, bias=_cat_views([bq, bk, bv]))
        ops.up(qkv, t, [Bq, Bk, Bv], r, scaling)
        attn = _empty(M, Hd, like=x)
        lse = _empty(cfg.B, cfg.H, cfg.L, dtype=F32, like=x)
        a = K.attn_args(cfg.B, cfg.L, cfg.H, cfg.H, cfg.D, qkv[:, :Hd], qkv.stride(0), qkv[:, Hd:2 * Hd],
                        qkv.stride(0), qkv[:, 2 * Hd:], qkv.stride(0), cfg.scale)
        K.attn_fwd(a, attn, lse)
        t_o = ops.down(attn, [Ao], r)
        out = _empty(M, Hd, like=x)
        K.linear_fwd(attn, [wo], out, kind=L.EPI_BIAS, bias=bo)
        ops.up(out, t_o, [Bo], r, scaling, resid=res)
        ctx.save_for_backward(x, wq, wk, wv, wo, qkv, attn, lse, t, t_o, Aq, Bq, Ak, Bk, Av, Bv, Ao, Bo)
        ctx.cfg, ctx.scaling, ctx.r = cfg, scaling, r
        return out

    @staticmethod
    def backward(ctx, dout):
        x, wq, wk, wv, wo, qkv, attn, lse, t, t_o, Aq, Bq, Ak, Bk, Av, Bv, Ao, Bo = ctx.saved_tensors
        cfg, s, r = ctx.cfg, ctx.scaling, ctx.r
        ops = _lora_ops()
        dout = _c(dout)
        M, Hd = x.shape
        nig = ctx.needs_input_grad
        dt_o, g_o = _lora_grads(ops, dout, t_o, attn, r, s, [Bo], [Ao], nig[19:21])
        dattn = torch.empty_like(attn)
        K.linear_dgrad(dout, [wo], dattn)
        ops.up_t(dattn, dt_o, [Ao], r)
        dqkv = torch.empty_like(qkv)
        a = K.attn_args(cfg.B, cfg.L, cfg.H, cfg.H, cfg.D, qkv[:, :Hd], qkv.stride(0), qkv[:, Hd:2 * Hd],
                        qkv.stride(0), qkv[:, 2 * Hd:], qkv.stride(0), cfg.scale)
        ld = dqkv.stride(0)
        K.attn_bwd(a, attn, dattn, lse, dqkv[:, :Hd], ld, dqkv[:, Hd:2 * Hd], ld, dqkv[:, 2 * Hd:], ld)
        dt, g_qkv = _lora_grads(ops, dqkv, t, x, r, s, [Bq, Bk, Bv], [Aq, Ak, Av], nig[13:19])
        dx = None
        if nig[0]:  # layer 0 reads the frozen patch embedding: nothing upstream to train
            dx = torch.empty_like(x)
            K.linear_dgrad(dqkv, [wq, wk, wv], dx)
            ops.up_t(dx, dt, [Aq, Ak, Av], r)
        dres = dout if nig[1] else None
        if ctx.slot is not None and dres is not None:  # handed to layer_norm1's backward (ResidualSlot)
            ctx.slot.put(dout)
            dres = None
        return (dx, dres, *([None] * 11), *g_qkv, *g_o, None)


class SiglipMLPLoRAFn(torch.autograd.Function):
    """SiglipMLPFn with a LoRA adapter on fc1 and fc2: fc1's rank-r pass leaves the adapted pre-activation in place and
    writes gelu_tanh of it (GELU), fc2's adds the encoder residual (RESID)."""

    @staticmethod
    def forward(ctx, x, res, w1, b1, w2, b2, scaling: float, r: int, A1, B1, A2, B2, slot=None):
        _frozen(ctx, (2, 3, 4, 5), "SiglipMLPLoRAFn")
        ctx.slot = slot
        ops = _lora_ops()
        x, res = _c(x), _c(res)
        M = x.shape[0]
        I = w1.shape[0]
        t1 = ops.down(x, [A1], r)
        pre = _empty(M, I, like=x)
        K.linear_fwd(x, [w1], pre, kind=L.EPI_BIAS, bias=b1)
        act = _empty(M, I, like=x)
        ops.up(pre, t1, [B1], r, scaling, gelu_out=act)
        t2 = ops.down(act, [A2], r)
        out = _empty(M, w2.shape[0], like=x)
        K.linear_fwd(act, [w2], out, kind=L.EPI_BIAS, bias=b2)
        ops.up(out, t2, [B2], r, scaling, resid=res)
        ctx.save_for_backward(x, w1, w2, pre, act, t1, t2, A1, B1, A2, B2)
        ctx.scaling, ctx.r = scaling, r
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w1, w2, pre, act, t1, t2, A1, B1, A2, B2 = ctx.saved_tensors
        s, r = ctx.scaling, ctx.r
        ops = _lora_ops()
        dout = _c(dout)
        nig = ctx.needs_input_grad
        dt2, g2 = _lora_grads(ops, dout, t2, act, r, s, [B2], [A2], nig[10:12])
        dpre = torch.empty_like(pre)
        K.linear_dgrad(dout, [w2], dpre)
        ops.up_t(dpre, dt2, [A2], r)  # the adapter's share enters dAct before the GELU derivative
        K.gelu_rows(K.GELU_TANH_BWD, dpre, dpre, pre=pre)
        dt1, g1 = _lora_grads(ops, dpre, t1, x, r, s, [B1], [A1], nig[8:10])
        dx = None
        if nig[0]:
            dx = torch.empty_like(x)
            K.linear_dgrad(dpre, [w1], dx)
            ops.up_t(dx, dt1, [A1], r)
        dres = dout if nig[1] else None
        if ctx.slot is not None and dres is not None:  # handed to layer_norm2's backward (ResidualSlot)
            ctx.slot.put(dout)
            dres = None
        return (dx, dres, None, None, None, None, None, None, *g1, *g2, None)


class LinearLoRAFn(torch.autograd.Function):
    """LinearFn with a LoRA adapter (the projector: post_scale through SCALE; Ego3D head.0: plain; head.3: the vision
    features through RESID).  A reduction dim padded to a multiple of 8 (head.0: 204 -> 208 columns of x) pads the
    base weight and A [r, 204] with zero columns per call; dA is trimmed back to the parameter's shape."""

    @staticmethod
    def forward(ctx, x, w, b, res, post_scale, scaling: float, r: int, A, B):
        _frozen(ctx, (1, 2), "LinearLoRAFn")
        ops = _lora_ops()
        x = _c(x)
        M, Kx = x.shape
        N, Kw = w.shape
        wk, Ak = w, A
        if Kx != Kw:
            wk = torch.zeros(N, Kx, dtype=BF16, device=w.device)
            wk[:, :Kw] = w
            Ak = torch.zeros(r, Kx, dtype=BF16, device=w.device)
            Ak[:, :Kw] = A.detach()
        t = ops.down(x, [Ak], r)
        y = _empty(M, N, like=x)
        if b is not None:
            K.linear_fwd(x, [wk], y, kind=L.EPI_BIAS, bias=b)
        else:
            K.linear_fwd(x, [wk], y)
        if res is not None:
            if post_scale != 1.0:
                raise NotImplementedError("LinearLoRAFn: a residual together with a post-scale")
            ops.up(y, t, [B], r, scaling, resid=_c(res))
        else:
            ops.up(y, t, [B], r, scaling, post_scale=post_scale if post_scale != 1.0 else None)
        ctx.save_for_backward(x, w, A, B, t)
        ctx.post_scale, ctx.scaling, ctx.r = post_scale, scaling, r
        ctx.has_res = res is not None
        ctx.wk, ctx.Ak = (wk, Ak) if wk is not w else (None, None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, A, B, t = ctx.saved_tensors
        s, r = ctx.scaling, ctx.r
        ops = _lora_ops()
        dy = _c(dy)
        nig = ctx.needs_input_grad
        dres = dy if ctx.has_res and nig[3] else None
        if ctx.post_scale != 1.0:
            # y = bf16(z * post): dz = bf16(dy * post) (autograd of the reference's division), as LinearFn
            dy = (dy * ctx.post_scale).to(BF16)
        if ctx.Ak is None:
            dt, (gA, gB) = _lora_grads(ops, dy, t, x, r, s, [B], [A], nig[7:9])
        else:  # dA over the padded columns into a temporary, trimmed into the parameter's destination
            dt, (tmp, gB) = _lora_grads(ops, dy, t, x, r, s, [B], [ctx.Ak], nig[7:9])
            gA = None
            if tmp is not None:
                dA, acc, gA = _grad_dest(A, True)
                src = tmp[:, :A.shape[1]]
                dA.add_(src) if acc else dA.copy_(src)
        dx = None
        if nig[0]:
            dx = torch.empty_like(x)
            K.linear_dgrad(dy, [ctx.wk if ctx.wk is not None else w], dx)
            ops.up_t(dx, dt, [ctx.Ak if ctx.Ak is not None else A], r)
        return dx, None, None, dres, None, None, None, gA, gB


class PatchEmbedFn(torch.autograd.Function):
    """SiglipVisionEmbeddings.forward (transformers siglip [3p]): Conv2d(3, H, k=s=14) + bias +
    position embedding, as im2col + one GEMM whose epilogue adds bias and position rows."""

    @staticmethod
    def forward(ctx, pix, w, b, pos, patch):
        pix = _c(pix)
        B, C, S, _ = pix.shape
        np_ = (S // patch) ** 2
        Kc = C * patch * patch
        Kp = K.round_up(Kc, 8)
        cols = _empty(B * np_, Kp, like=pix)
        K.im2col_patch(pix, patch, cols)
        w2 = w.reshape(w.shape[0], Kc)
        wk = torch.zeros(w.shape[0], Kp, dtype=BF16, device=w.device)
        wk[:, :Kc] = w2
        posx = pos.unsqueeze(0).expand(B, np_, pos.shape[1]).reshape(B * np_, pos.shape[1])
        y = _empty(B * np_, w.shape[0], like=pix)
        K.linear_fwd(cols, [wk], y, kind=L.EPI_BIAS_RESID, bias=b, in0=_c(posx))
        ctx.save_for_backward(cols, w, b, pos)
        ctx.B, ctx.np = B, np_
        return y

    @staticmethod
    def backward(ctx, dy):
        cols, w, b, pos = ctx.saved_tensors
        dy = _c(dy)
        Kc = w[0].numel()
        rw = None
        if ctx.needs_input_grad[1]:
            tmp = _empty(w.shape[0], cols.shape[1], like=cols)
            K.linear_wgrad(dy, cols, [tmp])
            dw, acc, rw = _grad_dest(w, True)
            src = tmp[:, :Kc].reshape(w.shape)
            dw.add_(src) if acc else dw.copy_(src)
        rb = _bias_grad(dy, b, ctx.needs_input_grad[2])
        rp = None
        if ctx.needs_input_grad[3]:
            dp, acc, rp = _grad_dest(pos, True)
            K.colsum_bf16(dy.view(ctx.B, ctx.np * pos.shape[1]), dp.view(-1), accumulate=acc)
        return None, rw, rb, rp, None


class EmbedMergeFn(torch.autograd.Function):
    """Embedding merge of SpatialVLAForConditionalGeneration.forward (modeling_spatialvla.py:361-387)
    times the Gemma2 normalizer (modeling_gemma2.py:741-742): token embeddings (frozen table), spatial
    action-token embeddings, image features scattered into the <image> slots in (b, t) order."""

    @staticmethod
    def forward(ctx, ids, img_index, img_feats, spatial_w, embed_w, a0, normalizer, sort_rows, offsets):
        ids = _c(ids).view(-1)
        H = embed_w.shape[1]
        out = _empty(ids.numel(), H, like=embed_w)
        na = spatial_w.shape[0] if spatial_w is not None else 0
        K.embed_merge(ids, img_index, embed_w, spatial_w, a0, na, img_feats, normalizer, out)
        ctx.save_for_backward(ids, img_index, sort_rows, offsets, spatial_w, img_feats)
        ctx.normalizer, ctx.na = normalizer, na
        return out

    @staticmethod
    def backward(ctx, dout):
        ids, img_index, sort_rows, offsets, spatial_w, img_feats = ctx.saved_tensors
        dout = _c(dout)
        dimg = torch.empty_like(img_feats) if (img_feats is not None and ctx.needs_input_grad[2]) else None
        dsp, acc, rsp = (None, False, None)
        if spatial_w is not None and ctx.needs_input_grad[3]:
            dsp, acc, rsp = _grad_dest(spatial_w, True)
            if acc:
                tmp = torch.empty_like(spatial_w)
                K.embed_merge_bwd(ids, img_index, sort_rows, offsets, ctx.na, dout, ctx.normalizer, tmp, None)
                dsp.add_(tmp)
                dsp = None
        if dimg is not None or dsp is not None:
            K.embed_merge_bwd(ids, img_index, sort_rows, offsets, ctx.na, dout, ctx.normalizer, dsp, dimg)
        return None, None, dimg, rsp, None, None, None, None, None


class EmbedMergeLoRAFn(torch.autograd.Function):
    """EmbedMergeFn with a peft Embedding adapter on the spatial table (add_lora("spatialvla-linear+emb"), reference
    train/spatialvla_finetune.py:272-278): the row of action token id is bf16(W[id] + bf16(s sum_j A[j, id] B[:, j]))
    before the normalizer, A [r, na] (lora_embedding_A), B [H, r] (lora_embedding_B).  The merge kernel runs as it
    does without an adapter and svla_lora_embed_fwd rewrites the action-token rows; the backward adds dA / dB
    (svla_lora_embed_bwd, over the CSR _merge_inputs builds) to the image-feature gradient.  The table is frozen.
    LORA_KERNELS[0] = False: the effective table W + bf16(s (B A)^T) and its gradient's two products as torch ops
    around the plain merge kernels."""

    @staticmethod
    def forward(ctx, ids, img_index, img_feats, spatial_w, embed_w, a0, normalizer, sort_rows, offsets, scaling, r,
                A, B):
        _frozen(ctx, (3, 4), "EmbedMergeLoRAFn")
        ids = _c(ids).view(-1)
        H = embed_w.shape[1]
        na = spatial_w.shape[0]
        out = _empty(ids.numel(), H, like=embed_w)
        ctx.kernels = LORA_KERNELS[0]
        if ctx.kernels:
            K.embed_merge(ids, img_index, embed_w, spatial_w, a0, na, img_feats, normalizer, out)
            K.lora_embed_fwd(ids, img_index, embed_w, spatial_w, a0, A, B, r, scaling, normalizer, out)
        else:
            delta = ((A.detach().float().t() @ B.detach().float().t()) * scaling).to(BF16)
            K.embed_merge(ids, img_index, embed_w, spatial_w.detach() + delta, a0, na, img_feats, normalizer, out)
        ctx.save_for_backward(ids, img_index, sort_rows, offsets, img_feats, A, B)
        ctx.normalizer, ctx.na, ctx.a0, ctx.scaling, ctx.r = normalizer, na, a0, scaling, r
        return out

    @staticmethod
    def backward(ctx, dout):
        ids, img_index, sort_rows, offsets, img_feats, A, B = ctx.saved_tensors
        dout = _c(dout)
        nig = ctx.needs_input_grad
        dimg = torch.empty_like(img_feats) if (img_feats is not None and nig[2]) else None
        if dimg is not None:
            K.embed_merge_bwd(ids, img_index, sort_rows, offsets, ctx.na, dout, ctx.normalizer, None, dimg)
        gA, accA, rA = _grad_dest(A, nig[11])
        gB, accB, rB = _grad_dest(B, nig[12])
        if gA is None and gB is None:
            return (None, None, dimg) + (None,) * 10
        if ctx.kernels:
            if accA == accB or gA is None or gB is None:
                K.lora_embed_bwd(ids, sort_rows, offsets, ctx.a0, ctx.na, dout, ctx.normalizer, A, B, ctx.r,
                                 ctx.scaling, gA, gB, accumulate=accA if gA is not None else accB)
            else:
                K.lora_embed_bwd(ids, sort_rows, offsets, ctx.a0, ctx.na, dout, ctx.normalizer, A, B, ctx.r,
                                 ctx.scaling, gA, None, accumulate=accA)
                K.lora_embed_bwd(ids, sort_rows, offsets, ctx.a0, ctx.na, dout, ctx.normalizer, A, B, ctx.r,
                                 ctx.scaling, None, gB, accumulate=accB)
        else:
            dsp = _empty(ctx.na, dout.shape[1], like=dout)
            K.embed_merge_bwd(ids, img_index, sort_rows, offsets, ctx.na, dout, ctx.normalizer, dsp, None)
            dsp = dsp.float()
            for g, acc, val in ((gA, accA, lambda: (dsp @ B.float()).t() * ctx.scaling),
                                (gB, accB, lambda: (dsp.t() @ A.float().t()) * ctx.scaling)):
                if g is not None:
                    v = val().to(BF16)
                    g.add_(v) if acc else g.copy_(v)
        return (None, None, dimg) + (None,) * 8 + (rA, rB)


class LMHeadCEFn(torch.autograd.Function):
    """lm_head + final logit softcap (modeling_gemma2.py:993-997) + the shifted, masked cross-entropy of
    SpatialVLAForConditionalGeneration.forward (modeling_spatialvla.py:415-430).  Logits are written once
    in bf16 (row stride padded to a multiple of 64 columns); softmax statistics come from the GEMM
    epilogue, so the fp32 [B, L, V] tensor of the reference is never materialised.
    Returns (logits [M, V] view, loss scalar fp32); argmax / lse are stashed on ctx-owned tensors."""

    @staticmethod
    def _lora_setup(ctx, n_in, scaling, r, A, B):
        """The optional lm_head adapter (add_lora("spatialvla-linear+emb+h")): logits = bf16(W h) + bf16(s B (A h))
        before the softcap, svla_lora_up's rounding points.  Its term is added by the pass that softcaps the raw
        logits (svla_lora_softcap_ce_rows: one trip over the buffer instead of two); the base weight is frozen."""
        ctx.n_in = n_in
        ctx.lora = None
        if A is not None:
            _frozen(ctx, (1,), "LMHeadCEFn")
            ctx.lora = (float(scaling), int(r))

    @staticmethod
    def _lora_softcap(logits_buf, V, stats, cap, x, lora, A, B):
        """t = x A^T, then the adapter term, the softcap and the statistics on the raw logits; returns t."""
        s, r = lora
        t = _lora_ops().down(x, [A], r)
        if LORA_KERNELS[0]:
            K.lora_softcap_ce_rows(logits_buf, V, t, B, r, s, stats, cap)
        else:
            u = _empty(x.shape[0], logits_buf.shape[1], like=x)
            K.linear_fwd(t[:, :r], [B], u[:, :V], alpha=s)
            logits_buf[:, :V] += u[:, :V]
            K.softcap_ce_rows(logits_buf, V, stats, cap)
        return t

    @staticmethod
    def _lora_backward(ctx, dlog, V, x_r, t_r, A, B, dh_r):
        """From dlog [R, ld] (zero beyond V): dt = s dlog B (a reduction over V, on the general GEMM with N = r),
        dB = s dlog^T t (the general GEMM with r output columns), dA = dt^T x, and dh_r += dt A (svla_lora_wgrad /
        svla_lora_up summed mode, or their compositions).  Returns (dA, dB) for autograd."""
        s, r = ctx.lora
        ops = _lora_ops()
        R, ldv = dlog.shape
        dt = torch.zeros(R, K.lora_R(r), dtype=BF16, device=dlog.device)
        K.gemm(R, r, ldv, K._operand([dlog], L.LAYOUT_KC, k_valid=ldv), K._operand([B], L.LAYOUT_RC, k_valid=V),
               [dt], [0], dt.stride(0), K._epi(L.EPI_STORE, alpha=s))
        nA, nB = ctx.needs_input_grad[7], ctx.needs_input_grad[8]
        gB, accB, rB = _grad_dest(B, nB)
        if gB is not None:
            K.gemm(V, r, R, K._operand([dlog[:, :V]], L.LAYOUT_RC), K._operand([_c(t_r[:, :r])], L.LAYOUT_RC),
                   [gB], [0], r, K._epi(L.EPI_STORE, accumulate=accB, alpha=s))
        dA = _grad_dest(A, nA)
        if dA[0] is not None:
            ops.wgrad(x_r, dt, [dA], r, False, 1.0, None)
        if dh_r is not None:
            ops.up_t(dh_r, dt, [A], r)
        return dA[2], rB

    @staticmethod
    def _ret(ctx, dh, rw, rA=None, rB=None):
        out = (dh, rw, None, None, None, None, None, rA, rB)
        return out[:ctx.n_in]

    @staticmethod
    def forward(ctx, h, w, target, cap, stash, *adapter):
        """adapter: () or (scaling, r, A [r, H], B [V, r]) -- the lm_head LoRA adapter."""
        h = _c(h)
        M = h.shape[0]
        V = w.shape[0]
        ldv = K.round_up(V, 64)
        scaling, r, A, B = adapter if adapter else (None, 0, None, None)
        LMHeadCEFn._lora_setup(ctx, 5 + len(adapter), scaling, r, A, B)
        rows = stash.pop("label_rows", None) if stash is not None else None
        if rows is not None:
            return LMHeadCEFn._forward_rows(ctx, h, w, target, cap, stash, rows, A, B)
        ctx.rows_only = False
        logits_buf = _empty(M, ldv, like=h)
        ntn = K.ceil_div(V, 128)
        stats = _empty(M, ntn, 3, dtype=F32, like=h)
        # plain-store GEMM (the 4-wave kernel's direct epilogue), then softcap + statistics as one HBM pass: the
        # VALU-heavy SOFTCAP_CE epilogue inside the GEMM cost 13.4-13.9 ms per step against 9.2 + ~2 ms
        K.linear_fwd(h, [w], logits_buf[:, :V])
        t = None
        if ctx.lora is not None:
            t = LMHeadCEFn._lora_softcap(logits_buf, V, stats, cap, h, ctx.lora, A, B)
        else:
            K.softcap_ce_rows(logits_buf, V, stats, cap)
        lse = _empty(M, dtype=F32, like=h)
        argmax = _empty(M, dtype=torch.int64, like=h)
        loss_rows = _empty(M, dtype=F32, like=h)
        loss2 = _empty(2, dtype=F32, like=h)
        K.ce_finalize(V, ntn, stats, logits_buf[:, :V], target, lse, argmax, loss_rows, loss2)
        stash["argmax"] = argmax
        stash["lse"] = lse
        stash["n_valid"] = loss2[1:2]
        ctx.save_for_backward(h, w, logits_buf, lse, target, loss2, t, A, B)
        ctx.cap, ctx.V = cap, V
        ctx.row_plan = stash.pop("row_plan", None) if stash is not None else None
        ctx.mark_non_differentiable(logits_buf)
        # the logits output never receives a gradient: without this autograd hands backward a materialised zero
        # [M, V] bf16 tensor (5.3 GB at B=32, ~0.9 ms of fills per step, r4 ATen attribution)
        ctx.set_materialize_grads(False)
        return logits_buf[:, :V], loss2[0]

    @staticmethod
    def _forward_rows(ctx, h, w, target, cap, stash, rows, A=None, B=None):
        """The training step's form (stash["label_rows"]: the R > 0 rows with a label, on the device, R known on the
        host): the loss is a mean over those rows and its caller reads nothing else, so the projection, the softcap
        pass and the statistics run over them alone -- the same plain-store GEMM over the gathered rows of h (each
        row's logits bitwise those of the full product), R/M of the work and of the logits buffer.  No logits output
        (None); argmax / lse keep their length M, -1 / NaN on the rows without a label.
        The gather, the GEMM, the softcap pass and the statistics are libsvla kernels; the bookkeeping on length-R and
        length-M vectors is torch (index_select of the targets, full + index_copy_ for argmax and lse: five launches
        over at most M elements each)."""
        M, V = h.shape[0], w.shape[0]
        R = int(rows.numel())
        ldv = K.round_up(V, 64)
        h_r = _empty(R, h.shape[1], like=h)
        K.gather_rows(rows, h, h_r)
        tgt_r = target.index_select(0, rows)
        logits_r = _empty(R, ldv, like=h)
        ntn = K.ceil_div(V, 128)
        stats = _empty(R, ntn, 3, dtype=F32, like=h)
        K.linear_fwd(h_r, [w], logits_r[:, :V])
        t_r = None
        if ctx.lora is not None:
            t_r = LMHeadCEFn._lora_softcap(logits_r, V, stats, cap, h_r, ctx.lora, A, B)
        else:
            K.softcap_ce_rows(logits_r, V, stats, cap)
        lse_r = _empty(R, dtype=F32, like=h)
        argmax_r = _empty(R, dtype=torch.int64, like=h)
        loss_rows = _empty(R, dtype=F32, like=h)
        loss2 = _empty(2, dtype=F32, like=h)
        K.ce_finalize(V, ntn, stats, logits_r[:, :V], tgt_r, lse_r, argmax_r, loss_rows, loss2)
        stash["argmax"] = torch.full((M,), -1, dtype=torch.int64, device=h.device).index_copy_(0, rows, argmax_r)
        stash["lse"] = torch.full((M,), float("nan"), dtype=F32, device=h.device).index_copy_(0, rows, lse_r)
        stash["n_valid"] = loss2[1:2]
        stash.pop("row_plan", None)
        ctx.save_for_backward(h_r, w, logits_r, lse_r, tgt_r, loss2, rows, t_r, A, B)
        ctx.cap, ctx.V, ctx.M = cap, V, M
        ctx.rows_only = True
        ctx.set_materialize_grads(False)
        return None, loss2[0]

    @staticmethod
    def _backward_rows(ctx, dloss):
        h_r, w, logits_r, lse_r, tgt_r, loss2, rows, t_r, lA, lB = ctx.saved_tensors
        R, ldv = logits_r.shape
        V = ctx.V
        gscale = (dloss.float() / torch.clamp(loss2[1], min=1.0)).reshape(1).contiguous()
        dw, acc, rw = _grad_dest(w, ctx.needs_input_grad[1])
        dlog = _empty(R, ldv, like=h_r)
        K.ce_bwd(V, logits_r[:, :V], lse_r, tgt_r, ctx.cap, gscale, dlog)
        dh, dh_r = None, None
        if ctx.needs_input_grad[0]:
            dh_r = _empty(R, h_r.shape[1], like=h_r)
            A = K._operand([dlog], L.LAYOUT_KC, k_valid=ldv)
            Bop = K._operand([w], L.LAYOUT_RC, k_valid=V)
            K.gemm(R, w.shape[1], ldv, A, Bop, [dh_r], [0], dh_r.stride(0), K._epi(L.EPI_STORE))
        rA = rB = None
        if ctx.lora is not None:
            rA, rB = LMHeadCEFn._lora_backward(ctx, dlog, V, h_r, t_r, lA, lB, dh_r)
        if dh_r is not None:
            dh = _empty(ctx.M, h_r.shape[1], like=h_r)
            K.scatter_rows(rows, dh_r, dh)
        if dw is not None:
            K.linear_wgrad(dlog[:, :V], h_r, [dw], accumulate=acc)
        return LMHeadCEFn._ret(ctx, dh, rw, rA, rB)

    @staticmethod
    def backward(ctx, dlogits_unused, dloss):
        """d(loss)/d(logits) is exactly zero on every row without a label (target < 0: the reference's
        CrossEntropyLoss ignore_index / attention-mask rows, modeling_spatialvla.py:415-430) -- at B=32 only the
        13 suffix rows of each 312-token episode carry one.  The softmax gradient and both lm_head backward GEMMs
        therefore run over the labelled rows only: dh is zero elsewhere and dW = sum over labelled rows, the same
        values as the dense products (whose other terms are exact zeros), at 1/24 of their cost."""
        if dloss is None:  # the loss did not reach the graph's output
            return LMHeadCEFn._ret(ctx, None, None)
        if ctx.rows_only:
            return LMHeadCEFn._backward_rows(ctx, dloss)
        h, w, logits_buf, lse, target, loss2, t, lA, lB = ctx.saved_tensors
        M, ldv = logits_buf.shape
        V = ctx.V
        gscale = (dloss.float() / torch.clamp(loss2[1], min=1.0)).reshape(1).contiguous()
        if ctx.row_plan is not None:  # labelled rows first + their count, fetched behind the forward's event
            order, cnt, ev = ctx.row_plan
            if ev is not None:
                ev.synchronize()
                cnt = int(cnt[0])
            rows = order[:cnt]
        else:
            rows = torch.nonzero(target >= 0).view(-1)
        R = int(rows.numel())
        dh = torch.zeros_like(h) if ctx.needs_input_grad[0] else None
        dw, acc, rw = _grad_dest(w, ctx.needs_input_grad[1])
        if R == 0:
            if dw is not None and not acc:
                dw.zero_()
            rets = []
            if ctx.lora is not None:  # no label: zero adapter gradients
                for p, need in ((lA, ctx.needs_input_grad[7]), (lB, ctx.needs_input_grad[8])):
                    g, gacc, ret = _grad_dest(p, need)
                    if g is not None and not gacc:
                        g.zero_()
                    rets.append(ret)
            return LMHeadCEFn._ret(ctx, dh, rw, *rets)
        dlog = _empty(R, ldv, like=h)
        K.ce_bwd(V, logits_buf.index_select(0, rows)[:, :V], lse.index_select(0, rows),
                 target.index_select(0, rows).contiguous(), ctx.cap, gscale, dlog)
        dh_r = None
        if dh is not None:
            dh_r = _empty(R, h.shape[1], like=h)
            # reduction over the padded vocab: dlog is zero in [V, ldv); W rows beyond V read as 0 (k_valid=V)
            A = K._operand([dlog], L.LAYOUT_KC, k_valid=ldv)
            Bop = K._operand([w], L.LAYOUT_RC, k_valid=V)
            K.gemm(R, w.shape[1], ldv, A, Bop, [dh_r], [0], dh_r.stride(0), K._epi(L.EPI_STORE))
        rA = rB = None
        if ctx.lora is not None:
            rA, rB = LMHeadCEFn._lora_backward(ctx, dlog, V, h.index_select(0, rows).contiguous(),
                                               t.index_select(0, rows), lA, lB, dh_r)
        if dh is not None:
            dh.index_copy_(0, rows, dh_r)
        if dw is not None:
            K.linear_wgrad(dlog[:, :V], h.index_select(0, rows).contiguous(), [dw], accumulate=acc)
        return LMHeadCEFn._ret(ctx, dh, rw, rA, rB)


def lm_head_fp8_decode_ok(h: torch.Tensor) -> bool:
    """Whether the decode head runs on the e4m3 lm_head: no grad, M <= 8 rows and a width svla_head_gemv_mxfp8 takes."""
    return not torch.is_grad_enabled() and h.is_cuda and K.head_gemv_mxfp8_ok(h.shape[0], h.shape[1])


def lm_head_fp8_decode(h, w, target, cap, stash, f8d: FP8DecodeWeights):
    """LMHeadCEFn's forward for a decode step (M <= 8 rows, no grad) on the e4m3 copy of lm_head: svla_head_gemv_mxfp8
    streams the copy once and leaves the softcapped logits and the statistics, then svla_ce_finalize.  Returns
    (logits [M, V] view, loss)."""
    h = _c(h)
    (wq,), (ws,) = f8d.get("lm_head", [w])
    return _decode_head(h, w.shape[0], target, stash,
                        lambda logits_buf, V, stats: K.head_gemv_mxfp8(h, wq, ws, logits_buf, V, stats, cap))


def _decode_head(h, V, target, stash, stream_lm_head):
    """The part every decode head shares: stream_lm_head(logits_buf, V, stats) passes over lm_head once and leaves the
    softcapped logits and the per-tile statistics, svla_ce_finalize turns those into lse, argmax and the loss, and the
    stash gets what LMHeadCEFn leaves there.  Returns (logits [M, V] view, loss)."""
    M = h.shape[0]
    logits_buf = _empty(M, K.round_up(V, 64), like=h)
    ntn = K.ceil_div(V, 128)
    stats = _empty(M, ntn, 3, dtype=F32, like=h)
    stream_lm_head(logits_buf, V, stats)
    lse = _empty(M, dtype=F32, like=h)
    argmax = _empty(M, dtype=torch.int64, like=h)
    loss_rows = _empty(M, dtype=F32, like=h)
    loss2 = _empty(2, dtype=F32, like=h)
    K.ce_finalize(V, ntn, stats, logits_buf[:, :V], target, lse, argmax, loss_rows, loss2)
    stash["argmax"] = argmax
    stash["lse"] = lse
    stash["n_valid"] = loss2[1:2]
    return logits_buf[:, :V], loss2[0]


def lm_head_lora_decode_ok(h: torch.Tensor, r: int) -> bool:
    """Whether the decode head with an lm_head adapter runs as lm_head_lora_decode: no grad, M <= 8 rows, the decode
    adapter kernels on (SVLA_LORA_DECODE_KERNELS) and a width svla_lora_head_gemv takes."""
    return (not torch.is_grad_enabled() and LORA_DECODE_KERNELS[0] and LORA_DECODE_EMB_HEAD_KERNELS[0] and h.is_cuda
            and K.lora_head_gemv_ok(h.shape[0], h.shape[1], r))


def lm_head_lora_decode(h, w, target, cap, stash, scaling, r, A, B, f8d: Optional[FP8DecodeWeights] = None):
    """LMHeadCEFn's forward for a decode step (M <= 8 rows, no grad) with the lm_head adapter attached, in the launch
    count of the head without one: t = h A^T (svla_lora_gemv_down), then svla_lora_head_gemv streams lm_head once and
    leaves the softcapped logits and the statistics, then svla_ce_finalize.  f8d (enable_fp8_lora_decode): the e4m3
    copy of lm_head is streamed instead (svla_lora_head_gemv_mxfp8) where that kernel takes the width.  Returns
    (logits [M, V] view, loss)."""
    h = _c(h)
    M = h.shape[0]
    t = _empty(M, K.lora_R(r), like=h)
    K.lora_gemv_down(h, [A], r, t)

    def stream_lm_head(logits_buf, V, stats):
        if f8d is not None and K.lora_head_gemv_mxfp8_ok(M, h.shape[1], r):
            (wq,), (ws,) = f8d.get("lm_head", [w])
            K.lora_head_gemv_mxfp8(h, wq, ws, t, B, r, scaling, logits_buf, V, stats, cap)
        else:
            K.lora_head_gemv(h, w, t, B, r, scaling, logits_buf, V, stats, cap)
    return _decode_head(h, w.shape[0], target, stash, stream_lm_head)


# ------------------------------------------------------------------------------------ attention plug-in
def kv_class_from_additive_mask(mask: Optional[torch.Tensor], B: int, Lq: int, Lk: int, device) -> torch.Tensor:
    """Per-key classes (0 visible to all queries, 1 visible to queries i >= j, 2 never visible) equivalent to
    the reference's additive [B,1,Lq,Lk] mask (modeling_spatialvla.py:258-306).  Raises ValueError when the
    mask is not of that form (the kernel never materialises an L x L mask)."""
    if mask is None:
        return torch.zeros(B, Lk, dtype=torch.uint8, device=device)
    if Lq != Lk:
        raise ValueError(f"svla attention: query length {Lq} != key length {Lk} (KV cache not supported)")
    vis = mask[:, 0, :, :Lk] == 0                                   # [B, Lq, Lk]
    all_vis = vis.all(dim=1)
    none_vis = ~vis.any(dim=1)
    cls = torch.where(all_vis, 0, torch.where(none_vis, 2, 1)).to(torch.uint8)
    i = torch.arange(Lq, device=device)
    causal = i[:, None] >= i[None, :]
    rebuilt = torch.where(cls[:, None, :] == 0, True, torch.where(cls[:, None, :] == 2, False, causal[None]))
    if not bool((rebuilt == vis).all()):
        raise ValueError("svla attention: mask is not a per-key prefix-LM/causal/padding mask")
    return cls.contiguous()


def gemma2_attention_forward(module, query, key, value, mask, **_kwargs):
    """Drop-in entry for the reference's plugin table GEMMA2_ATTENTION_FUNCTION (modeling_gemma2.py:317-322,
    called at :401-403 as fn(self, q, k, v, attention_mask, output_attentions=...)).  Same arguments and
    return as eager_attention_forward (:169-195): q [B,Hq,L,D], k/v [B,Hkv,L,D] after RoPE, additive mask
    [B,1,L,L] or None -> (out [B,L,Hq,D] contiguous, None).  Scale = module.scaling, softcap =
    module.attn_logit_softcapping; probabilities are rounded to bf16 before PV as in the reference (Q3)."""
    if _kwargs.get("output_attentions"):
        raise NotImplementedError("svla attention does not materialise attention weights")
    B, _, Lq, _ = query.shape
    cls = kv_class_from_additive_mask(mask, B, Lq, key.shape[2], query.device)
    softcap = getattr(module, "attn_logit_softcapping", None) or 0.0
    return hip_attention(query, key, value, module.scaling, softcap, cls, 0), None


def hip_attention(q, k, v, scale, softcap=0.0, kv_class=None, window=0):
    """Reference plug-in signature adapter (GEMMA2_ATTENTION_FUNCTION, modeling_gemma2.py:317-322):
    q [B, Hq, L, D], k/v [B, Hkv, L, D] (post-RoPE) -> [B, L, Hq, D].  Differentiable."""
    return _PluginAttnFn.apply(q, k, v, float(scale), float(softcap or 0.0), kv_class, int(window or 0))


class _PluginAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, softcap, kv_class, window):
        B, Hq, Lq, D = q.shape
        Hkv = k.shape[1]
        qt = q.transpose(1, 2).contiguous().view(B * Lq, Hq * D)
        kt = k.transpose(1, 2).contiguous().view(B * Lq, Hkv * D)
        vt = v.transpose(1, 2).contiguous().view(B * Lq, Hkv * D)
        out = _empty(B * Lq, Hq * D, like=q)
        lse = _empty(B, Hq, Lq, dtype=F32, like=q)
        a = K.attn_args(B, Lq, Hq, Hkv, D, qt, qt.stride(0), kt, kt.stride(0), vt, vt.stride(0), scale, softcap,
                        kv_class, window)
        K.attn_fwd(a, out, lse)
        ctx.save_for_backward(qt, kt, vt, out, lse, kv_class)
        ctx.meta = (B, Lq, Hq, Hkv, D, scale, softcap, window)
        return out.view(B, Lq, Hq, D)

    @staticmethod
    def backward(ctx, dout):
        qt, kt, vt, out, lse, kv_class = ctx.saved_tensors
        B, Lq, Hq, Hkv, D, scale, softcap, window = ctx.meta
        do = _c(dout).view(B * Lq, Hq * D)
        dq, dk, dv = torch.empty_like(qt), torch.empty_like(kt), torch.empty_like(vt)
        a = K.attn_args(B, Lq, Hq, Hkv, D, qt, qt.stride(0), kt, kt.stride(0), vt, vt.stride(0), scale, softcap,
                        kv_class, window)
        K.attn_bwd(a, out, do, lse, dq, dq.stride(0), dk, dk.stride(0), dv, dv.stride(0))
        tr = lambda t, H: t.view(B, Lq, H, D).transpose(1, 2)  # noqa: E731
        return tr(dq, Hq), tr(dk, Hkv), tr(dv, Hkv), None, None, None, None


# ------------------------------------------------------------------------------------ BEiT layer (ZoeDepth)
def _beit_weights(layer):
    """q|k|v weight [3H, H] and bias [3H] (k has none) of a BeitLayer, concatenated once and cached against the
    parameters' storage and version (the estimator is frozen)."""
    at = layer.attention
    ps = (at.q_proj.weight, at.k_proj.weight, at.v_proj.weight, at.q_proj.bias, at.v_proj.bias)
    key = tuple((p.data_ptr(), p._version) for p in ps)
    hit = getattr(layer, "_svla_qkv", None)
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    w = torch.cat([at.q_proj.weight, at.k_proj.weight, at.v_proj.weight], 0).contiguous()
    b = torch.cat([at.q_proj.bias, torch.zeros_like(at.k_proj.weight[:, 0]), at.v_proj.bias], 0).contiguous()
    layer._svla_qkv = (key, w, b)
    return w, b


def _layer_scale(lam, H, like):
    if isinstance(lam, torch.Tensor):
        return _c(lam.to(like.dtype))
    return torch.full((H,), float(lam), dtype=like.dtype, device=like.device)


def beit_layer(layer, hidden_states, bias):
    """transformers BeitLayer.forward [3p] (the ZoeDepth backbone, called at model/modeling_spatialvla.py:314-323)
    in inference on the HIP kernels:
        h = x + lambda_1 * o_proj(attn(q_proj|k_proj|v_proj(LN_before(x)), + rel-pos bias))
        y = h + lambda_2 * fc2(gelu(fc1(LN_after(h))))
    LayerNorm: svla_layernorm_fwd; the three projections one GEMM with the [bq, 0, bv] bias epilogue; attention
    svla_attn_fwd at head_dim 64 with the additive bias (fp32 scores and softmax, P in bf16); o_proj and fc2 with
    the BIAS_SCALE_RESID epilogue (bf16(bf16(lambda * bf16(acc + b)) + residual), the module's rounding points);
    fc1 with BIAS_GELU_ERF.  bias: [heads, L, ld] bf16 or None."""
    B, Lq, H = hidden_states.shape
    at = layer.attention
    D = at.head_dim
    nh = at.num_attention_heads
    x = _c(hidden_states).view(B * Lq, H)
    M = B * Lq
    ln_before, ln_after = layer.layernorm_before, layer.layernorm_after
    mean = _empty(M, dtype=F32, like=x)
    rstd = _empty(M, dtype=F32, like=x)
    xn = _empty(M, H, like=x)
    K.layernorm_fwd(x, ln_before.weight, ln_before.bias, float(ln_before.eps), xn, mean, rstd)
    wqkv, bqkv = _beit_weights(layer)
    qkv = _empty(M, 3 * H, like=x)
    K.linear_fwd(xn, [wqkv], qkv, kind=L.EPI_BIAS, bias=bqkv)
    a = K.attn_args(B, Lq, nh, nh, D, qkv[:, :H], qkv.stride(0), qkv[:, H:2 * H], qkv.stride(0), qkv[:, 2 * H:],
                    qkv.stride(0), float(at.scaling), 0.0, None, 0, bias=bias)
    ctx = _empty(M, H, like=x)
    lse = _empty(B, nh, Lq, dtype=F32, like=x)
    K.attn_fwd(a, ctx, lse)
    h = _empty(M, H, like=x)
    K.linear_fwd(ctx, [at.o_proj.weight], h, kind=L.EPI_BIAS_SCALE_RESID, bias=at.o_proj.bias,
                 colscale=_layer_scale(layer.lambda_1, H, x), in0=x)
    K.layernorm_fwd(h, ln_after.weight, ln_after.bias, float(ln_after.eps), xn, mean, rstd)
    f1 = _empty(M, layer.mlp.fc1.weight.shape[0], like=x)
    if GELU_PASS[0]:
        K.linear_fwd(xn, [layer.mlp.fc1.weight], f1, kind=L.EPI_BIAS, bias=layer.mlp.fc1.bias)
        K.gelu_rows(K.GELU_ERF, f1, f1)
    else:
        K.linear_fwd(xn, [layer.mlp.fc1.weight], f1, kind=L.EPI_BIAS_GELU_ERF, bias=layer.mlp.fc1.bias)
    y = _empty(M, H, like=x)
    K.linear_fwd(f1, [layer.mlp.fc2.weight], y, kind=L.EPI_BIAS_SCALE_RESID, bias=layer.mlp.fc2.bias,
                 colscale=_layer_scale(layer.lambda_2, H, x), in0=h)
    return y.view(B, Lq, H)
