"""SpatialVLAForConditionalGeneration on MI355X: the drop-in model class.

Mirrors the reference's public surface (model/modeling_spatialvla.py:162-526): constructor
signature, sub-module attribute names (= state-dict keys), `forward(...)`
arguments and the `SpatialVLACausalLMOutputWithPast` return, `get_image_features`,
`backproject_patch`, `predict_action`, `from_pretrained` (spatial-embedding tail copy :524-525).

Hot-path compute runs on libsvla (HIP, gfx950) through `spatialvla_amd.functional`:
SigLIP, Ego3D, projector, embedding merge, 26 Gemma2 layers, softcapped lm_head + CE.
The frozen ZoeDepth estimator runs under no_grad with its BEiT layers, every convolution, the DPT resizes and the
metric-head tail on libsvla (zoe_fast); its preprocessing (reflect pad + bicubic, process_zoe) and the attractor /
seed-regressor modules are the remaining stock PyTorch-ROCm ops.
"""
import os
import warnings
from dataclasses import dataclass
from typing import List, Optional, Tuple, Union

import torch
import torch.nn.functional as F
from torch import nn
from transformers import GenerationMixin, PreTrainedModel
from transformers.utils import ModelOutput

from . import functional as Fn
from . import zoe_fast

# the Zoe depth + Ego3D encoding of the training forward on the side stream beside SigLIP (SVLA_ZOE_STREAM=0: serial)
ZOE_STREAM = [os.environ.get("SVLA_ZOE_STREAM", "1") != "0"]
# ... also inside the captured B=1 prefill graph (two branches of the graph): prefill + first token 15.3 -> 12.6 ms,
# configs[1] (prompt -> 4 tokens) 20.9 -> 18.2 ms (profiles/r8y_prefill_zoe_branch_ab.txt)
ZOE_STREAM_CAPTURE = [os.environ.get("SVLA_ZOE_STREAM_CAPTURE", "1") != "0"]
from . import kernels as K
from .configuration_spatialvla import SpatialVLAConfig
from .modeling_gemma2 import LORA_TARGETS, Gemma2ForCausalLM, Gemma2KVCache, KVMask, LoRAAdapter
from .modeling_siglip import SiglipVisionModel

SIGLIP_MEAN, SIGLIP_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)
# the module-name suffixes the reference's default lora_target="linear" hands to peft (train/spatialvla_finetune.py:
# 264-270), in its order; peft matches by suffix, so q_proj / k_proj / v_proj also catch the SigLIP attention
LORA_TARGETS_FULL = ("q_proj", "o_proj", "k_proj", "v_proj", "gate_proj", "up_proj", "down_proj", "fc1", "fc2",
                     "out_proj", "linear", "position_embedding_head.0", "position_embedding_head.3")
# ... and of its lora_target="linear+emb" / "linear+emb+h" (train/spatialvla_finetune.py:272-286): also a peft Embedding
# adapter on spatial_embed_tokens, and a Linear adapter on lm_head
LORA_TARGETS_EMB = LORA_TARGETS_FULL + ("spatial_embed_tokens",)
LORA_TARGETS_EMB_H = LORA_TARGETS_FULL[:7] + ("lm_head",) + LORA_TARGETS_FULL[7:] + ("spatial_embed_tokens",)
LORA_SETS = {"gemma2-linear": LORA_TARGETS, "spatialvla-linear": LORA_TARGETS_FULL,
             "spatialvla-linear+emb": LORA_TARGETS_EMB, "spatialvla-linear+emb+h": LORA_TARGETS_EMB_H}
SPATIAL_TABLE = "spatial_embed_tokens"
ZOE_MEAN, ZOE_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)


class LoRAEmbeddingAdapter(nn.Module):
    """The LoRA pair of an nn.Embedding (peft's Embedding LoRA layer): the looked-up row of id gains
    scaling * (B A)^T[id, :] with A = lora_embedding_A [r, num_embeddings], B = lora_embedding_B [dim, r], bf16.
    Attached as `<embedding>.lora`, so the parameters are `<embedding>.lora.A` / `.lora.B` and the base state-dict keys
    stay as they are."""

    def __init__(self, A: torch.Tensor, B: torch.Tensor, r: int, lora_alpha: float):
        super().__init__()
        self.A = nn.Parameter(A)
        self.B = nn.Parameter(B)
        self.r = int(r)
        self.lora_alpha = float(lora_alpha)
        self.scaling = float(lora_alpha) / int(r)

    def extra_repr(self):
        return f"r={self.r}, lora_alpha={self.lora_alpha}"


class Ego3DPositionEmbeddingMLP(nn.Module):
    """Reference :41-97.  Frequency encoding is done by the svla_ego3d_encode kernel (fused with the
    depth back-projection); the MLP head runs on HIP GEMM/LayerNorm/ReLU kernels and its last Linear
    adds the SigLIP features in its epilogue (:327-328)."""

    def __init__(self, in_channels=3, num_pos_feats=768, n_freqs=8, logscale=True):
        super().__init__()
        self.n_freqs = n_freqs
        self.freq_out_channels = in_channels * (2 * n_freqs + 1)
        if not logscale:
            raise ValueError("only logscale frequency bands are used by SpatialVLA")
        freq_bands = 2 ** torch.linspace(0, n_freqs - 1, n_freqs)
        center = torch.tensor([0.0, 0.0, 2.0]).repeat(in_channels // 3)
        self.register_buffer("freq_bands", freq_bands, persistent=False)
        self.register_buffer("center", center, persistent=False)
        self.position_embedding_head = nn.Sequential(
            nn.Linear(self.freq_out_channels, num_pos_feats),
            nn.LayerNorm(num_pos_feats),
            nn.ReLU(),
            nn.Linear(num_pos_feats, num_pos_feats),
        )
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p, gain=0.01)

    def forward_residual(self, feat_padded, residual2d):
        """feat_padded [N, round8(F)] (zero tail) -> residual + head(feat)."""
        h0, ln, _, h3 = self.position_embedding_head
        x = _linear(h0, feat_padded, None, 1.0)
        x = Fn.LayerNormFn.apply(x, ln.weight, ln.bias, ln.eps, None)
        x = Fn.ReLUFn.apply(x)
        return _linear(h3, x, residual2d, 1.0)


def _linear(lin, x, res, post_scale):
    """Fn.LinearFn on an nn.Linear, or Fn.LinearLoRAFn when add_lora("spatialvla-linear") attached an adapter to it."""
    ad = getattr(lin, "lora", None)
    if ad is None:
        return Fn.LinearFn.apply(x, lin.weight, lin.bias, res, post_scale)
    return Fn.LinearLoRAFn.apply(x, lin.weight, lin.bias, res, post_scale, ad.scaling, ad.r, ad.A, ad.B)


_ZOE_CONSTS = {}


def _zoe_norm_consts(dtype, device):
    """Zoe mean/std as device tensors, made once per (dtype, device): no host->device copy per call, so the
    preprocessing can sit inside a captured HIP graph."""
    key = (dtype, str(device))
    if key not in _ZOE_CONSTS:
        _ZOE_CONSTS[key] = (torch.tensor(ZOE_MEAN, dtype=dtype, device=device).view(1, -1, 1, 1),
                            torch.tensor(ZOE_STD, dtype=dtype, device=device).view(1, -1, 1, 1))
    return _ZOE_CONSTS[key]


def process_zoe(pixel_values, pad_mode="reflect", output_size=(384, 512)):
    """Reference :99-110 (ZoeDepth preprocessing): reflect pad 31, bicubic to 384^2 (align_corners), normalise.  On
    the GPU (bf16) one libsvla kernel (svla_zoe_preprocess); other devices / dtypes run the stock ops."""
    ph, pw = 31, 31
    if pixel_values.is_cuda and pixel_values.dtype == torch.bfloat16 and pad_mode == "reflect":
        C = pixel_values.shape[1]  # mean / std as the bf16 values TF.normalize uses on a bf16 image
        return (K.zoe_preprocess(pixel_values.contiguous(), ph, (384, 384),
                                 [float(torch.tensor(v, dtype=torch.bfloat16)) for v in ZOE_MEAN[:C]],
                                 [float(torch.tensor(v, dtype=torch.bfloat16)) for v in ZOE_STD[:C]]), ph, pw)
    images = F.pad(pixel_values, (pw, pw, ph, ph), mode=pad_mode)
    images = F.interpolate(images, size=(384, 384), mode="bicubic", align_corners=True)
    mean, std = _zoe_norm_consts(images.dtype, images.device)
    images = (images - mean) / std
    return images, ph, pw


@dataclass
class SpatialVLACausalLMOutputWithPast(ModelOutput):
    loss: Optional[torch.FloatTensor] = None
    logits: torch.FloatTensor = None
    past_key_values: Optional[Union[List[torch.FloatTensor], object]] = None
    hidden_states: Optional[Tuple[torch.FloatTensor]] = None
    attentions: Optional[Tuple[torch.FloatTensor]] = None
    image_hidden_states: Optional[torch.FloatTensor] = None


class SpatialVLAMultiModalProjector(nn.Module):
    def __init__(self, config: SpatialVLAConfig):
        super().__init__()
        self.linear = nn.Linear(config.vision_config.hidden_size, config.vision_config.projection_dim, bias=True)


class SpatialVLAPreTrainedModel(PreTrainedModel):
    config_class = SpatialVLAConfig
    base_model_prefix = "model"
    # gradient_checkpointing_enable / the training script's language_model._set_gradient_checkpointing(): the Gemma2
    # decoder layers re-run in the backward (Gemma2ForCausalLM._set_gradient_checkpointing); the vision tower's flag is
    # recorded only, as in the reference (spatialvla_pretrain.py:331 sets an attribute its encoder never reads)
    supports_gradient_checkpointing = True
    _no_split_modules = ["SpatialVLAMultiModalProjector", "ZoeDepthForDepthEstimation", "Ego3DPositionEmbeddingMLP"]

    def _init_weights(self, module):
        std = getattr(self.config, "initializer_range", None) or self.config.text_config.initializer_range
        if isinstance(module, (nn.Linear, nn.Conv2d)):
            module.weight.data.normal_(mean=0.0, std=std)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(mean=0.0, std=std)
            if module.padding_idx is not None:
                module.weight.data[module.padding_idx].zero_()


class SpatialVLAForConditionalGeneration(SpatialVLAPreTrainedModel, GenerationMixin):
    def __init__(self, config: SpatialVLAConfig, vision_model=None, vision_zoe_model=None, projector_model=None,
                 language_model=None):
        super().__init__(config)
        self.vision_tower = vision_model or SiglipVisionModel(config.vision_config)
        self.multi_modal_projector = projector_model or SpatialVLAMultiModalProjector(config)
        self.vocab_size = config.text_config.vocab_size
        self.language_model = language_model or Gemma2ForCausalLM(config.text_config)
        if config.use_vision_zoe:
            from transformers import ZoeDepthForDepthEstimation  # frozen 3p module tree; compute patched by zoe_fast
            self.vision_zoe_model = vision_zoe_model or ZoeDepthForDepthEstimation(config.vision_zoe_config)
            zoe_fast.install(self.vision_zoe_model)
            self.position_embedding_3d = Ego3DPositionEmbeddingMLP(
                config.ego3d_patch_reso ** 2 * 3, num_pos_feats=config.vision_config.hidden_size,
                n_freqs=config.n_freqs)
            patch_size, reso, image_size = (config.vision_config.patch_size, config.ego3d_patch_reso,
                                            config.vision_config.image_size)
            y, x = torch.meshgrid(torch.arange(0, image_size, patch_size // reso),
                                  torch.arange(0, image_size, patch_size // reso), indexing="ij")
            y, x = y + patch_size / reso / 2, x + patch_size / reso / 2
            uv_h = torch.stack([x, y, torch.ones_like(x)], dim=0).reshape(3, -1)
            self.register_buffer("uv_h", uv_h, persistent=False)
        if config.use_spatial_token:
            self.spatial_embed_tokens = nn.Embedding(config.spatial_token_num, config.text_config.hidden_size)
        else:
            self.spatial_embed_tokens = None
        self.pad_token_id = config.pad_token_id if config.pad_token_id is not None else -1
        # predict_action replays each decode step from a captured HIP graph (SVLA_DECODE_GRAPHS=0: eager launches)
        self.decode_graphs = os.environ.get("SVLA_DECODE_GRAPHS", "1") != "0"
        # reference raises on an image-token count mismatch inside the same forward (:379-385), and so does this
        # forward by default (one host read of the count).  defer_checks = True (opt-in: TrainEngine(...,
        # defer_host_checks=True), bench.py) copies the count to pinned host memory behind an event instead and
        # raises at the next forward / check_deferred(), so a training step never waits on the GPU.
        self.strict_checks = True
        self.defer_checks = False
        self._deferred = []
        # True (TrainEngine.train_step sets it around its own forward): a forward with labels and gradients runs the
        # lm_head over the rows that carry a label only and returns logits = None (LMHeadCEFn._forward_rows)
        self.head_label_rows = False
        self.last_stash = {}
        self.post_init()

    # ------------------------------------------------------------------ deferred host checks
    @staticmethod
    def _pinned_i64(dev):
        return torch.zeros(1, dtype=torch.int64, pin_memory=dev.type == "cuda")  # torch's caching host allocator

    def _defer(self, value, check):
        """check(v) on the device scalar `value`: at once (the reference's synchronous raise, default), or, with
        defer_checks, after copying it to pinned host memory behind an event at the next check_deferred().
        CPU tensors are always checked at once."""
        if value.device.type != "cuda" or not self.defer_checks:
            check(int(value))
            return
        buf = self._pinned_i64(value.device)
        buf.copy_(value.reshape(1).to(torch.int64), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._deferred.append((buf, ev, check))

    def check_deferred(self):
        """Run the pending host checks (waits for their events: recorded one forward earlier, long complete)."""
        pend, self._deferred = self._deferred, []
        for buf, ev, check in pend:
            ev.synchronize()
            check(int(buf[0]))

    # ------------------------------------------------------------------ reference accessors
    def get_input_embeddings(self):
        return self.language_model.get_input_embeddings()

    def set_input_embeddings(self, value):
        self.language_model.set_input_embeddings(value)

    def get_output_embeddings(self):
        return self.language_model.get_output_embeddings()

    def set_output_embeddings(self, new_embeddings):
        self.language_model.set_output_embeddings(new_embeddings)

    def get_decoder(self):
        return self.language_model.get_decoder()

    def set_decoder(self, decoder):
        self.language_model.set_decoder(decoder)

    def tie_weights(self, *args, **kwargs):
        return None  # SpatialVLA unties lm_head (spatialvla_pretrain.py:321-325)

    def _set_gradient_checkpointing(self, enable: bool = True, gradient_checkpointing_func=None):
        """gradient_checkpointing_enable() lands here: the Gemma2 layers recompute in the backward (see
        Gemma2ForCausalLM._set_gradient_checkpointing); the vision tower's flag is recorded only."""
        self.language_model._set_gradient_checkpointing(enable, gradient_checkpointing_func)
        self.vision_tower.gradient_checkpointing = bool(enable)

    # ------------------------------------------------------------------ image path
    @torch.no_grad()
    def predict_depth(self, pixel_values):
        """Zoe depth at image resolution (reference :314-323), frozen; the estimator's layers on libsvla (zoe_fast)."""
        zoe_pv, ph, pw = process_zoe(pixel_values, pad_mode="reflect")
        pvh, pvw = pixel_values.shape[-2:]
        depth = self.vision_zoe_model(pixel_values=zoe_pv).predicted_depth
        if depth.is_cuda and depth.dtype == torch.bfloat16:  # resize + crop in one kernel (svla_zoe_depth_resize)
            return K.zoe_depth_resize(depth.contiguous(), ph, (pvh, pvw))
        depth = F.interpolate(depth.unsqueeze(1), size=(pvh + 2 * ph, pvw + 2 * pw), mode="bicubic",
                              align_corners=True)[..., ph:-ph, pw:-pw]
        return depth.contiguous()

    @torch.no_grad()
    def ego3d_features(self, intrinsic, depth, kinv=None):
        """backproject_patch (:195-223) + frequency_encoding (:74-91) in one kernel -> [B*np, round8(F)]."""
        cfg = self.config
        B = depth.shape[0]
        np_ = (cfg.vision_config.image_size // cfg.vision_config.patch_size) ** 2
        nfeat = self.position_embedding_3d.freq_out_channels
        dt = self.multi_modal_projector.linear.weight.dtype
        feat = torch.empty(B * np_, K.round_up(nfeat, 8), dtype=dt, device=depth.device)
        if kinv is None:
            kinv = K.inv3x3(intrinsic)
        K.ego3d_encode(depth.float().contiguous(), kinv, self.uv_h.float().contiguous(),
                       cfg.vision_config.patch_size, cfg.ego3d_patch_reso, cfg.n_freqs, feat)
        return feat

    def backproject_patch(self, K_: torch.Tensor, depth: torch.Tensor, patch_size=14, reso=2) -> torch.Tensor:
        """Reference :195-223 — returns xyz [B, np, 3*reso^2] (fp32), computed by the HIP kernel."""
        B = depth.shape[0]
        np_ = (depth.shape[-2] // patch_size) * (depth.shape[-1] // patch_size)
        nfeat = 3 * reso * reso * (2 * self.config.n_freqs + 1)
        feat = torch.empty(B * np_, K.round_up(nfeat, 8), dtype=torch.bfloat16, device=depth.device)
        xyz = torch.empty(B, np_, 3 * reso * reso, dtype=torch.float32, device=depth.device)
        K.ego3d_encode(depth.float().contiguous(), K.inv3x3(K_),
                       self.uv_h.float().contiguous(), patch_size, reso, self.config.n_freqs, feat, xyz)
        return xyz

    def _wait_all_params(self):
        """ZeRO-1: land every parameter all-gather still in flight (TrainEngine leaves them to the next forward's
        wait points, which a replayed inference graph does not contain)."""
        wait_all = getattr(self, "_svla_param_wait_all", None)
        if wait_all is not None:
            wait_all()

    def _wait_params(self):
        pwait = getattr(self, "_svla_param_wait", None)  # ZeRO-1: embeddings / projector / Ego3D all-gathered
        if pwait is not None:
            pwait("pre")

    def get_image_features(self, pixel_values: torch.FloatTensor, intrinsic: torch.FloatTensor, kinv=None,
                           depth=None):
        """Reference :308-333 -> [B, np, H_text].  depth: a precomputed Zoe depth (predict_action computes it outside
        its prefill graph); None = predict it here."""
        self._wait_params()
        dt = self.multi_modal_projector.linear.weight.dtype
        pv = pixel_values.to(dt).contiguous()
        sig_in = torch.empty_like(pv)
        K.affine(pv, 1.0 / SIGLIP_STD[0], -SIGLIP_MEAN[0], sig_in)  # TF.normalize (:309)
        B = pv.shape[0]
        enc = None
        capturing = pv.is_cuda and torch.cuda.is_current_stream_capturing()
        if self.config.use_vision_zoe and depth is None and ZOE_STREAM[0] and pv.is_cuda and \
                (not capturing or ZOE_STREAM_CAPTURE[0]) and \
                Fn.side_stream(pv.device) != torch.cuda.current_stream(pv.device):
            # the frozen Zoe estimator and the Ego3D encoding (no autograd) on the side stream, beside the SigLIP
            # tower: two independent networks, each filling the CUs the other's kernel tails leave idle (also inside
            # the captured B=1 prefill graph: a fork / join of two branches)
            main = torch.cuda.current_stream(pv.device)
            side = Fn.side_stream(pv.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                enc = self.ego3d_features(intrinsic, self.predict_depth(pixel_values.to(dt)), kinv)
            feats = self.vision_tower(sig_in)                       # [B, np, Hv]
            main.wait_stream(side)
            if not capturing:  # (a captured graph's pool keeps its buffers alive for every replay)
                enc.record_stream(main)  # allocated on the side stream, read (and saved for backward) on this one
        else:
            feats = self.vision_tower(sig_in)                       # [B, np, Hv]
        Hv = feats.shape[-1]
        sel = feats.reshape(-1, Hv)
        if self.config.use_vision_zoe:
            if enc is None:
                if depth is None:
                    depth = self.predict_depth(pixel_values.to(dt))
                enc = self.ego3d_features(intrinsic, depth, kinv)  # kinv: precomputed outside a graph capture
            sel = self.position_embedding_3d.forward_residual(enc, sel)
        lin = self.multi_modal_projector.linear
        img = _linear(lin, sel, None, 1.0 / (self.config.text_config.hidden_size ** 0.5))
        return img.view(B, -1, img.shape[-1])

    # ------------------------------------------------------------------ forward
    def _merge_inputs(self, input_ids, image_features):
        self._wait_params()
        cfg = self.config
        B, Lq = input_ids.shape
        dev = input_ids.device
        embed_w = self.get_input_embeddings().weight
        if embed_w.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("training embed_tokens is not supported: freeze it as the reference does "
                                      "(freeze_llm_embed, spatialvla_pretrain.py:341-342)")
        ids = input_ids.reshape(-1).contiguous()
        img_index = None
        if image_features is not None:
            img_mask = ids == cfg.image_token_index
            n_img = image_features.shape[0] * image_features.shape[1]
            if self.strict_checks:
                def check(n_tok, n_img=n_img):
                    if n_tok != n_img:
                        raise ValueError(
                            "Number of images does not match number of special image tokens in the input text. "
                            f"Got {n_tok} image tokens in the text but {n_img} tokens from image embeddings.")
                self._defer(img_mask.sum(), check)
            # image rows beyond the features (a mismatch, reported by a deferred check) read the text embedding
            # instead of past the end of the feature rows
            idx = torch.cumsum(img_mask.to(torch.int32), 0) - 1
            img_index = torch.where(img_mask & (idx < n_img), idx, -1).to(torch.int32)
        ad = self._emb_adapter
        if (ad is not None and image_features is None and ids.numel() <= K.LORA_EMBED_DECODE_MAX_ROWS
                and not torch.is_grad_enabled() and self.lora_decode_emb_head and Fn.LORA_DECODE_KERNELS[0]
                and Fn.LORA_DECODE_EMB_HEAD_KERNELS[0] and ids.is_cuda):
            # a decode step under the Embedding adapter: nothing reads the CSR without a backward, and the merge and
            # the adapter rows are one launch (svla_lora_embed_decode)
            hidden = cfg.text_config.hidden_size
            out = torch.empty(ids.numel(), hidden, dtype=embed_w.dtype, device=dev)
            K.lora_embed_decode(ids, embed_w, self.spatial_embed_tokens.weight, int(cfg.action_token_begin_idx), ad.A,
                                ad.B, ad.r, ad.scaling, float(torch.tensor(hidden ** 0.5, dtype=embed_w.dtype)), out)
            return out.view(B, Lq, hidden)
        spatial_w, sort_rows, offsets, a0 = None, None, None, 0
        if cfg.use_spatial_token:
            spatial_w = self.spatial_embed_tokens.weight
            a0, na = int(cfg.action_token_begin_idx), spatial_w.shape[0]
            sel = (ids >= a0) & (ids < a0 + na)
            key = torch.where(sel, ids - a0, na)
            skey, order = torch.sort(key, stable=True)
            sort_rows = order.to(torch.int32)
            # CSR row offsets of each spatial-token id in the sorted order: a binary search instead of a
            # scatter_add histogram (every non-action token hits one bin: 0.11 ms of atomics at B=32)
            offsets = torch.searchsorted(skey, torch.arange(na + 1, dtype=skey.dtype, device=dev)).to(torch.int32)
        hidden = cfg.text_config.hidden_size
        normalizer = float(torch.tensor(hidden ** 0.5, dtype=embed_w.dtype))
        img2d = image_features.reshape(-1, image_features.shape[-1]) if image_features is not None else None
        ad = self._emb_adapter
        if ad is None:
            out = Fn.EmbedMergeFn.apply(ids, img_index, img2d, spatial_w, embed_w, a0, normalizer, sort_rows, offsets)
        else:  # add_lora("spatialvla-linear+emb"): the Embedding adapter on the spatial table
            out = Fn.EmbedMergeLoRAFn.apply(ids, img_index, img2d, spatial_w, embed_w, a0, normalizer, sort_rows,
                                            offsets, ad.scaling, ad.r, ad.A, ad.B)
        return out.view(B, Lq, hidden)

    def _merge_embeds(self, input_ids, inputs_embeds, image_features):
        """forward(inputs_embeds=...) (reference :361-387): the caller's embeddings instead of the table lookup, the
        spatial-token override (x * 0.0 + spatial row, quirk Q10) and the image-slot scatter keyed by input_ids, then
        the bf16 normalizer (modeling_gemma2.py:741-742).  Rare path: stock torch ops on the device, differentiable
        in inputs_embeds, the spatial table and the image features."""
        self._wait_params()
        cfg = self.config
        emb = inputs_embeds.to(self.multi_modal_projector.linear.weight.dtype).clone()
        if cfg.use_spatial_token and input_ids is not None:
            a0, na = int(cfg.action_token_begin_idx), int(cfg.spatial_token_num)
            sel = (input_ids >= a0) & (input_ids < a0 + na)
            sid = input_ids[sel] - a0
            rows = self.spatial_embed_tokens.weight[sid]
            ad = self._emb_adapter
            if ad is not None:  # the Embedding adapter's term, bf16(W[id] + bf16(s (B A)^T[id]))
                rows = rows + ((ad.A[:, sid].t().float() @ ad.B.t().float()) * ad.scaling).to(rows.dtype)
            emb[sel] = emb[sel] * 0.0 + rows
        if image_features is not None:
            m = (input_ids == cfg.image_token_index).unsqueeze(-1).expand_as(emb)
            if self.strict_checks:
                n_img = image_features.shape[0] * image_features.shape[1]

                def check(n_tok, n_img=n_img):
                    if n_tok != n_img:
                        raise ValueError(
                            "Number of images does not match number of special image tokens in the input text. "
                            f"Got {n_tok} image tokens in the text but {n_img} tokens from image embeddings.")
                self._defer((input_ids == cfg.image_token_index).sum(), check)
            emb = emb.masked_scatter(m, image_features.to(emb.dtype))
        normalizer = torch.tensor(cfg.text_config.hidden_size ** 0.5, dtype=emb.dtype, device=emb.device)
        return emb * normalizer

    def _label_rows(self, target):
        """Rows with a label, for the lm_head backward, without a host sync: the labelled rows first in order
        (stable sort of the validity flag) and their count copied to pinned memory behind an event recorded
        here -- the backward reads it after the whole forward, when the event has long completed."""
        valid = target >= 0
        order = torch.argsort((~valid).to(torch.int8), stable=True)
        if target.device.type != "cuda":
            return order, int(valid.sum()), None
        buf = self._pinned_i64(target.device)
        buf.copy_(valid.sum().reshape(1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return order, buf, ev

    @staticmethod
    def _targets(labels, attention_mask, B, Lq, dev, pad_mask=None):
        """Shifted CE targets per row (reference :415-430): target[b,t] = labels[b,t+1] where
        attention_mask[b,t+1] != 0 and label != -100, else -1 (ignored); last position ignored."""
        t = torch.full((B, Lq), -1, dtype=torch.int64, device=dev)
        if labels is None:
            return t.reshape(-1)
        sl = labels[:, 1:].clone()
        if attention_mask is not None:
            sl = torch.where(attention_mask[:, 1:] != 0, sl, -100)
        sl = torch.where(sl == -100, -1, sl)
        t[:, :-1] = sl
        return t.reshape(-1).contiguous()

    def forward(
        self,
        input_ids: torch.LongTensor = None,
        pixel_values: torch.FloatTensor = None,
        actions: Optional[torch.FloatTensor] = None,
        intrinsic: Optional[torch.Tensor] = None,
        attention_mask: Optional[torch.Tensor] = None,
        position_ids: Optional[torch.LongTensor] = None,
        past_key_values=None,
        token_type_ids: Optional[torch.LongTensor] = None,
        cache_position: Optional[torch.LongTensor] = None,
        inputs_embeds: Optional[torch.FloatTensor] = None,
        labels: Optional[torch.LongTensor] = None,
        use_cache: Optional[bool] = None,
        output_attentions: Optional[bool] = None,
        output_hidden_states: Optional[bool] = None,
        return_dict: Optional[bool] = None,
        num_logits_to_keep: int = 0,
        kv_mask: Optional[KVMask] = None,
    ) -> Union[Tuple, SpatialVLACausalLMOutputWithPast]:
        self.check_deferred()
        cache = past_key_values
        if cache is not None and not isinstance(cache, Gemma2KVCache):
            raise ValueError("past_key_values must be a Gemma2KVCache (see new_cache())")
        return_dict = True if return_dict is None else return_dict
        is_training = token_type_ids is not None and labels is not None  # reference :359
        if input_ids is None:
            if inputs_embeds is None:
                raise ValueError("forward needs input_ids (and optionally inputs_embeds)")
            if pixel_values is not None or self.config.use_spatial_token:
                # the reference reads input_ids for the image slots and the spatial tokens (:363-365, :376)
                raise ValueError("inputs_embeds without input_ids: the image and spatial-token merges need the ids")
        B, Lq = (input_ids if input_ids is not None else inputs_embeds).shape[:2]
        dev = (input_ids if input_ids is not None else inputs_embeds).device
        if cache is None and use_cache and not torch.is_grad_enabled():
            cache = self.new_cache(B, Lq + 256)
        if cache is not None:
            self._require_merged("forward(past_key_values=...)" if past_key_values is not None
                                 else "forward(use_cache=True) (it creates a KV cache)")

        if labels is not None and input_ids is not None:  # reference :390-395 (BC path), sync-free
            has_pad = (labels == self.pad_token_id).any()
            labels = torch.where(has_pad & (input_ids == self.pad_token_id), -100, labels)
        # the CE targets and the label-row plan depend on the batch alone: queued ahead of the vision tower, the
        # plan's row count has long reached the host when the head (head_label_rows) or the backward asks for it
        target = self._targets(labels, attention_mask, B, Lq, dev)
        stash = {}
        if labels is not None and torch.is_grad_enabled():
            stash["row_plan"] = self._label_rows(target)

        image_features = None
        if pixel_values is not None:
            image_features = self.get_image_features(pixel_values, intrinsic)

        if inputs_embeds is not None:
            hidden = self._merge_embeds(input_ids, inputs_embeds, image_features)
        else:
            hidden = self._merge_inputs(input_ids, image_features)
        past = cache.seen_tokens if cache is not None else 0
        if position_ids is None:
            start = past if cache_position is None else int(cache_position[0])
            position_ids = (torch.arange(start, start + Lq, device=dev) + 1)[None]  # 1-indexed (:372, :473-474)
        if kv_mask is not None:
            mask = kv_mask
        elif past == 0:
            mask = KVMask.build(attention_mask, token_type_ids, is_training, B, Lq, dev)
        else:
            # decode step: new tokens see the prompt and every earlier token (HybridCache path, :387-395);
            # attention_mask (if given) spans past + new tokens as in HF generate
            cls = torch.ones(B, Lq, dtype=torch.uint8, device=dev)
            if attention_mask is not None:
                cls = torch.where(attention_mask[:, -Lq:].to(dev) != 0, 1, 2).to(torch.uint8)
            mask = KVMask(cls.contiguous())
        attn_sink = [] if output_attentions else None
        h, all_h = self.language_model.model(hidden, mask, position_ids, output_hidden_states=bool(output_hidden_states),
                                             cache=cache, attn_sink=attn_sink)

        if self.head_label_rows and "row_plan" in stash:
            # the training step reads the loss alone: lm_head, softcap and statistics over the rows with a label
            # (LMHeadCEFn._forward_rows); no label in the batch: the full path
            order, cnt, ev = stash["row_plan"]
            if ev is not None:
                ev.synchronize()
                cnt = int(cnt[0])
            if cnt > 0:
                stash["label_rows"] = order[:cnt]
        logits2d, loss = self.language_model.head(h, target, stash, decode=past > 0)
        self.last_stash = stash
        logits = logits2d.view(B, Lq, -1) if logits2d is not None else None
        if num_logits_to_keep and logits is not None:
            logits = logits[:, -num_logits_to_keep:]
        if labels is None:
            loss = None
        if not return_dict:
            out = (logits,)
            return (loss,) + out if loss is not None else out
        return SpatialVLACausalLMOutputWithPast(loss=loss, logits=logits, past_key_values=cache, hidden_states=all_h,
                                                attentions=tuple(attn_sink) if attn_sink is not None else None,
                                                image_hidden_states=image_features)

    def action_argmax(self):
        """argmax over V of the last forward's logits [B*L] (int64), computed in the lm_head epilogue
        (train/monkey_patch.py:267 uses logits[..., :-1, :].argmax(-1))."""
        return self.last_stash.get("argmax")

    def action_token_ranges(self, action_tokenizer=None):
        """Inclusive token-id bounds (translation lo, hi, rotation lo, hi, gripper lo, hi) of the spatial action
        tokens: from `action_tokenizer` (or self.action_tokenizer, as train/monkey_patch.py:270-297 reads them) when
        given, else the canonical 4096 / 4096 / 2 split of the spatial_token_num tokens at action_token_begin_idx
        (scripts/action_config.json)."""
        at = action_tokenizer if action_tokenizer is not None else getattr(self, "action_tokenizer", None)
        if at is not None:
            return tuple(int(v) for t in (at.translation_tokenizer, at.rotation_tokenizer, at.gripper_tokenizer)
                         for v in (t.token_start_idx, t.token_end_idx))
        a0, n = int(self.config.action_token_begin_idx), int(self.config.spatial_token_num)
        if n != 8194:
            raise ValueError("action_token_ranges: pass the action tokenizer (non-canonical spatial_token_num)")
        return (a0, a0 + 4095, a0 + 4096, a0 + 8191, a0 + 8192, a0 + 8193)

    def action_metrics(self, labels: torch.Tensor, actions: Optional[torch.Tensor] = None, action_tokenizer=None,
                       argmax: Optional[torch.Tensor] = None):
        """The per-step metrics of the reference's compute_loss (train/monkey_patch.py:267-324) for the last
        training forward: accuracy, translation_accuracy, rotation_accuracy, gripper_accuracy as device fp32
        scalars, from the argmax the lm_head epilogue already produced (no [B, L, V] argmax pass, no host sync);
        with `actions` and an action tokenizer also l1_loss, decoded on the host as the reference does (:308-311)."""
        B, Lq = labels.shape
        am = argmax if argmax is not None else self.action_argmax()
        if am is None:
            raise ValueError("action_metrics: no argmax of a previous forward (run a training forward first)")
        am = am.view(B, -1)
        ranges = self.action_token_ranges(action_tokenizer)
        _counts, acc = K.action_accuracy(am, labels.contiguous(), ranges)
        out = {"accuracy": acc[0], "translation_accuracy": acc[1], "rotation_accuracy": acc[2],
               "gripper_accuracy": acc[3]}
        at = action_tokenizer if action_tokenizer is not None else getattr(self, "action_tokenizer", None)
        if actions is not None and at is not None:
            sl = labels[:, 1:]
            mask = (sl >= ranges[0]) & (sl <= ranges[5])
            pred_ids = am[:, :Lq - 1][mask].cpu().numpy().reshape(-1, 3)
            gt = actions.reshape(-1, 7).to(device="cpu", dtype=torch.float32)
            out["l1_loss"] = F.l1_loss(torch.tensor(at.decode_token_ids_to_actions(pred_ids)), gt)
        return out

    # ------------------------------------------------------------------ inference
    def new_cache(self, batch_size: int, capacity: int) -> Gemma2KVCache:
        """An empty KV cache for `capacity` tokens per sequence (prompt + generated)."""
        w = self.language_model.lm_head.weight
        return Gemma2KVCache(self.config.text_config, batch_size, capacity, w.device, w.dtype)

    def _prompt_classes(self, am, B, P, dev):
        if am is None:
            return torch.zeros(B, P, dtype=torch.uint8, device=dev)
        return torch.where(am.to(dev) != 0, 0, 2).to(torch.uint8).contiguous()

    def _next_token(self, h, finished, eos):
        """Greedy pick from the last position's logits (softcapped lm_head, argmax in its epilogue); sequences
        that already emitted eos get pad, as HF generate does for finished sequences."""
        B = h.shape[0]
        stash = {}
        tgt = torch.full((B,), -1, dtype=torch.int64, device=h.device)
        self.language_model.head(h[:, -1:].contiguous(), tgt, stash)
        nxt = stash["argmax"].view(B, 1)
        if eos is not None:
            nxt = torch.where(finished, torch.full_like(nxt, max(self.pad_token_id, 0)), nxt)
            finished = finished | (nxt == eos)
        return nxt, finished

    def _predict_inputs(self, model_inputs):
        dev = self.language_model.lm_head.weight.device
        ids = model_inputs["input_ids"].to(dev)
        pv = model_inputs.get("pixel_values")
        pv = pv.to(dev, torch.bfloat16) if pv is not None else None
        intr = model_inputs.get("intrinsic")
        intr = intr.to(dev, torch.bfloat16) if intr is not None else None
        return ids, pv, intr, model_inputs.get("attention_mask"), dev

    DECODE_STATES_MAX = 2      # decode states (KV cache + captured graphs) kept per model, least recently used out
    DECODE_CAPACITY_STEP = 64  # cache capacities are bucketed: prompts of nearby lengths share one state
    EOS_CHECK_EVERY = 8        # predict_action reads the device's finished flags once per this many decode steps

    def enable_fp8_projections(self, enabled: bool = True):
        """BASELINE configs[4]: the Gemma2 q|k|v, o, gate|up and down forward projections on the fp8 (OCP e4m3,
        row-scaled) MFMA GEMM, the attention and every backward GEMM unchanged (bf16).  Tolerances: tests/
        test_fp8_gpu.py; the captured prefill/decode graphs are dropped (the prefill changes)."""
        for layer in self.language_model.model.layers:
            layer.set_fp8_projections(enabled)  # off: also turns enable_fp8_lora off
        self.clear_decode_cache()

    @property
    def fp8_decode(self) -> bool:
        return bool(self.language_model.model.fp8_decode)

    def enable_fp8_decode(self, enabled: bool = True):
        """Weight-only MX fp8 decode (opt-in): the decode steps of predict_action, generate and
        forward(past_key_values=...) -- cache position > 0, at most 8 new token rows -- stream OCP MX e4m3 copies of the
        Gemma2 q|k|v, o, gate|up and down weights and of lm_head (svla_quant_mx_rows' values and exponents, dequantised
        in registers by svla_gemv_mxfp8 / svla_head_gemv_mxfp8) instead of the bf16 weights: half the bytes per token.
        Activations, the fp32 accumulation, norms, RoPE, attention, the KV cache and the softcap are unchanged, and the
        prefill keeps the bf16 weights (bitwise the prefill of a model without the switch).  The copies (about 2.6 GiB
        + 1/32 of that in exponents at 4B, beside the bf16 weights) are built by the first fp8 decode step and rebuilt
        when a weight moved, changed in place or the optimizer stepped; shapes the kernels refuse (more than 8 rows, a
        width that is no multiple of 128) keep the bf16 path.  Independent of enable_fp8_projections (the training
        step's fp8 GEMMs); with both on the decode steps take this path.  Not combined with LoRA adapters: refused while
        adapters are attached (merge_lora() first), and add_lora / load_lora are refused while it is on.  Toggling drops
        the captured decode states."""
        if enabled and (self.has_lora or self._emb_adapter is not None or self._head_adapter is not None):
            raise RuntimeError("enable_fp8_decode: LoRA adapters are attached: call merge_lora() first (the e4m3 decode "
                               "copies are made from the merged weights)")
        self.language_model.enable_fp8_decode(enabled)
        self.clear_decode_cache()

    @property
    def batched_decode(self) -> bool:
        return bool(self.language_model.batched_decode)

    def enable_batched_decode(self, enabled: bool = True):
        """Batched decode (opt-in, default off), for callers that step many sequences at once: the decode steps of
        predict_action, generate and forward(past_key_values=...) that add more than 8 token rows (batch x new tokens,
        functional.BATCHED_DECODE_MIN_ROWS..MAX_ROWS) run the Gemma2 q|k|v and o projections on svla_gemm_skinny,
        which streams each bf16 weight once into v_mfma_f32_16x16x32_bf16 fragments.  In these products a sequence's
        rows are bit-identical whatever the batch size and wherever the sequence sits in the batch.  Everything else
        in the step is unchanged, and functional.batched_decode_ok states which steps are excluded (each keeps the
        path it had).  Toggling drops the captured decode states."""
        self.language_model.enable_batched_decode(enabled)
        self.clear_decode_cache()

    SAMPLE_MAX_RANGES = 16     # capacity of a decode state's allowed-range table (allowed_ranges entries)

    @property
    def sampled_decode(self) -> bool:
        return bool(self.__dict__.get("_svla_sampled_decode", False))

    def enable_sampled_decode(self, on: bool = True):
        """Sampled decoding with log-probabilities (opt-in, default off): predict_action takes do_sample, temperature,
        top_k, top_p, seed, allowed_ranges and return_logprobs, and generate(do_sample=True) runs.  While on, every
        decode head is followed by svla_sample_rows (include/svla.h: allowed column range, top-k, top-p, Gumbel-max
        over Philox4x32-10, the token's log-probability under the sampled distribution and under the raw softmax),
        inside the captured prefill and step graphs; the settings live in a device block the host writes before the
        first replay, so one graph per cache position serves every setting and every call.  A row's noise is keyed by
        (seed, draw, cache position, sequence index): independent of the batch size and of the other rows.  Without
        do_sample the kernel runs its greedy form and the tokens are those of the switch-off path.  Works under
        enable_fp8_decode, enable_lora_decode (both forms), enable_fp8_lora_decode and enable_batched_decode: it only
        reads the logits they write.  Toggling drops the captured decode states."""
        self.__dict__["_svla_sampled_decode"] = bool(on)
        self.clear_decode_cache()

    def _sample_args(self, what, do_sample, temperature, top_k, top_p, seed, allowed_ranges, return_logprobs=False):
        """Validate a call's sampling arguments; returns None for a plain greedy call with the switch off, else the
        settings dict of _write_sample_params."""
        asked = (bool(do_sample) or return_logprobs or allowed_ranges is not None or seed is not None
                 or float(temperature) != 1.0 or int(top_k) != 0 or float(top_p) != 1.0)
        if not self.sampled_decode:
            if asked:
                raise RuntimeError(f"{what}: sampling arguments need enable_sampled_decode() (off by default)")
            return None
        if do_sample and not float(temperature) > 0:
            raise ValueError(f"{what}: `temperature` (={temperature}) has to be a strictly positive float with "
                             "do_sample=True; use do_sample=False for greedy decoding")
        if do_sample and not (int(top_k) >= 0 and float(top_p) > 0):
            raise ValueError(f"{what}: top_k must be >= 0 and top_p > 0")
        ranges = []
        if allowed_ranges is not None:
            ranges = [(int(lo), int(hi)) for lo, hi in allowed_ranges]
            V = self.language_model.lm_head.weight.shape[0]
            if not 1 <= len(ranges) <= self.SAMPLE_MAX_RANGES or any(not 0 <= lo < hi <= V for lo, hi in ranges):
                raise ValueError(f"{what}: allowed_ranges must be 1..{self.SAMPLE_MAX_RANGES} pairs 0 <= lo < hi <= {V}")
        if do_sample and seed is None:
            # a fresh seed per call from torch's default generator: torch.manual_seed makes a run of calls reproducible
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        # the kernel's draw counter stays 0 here: a call is determined by its seed alone (a counter kept by the model
        # would make a re-seeded run depend on the calls before it)
        return {"temperature": float(temperature) if do_sample else 0.0, "top_k": int(top_k) if do_sample else 0,
                "top_p": float(top_p) if do_sample else 1.0, "seed": int(seed or 0), "draw": 0, "ranges": ranges}

    @staticmethod
    def _sample_buffers(B, cap, dev, max_ranges):
        """The sampler's share of a decode state: the parameter block, the row ids (sequence index), the range table
        with the generated-token counter, the kernel's outputs and the log-probabilities at each cache position."""
        return {"params": torch.zeros(32, dtype=torch.uint8, device=dev),
                "rows": torch.arange(B, dtype=torch.int32, device=dev),
                "ranges": torch.zeros(max_ranges, 2, dtype=torch.int32, device=dev),
                "step": torch.zeros(1, dtype=torch.int64, device=dev),
                "lps": torch.zeros(2, B, cap + 1, dtype=torch.float32, device=dev)}

    @staticmethod
    def _write_sample_params(sb, sa):
        """Host -> device: the settings of one call (before the first graph replay) and the token counter's reset."""
        sa = sa or {"temperature": 0.0, "top_k": 0, "top_p": 1.0, "seed": 0, "draw": 0, "ranges": []}
        sb["params"].copy_(K.pack_sample_params(sa["temperature"], sa["top_p"], sa["top_k"], sa["seed"], sa["draw"],
                                                len(sa["ranges"])))
        if sa["ranges"]:
            sb["ranges"][:len(sa["ranges"])].copy_(torch.tensor(sa["ranges"], dtype=torch.int32))
        sb["step"].zero_()

    @staticmethod
    def _sample(sb, logits2d, position):
        """svla_sample_rows over a head's logits [B, V] -> (token [B], logprob [B], logprob_raw [B])."""
        return K.sample_rows(logits2d, logits2d.shape[1], sb["params"], position, sb["rows"], sb["ranges"],
                             sb["step"])[:3]

    def _refuse_lora_under_fp8_decode(self, what: str):
        if self.fp8_decode:
            raise RuntimeError(f"{what}: weight-only fp8 decode is on (enable_fp8_decode): call "
                               "enable_fp8_decode(False) first -- the e4m3 decode copies hold the base weights only")

    def _fp8_decode_key(self):
        """What the captured decode graphs bake in about the fp8 decode: None with the switch off, else the count of
        this model's copy (re)builds after making every copy current -- the graphs hold raw pointers into the copies.
        predict_action asks on every call, so the walk over the 4 x layers + 1 copies is skipped while a cheap stamp of
        the quantised weights (WEIGHT_EPOCH, their summed tensor versions and addresses) is what it was at the last
        walk; clear_decode_cache() forgets the stamp (a rebound parameter is a new tensor object)."""
        if not self.fp8_decode:
            return None
        return self._fp8_copies_key("_svla_fp8_decode", self.language_model.fp8_decode_holders)

    def _fp8_lora_decode_key(self):
        """_fp8_decode_key for the copies of enable_fp8_lora_decode: None with that switch off, else (True, the count
        of their (re)builds) after making every copy current."""
        if not self.fp8_lora_decode:
            return None
        return self._fp8_copies_key("_svla_fp8_lora_decode", self.language_model.fp8_lora_decode_holders)

    def _fp8_copies_key(self, attr, holders):
        lm = self.language_model
        memo = self.__dict__.get(attr + "_memo")
        if memo is not None and memo[1] == self._fp8_decode_stamp(memo[0], holders):
            return memo[2]
        with torch.no_grad():
            for layer in lm.model.layers:
                f8d, at, mlp = getattr(layer, attr), layer.self_attn, layer.mlp
                f8d.get("qkv", [at.q_proj.weight, at.k_proj.weight, at.v_proj.weight])
                f8d.get("o", [at.o_proj.weight])
                f8d.get("gate_up", [mlp.gate_proj.weight, mlp.up_proj.weight])
                f8d.get("down", [mlp.down_proj.weight])
            getattr(lm, attr + "_head").get("lm_head", [lm.lm_head.weight])
        key = (True, sum(h.builds for h in holders()))
        ws = [lin.weight for _, lin in self._lora_linears()] + [lm.lm_head.weight]
        self.__dict__[attr + "_memo"] = (ws, self._fp8_decode_stamp(ws, holders), key)
        return key

    def _fp8_decode_stamp(self, ws, holders=None):
        holders = (holders or self.language_model.fp8_decode_holders)()
        return (Fn.WEIGHT_EPOCH[0], sum(w._version for w in ws), sum(w.data_ptr() for w in ws),
                sum(h.builds for h in holders))

    @property
    def fp8_lora_decode(self) -> bool:
        return bool(self.language_model.model.fp8_lora_decode)

    def enable_fp8_lora_decode(self, enabled: bool = True):
        """Weight-only MX fp8 decode under unmerged LoRA adapters (opt-in, on top of enable_lora_decode): the decode
        steps of predict_action, generate and forward(past_key_values=...) -- cache position > 0, at most 8 new token
        rows -- stream OCP MX e4m3 copies of the frozen base q|k|v, o, gate|up and down weights and of lm_head, and the
        rank-r adapter term is added in bf16 inside the same GEMV: every projection is svla_lora_gemv_down (unchanged,
        bf16) + svla_lora_gemv_mxfp8, still 9 launches per layer; the head is svla_lora_head_gemv_mxfp8 under an
        lm_head adapter (enable_lora_decode(True, emb_head=True)) and svla_head_gemv_mxfp8 without one.  The base
        weights are frozen, so the copies (the 2.5 GiB of enable_fp8_decode, beside the bf16 weights) are made once, by
        the first call, and survive every optimizer step on A and B and every load_lora() of the same set and rank,
        which copies A and B in place; a base weight that moved or changed in place rebuilds its copy and drops the
        captured graphs.  The prefill, svla_lora_embed_decode and every other forward are untouched (the prefill is
        bitwise that of the model with the switch off); shapes either kernel family refuses, and
        SVLA_LORA_DECODE_KERNELS=0, keep the bf16 adapter path.  fp8_decode stays False (the holders are separate), so
        load_lora is not refused; enable_fp8_lora (the training step) is independent.  Needs adapters attached and
        enable_lora_decode() on, else RuntimeError before any state changes.  Turned off, and the copies freed, by
        enable_fp8_lora_decode(False), enable_lora_decode(False) and merge_lora().  Toggling drops the captured decode
        states."""
        if enabled and not self.has_lora:
            raise RuntimeError("enable_fp8_lora_decode: no adapters attached (add_lora() / load_lora() first); a merged "
                               "model streams its e4m3 weights through enable_fp8_decode()")
        if enabled and not self.lora_decode:
            raise RuntimeError("enable_fp8_lora_decode: the unmerged decode is off: call enable_lora_decode() first "
                               "(the e4m3 copies replace the base weights of its adapter GEMVs)")
        self.language_model.enable_fp8_lora_decode(enabled)
        self.clear_decode_cache()

    @property
    def fp8_lora(self) -> bool:
        return any(getattr(l.mlp, "_svla_fp8_lora", None) is not None for l in self.language_model.model.layers)

    def enable_fp8_lora(self, enabled: bool = True):
        """With LoRA adapters attached: the frozen base q|k|v, o, gate|up and down projections of the training /
        uncached forward on the MX fp8 GEMM, forward and input gradient (FP8_SITES / FP8_DGRAD as for
        enable_fp8_projections); the rank-r adapter products, the attention and the adapter gradients stay bf16.  The
        e4m3 copies (one W and one W^T per projection, beside the bf16 weights the decode and the merge read) are
        built by the first forward and kept across optimizer steps, which rewrite the adapters only.  The KV-cached
        forward (predict_action, generate, also under enable_lora_decode) stays on its bf16 path.  Turned off, and the
        copies freed, by enable_fp8_lora(False), enable_fp8_projections(False) and merge_lora().  The captured decode
        states are dropped.  With the "spatialvla-linear" set the vision side (SigLIP, projector, Ego3D) stays bf16."""
        if enabled and not self.has_lora:
            raise RuntimeError("enable_fp8_lora: no adapters attached (add_lora() / load_lora() first); a model "
                               "without adapters runs its projections in fp8 through enable_fp8_projections()")
        for layer in self.language_model.model.layers:
            layer.set_fp8_lora(enabled)
        self.clear_decode_cache()

    # ------------------------------------------------------------------ LoRA fine-tuning
    def _lora_linears(self):
        """[(module path, nn.Linear)] of the seven Gemma2 projections of every decoder layer, in layer order."""
        out = []
        for i, layer in enumerate(self.language_model.model.layers):
            for sub, names in (("self_attn", LORA_TARGETS[:4]), ("mlp", LORA_TARGETS[4:])):
                for n in names:
                    out.append((f"language_model.model.layers.{i}.{sub}.{n}", getattr(getattr(layer, sub), n)))
        return out

    def _lora_vision_linears(self):
        """[(module path, nn.Linear)] of the vision-side linears of the reference's default target set, in the order
        add_lora initialises them: per SigLIP encoder layer q, k, v, out_proj, fc1, fc2; the projector; Ego3D
        position_embedding_head.0 and .3 (when the model has the Ego3D branch)."""
        out = []
        for i, layer in enumerate(self.vision_tower.vision_model.encoder.layers):
            pre = f"vision_tower.vision_model.encoder.layers.{i}."
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                out.append((f"{pre}self_attn.{n}", getattr(layer.self_attn, n)))
            for n in ("fc1", "fc2"):
                out.append((f"{pre}mlp.{n}", getattr(layer.mlp, n)))
        out.append(("multi_modal_projector.linear", self.multi_modal_projector.linear))
        ego = getattr(self, "position_embedding_3d", None)
        if ego is not None:
            for n in (0, 3):
                out.append((f"position_embedding_3d.position_embedding_head.{n}", ego.position_embedding_head[n]))
        return out

    def _lora_all_linears(self, vision: Optional[bool] = None):
        """The Gemma2 projections, then (vision=True, or None = when the vision side carries adapters) the vision-side
        linears: the fixed module order of initialisation, merge and the adapter files."""
        if vision is None:
            vision = getattr(self.multi_modal_projector.linear, "lora", None) is not None
        return self._lora_linears() + (self._lora_vision_linears() if vision else [])

    @property
    def _emb_adapter(self):
        tab = self.spatial_embed_tokens
        return getattr(tab, "lora", None) if tab is not None else None

    @property
    def _head_adapter(self):
        return getattr(self.language_model.lm_head, "lora", None)

    @property
    def lora_modules_to_save(self) -> List[str]:
        """peft's modules_to_save of the attached recipe: [] or ["spatial_embed_tokens"] (the spatial table trained
        in full beside the adapters and stored in the adapter file)."""
        return [SPATIAL_TABLE] if self.__dict__.get("_svla_modules_to_save") else []

    @property
    def has_lora(self) -> bool:
        return any(getattr(lin, "lora", None) is not None for _, lin in self._lora_linears())

    @property
    def lora_targets(self) -> Optional[str]:
        """The attached target set: None, "gemma2-linear", "spatialvla-linear", "spatialvla-linear+emb" or
        "spatialvla-linear+emb+h"."""
        if not self.has_lora:
            return None
        if self._head_adapter is not None:
            return "spatialvla-linear+emb+h"
        if self._emb_adapter is not None:
            return "spatialvla-linear+emb"
        vis = getattr(self.multi_modal_projector.linear, "lora", None) is not None
        return "spatialvla-linear" if vis else "gemma2-linear"

    @property
    def lora_decode(self) -> bool:
        return bool(self.language_model.model.lora_decode)

    @property
    def lora_decode_emb_head(self) -> bool:
        """Whether the unmerged decode also permits an adapter on spatial_embed_tokens / lm_head
        (enable_lora_decode(True, emb_head=True))."""
        return bool(self.__dict__.get("_svla_lora_decode_emb_head", False))

    def enable_lora_decode(self, enabled: bool = True, emb_head: bool = False):
        """Run predict_action, generate, forward(past_key_values=...) and forward(use_cache=True) with unmerged LoRA
        adapters attached (mid-training evaluation, a base model with a swappable adapter from load_lora): the prefill
        on the training forward's rank-r kernels, every decode-step projection as svla_lora_gemv_down + svla_lora_gemv
        (9 launches per layer; DESIGN.md section 4 "LoRA").  Off (the default): those entry points refuse adapters and
        ask for merge_lora().  The captured graphs read A and B in place, so an optimizer step on them needs no
        re-capture; toggling the switch drops the decode states.  This path is bf16 whether or not enable_fp8_lora is on
        (enable_fp8_lora_decode puts the decode steps' base weights on e4m3 copies; turning this switch off clears it).
        With the "spatialvla-linear" set the prefill's SigLIP / Ego3D / projector run through their LoRA Functions under
        no_grad, inside the captured prefill graph; the decode steps never touch the vision side.  A modules_to_save
        spatial table needs nothing special (the graphs read the table in place).  With an adapter on
        spatial_embed_tokens or lm_head ("spatialvla-linear+emb", "+emb+h") the unmerged decode is a second opt-in:
        without emb_head=True turning the switch on raises NotImplementedError, before any state changes (merge_lora()
        first, or pass emb_head=True).  emb_head=True turns the switch on and permits those two adapters: the prefill
        keeps EmbedMergeLoRAFn / LMHeadCEFn under no_grad inside its graph, a decode step embeds its token with
        svla_lora_embed_decode and runs the head as svla_lora_gemv_down + svla_lora_head_gemv + svla_ce_finalize
        (DESIGN.md section 4 "LoRA on both ends"); the graphs read those A and B in place as well.
        enable_lora_decode(False) clears both."""
        permit = bool(enabled) and bool(emb_head)
        if enabled and not permit:
            self._refuse_emb_head_decode("enable_lora_decode", permitted=False)
        self.language_model.enable_lora_decode(enabled)
        if not enabled:
            self.language_model.enable_fp8_lora_decode(False)  # it rides on the adapter GEMVs of this switch
        self.__dict__["_svla_lora_decode_emb_head"] = permit
        self.clear_decode_cache()

    def _adapter_key(self):
        """What the captured decode graphs bake in about the adapters: the switch, the first adapter's storage, its
        rank and scaling, and the storage of the projector's adapter when the vision side carries adapters (the prefill
        graph runs SigLIP, Ego3D and the projector with theirs; they are attached and rebound together), then the
        storage of the Embedding adapter and of the lm_head adapter when attached (the step graphs read them) -- None
        without adapters."""
        ad = getattr(self.language_model.model.layers[0].self_attn.q_proj, "lora", None)
        if ad is None:
            return None
        key = (self.lora_decode, ad.A.data_ptr(), ad.r, ad.scaling)
        for extra in (getattr(self.multi_modal_projector.linear, "lora", None), self._emb_adapter, self._head_adapter):
            if extra is not None:
                key += (extra.A.data_ptr(),)
        return key

    def _refuse_emb_head_decode(self, what: str, permitted: Optional[bool] = None):
        if permitted is None:
            permitted = self.lora_decode_emb_head
        if not permitted and (self._emb_adapter is not None or self._head_adapter is not None):
            raise NotImplementedError(f"{what}: the KV-cached decode with an unmerged adapter on spatial_embed_tokens or "
                                      f"lm_head (the {self.lora_targets!r} set) is a separate opt-in: call merge_lora() "
                                      "first, or enable_lora_decode(True, emb_head=True) (forward without a cache and "
                                      "predict_action_uncached run unmerged)")

    def _require_merged(self, what: str):
        self._refuse_emb_head_decode(what)
        if self.has_lora and not self.lora_decode:
            raise RuntimeError(f"{what}: call merge_lora() first (unmerged LoRA adapters; the KV-cached decode "
                               "kernels read the base weights only)")

    @staticmethod
    def _modules_to_save_arg(modules_to_save, what: str) -> bool:
        """None, [] or "" -> False; "spatial_embed_tokens" (string or one-element list) -> True; else refused."""
        mts = modules_to_save
        if isinstance(mts, str):
            mts = [m for m in mts.split("+") if m]
        mts = list(mts or [])
        for m in mts:
            if m != SPATIAL_TABLE:
                raise NotImplementedError(f"{what}: modules_to_save={m!r} is not built (only {SPATIAL_TABLE!r}, the "
                                          "reference's --adapt_emb --adpt_feature recipe)")
        return bool(mts)

    def add_lora(self, r: int, lora_alpha: float, target_modules="gemma2-linear", init: str = "gaussian",
                 seed: Optional[int] = None, modules_to_save=None):
        """LoRA fine-tuning as the reference sets it up (train/spatialvla_finetune.py:262-302: LoraConfig(r,
        lora_alpha, target_modules, init_lora_weights="gaussian"), dropout 0, get_peft_model): A [r, in] ~ N(0, 1/r^2)
        (peft "gaussian": std 1/r) and B [out, r] = 0 in bf16 on every targeted nn.Linear, every other parameter
        frozen.  Targets: the seven Gemma2 projections of every decoder layer ("gemma2-linear", or exactly those seven
        names); the decoder layers then run Fn.GemmaAttentionLoRAFn / Fn.GemmaMLPLoRAFn.  "spatialvla-linear" (or
        exactly the reference's 13 names, LORA_TARGETS_FULL) is the reference's default lora_target="linear" as peft
        resolves it by name suffix: the Gemma2 projections plus q/k/v/out_proj/fc1/fc2 of every SigLIP encoder layer,
        multi_modal_projector.linear and both Ego3D linears (Fn.SiglipAttentionLoRAFn / SiglipMLPLoRAFn /
        LinearLoRAFn).  One CPU generator seeded with `seed` is walked in the order of _lora_all_linears(): the Gemma2
        projections layer by layer (q, k, v, o, gate, up, down), then per SigLIP layer q, k, v, out_proj, fc1, fc2,
        then the projector, then Ego3D head.0 and head.3 -- the Gemma2 adapters of both target sets are the same
        values under one seed.  Build the TrainEngine after this call: its flat buffers then hold the adapters only.

        "spatialvla-linear+emb" / "spatialvla-linear+emb+h" (or exactly the name lists of
        train/spatialvla_finetune.py:272-286) are the reference's lora_target="linear+emb" / "linear+emb+h": the 13
        names plus a peft Embedding adapter on spatial_embed_tokens (LoRAEmbeddingAdapter: lora_embedding_A [r, na],
        lora_embedding_B [H, r]; Fn.EmbedMergeLoRAFn), and with "+h" an ordinary adapter on language_model.lm_head
        (A ~ N(0, 1/r^2), B = 0; Fn.LMHeadCEFn adds bf16(s B (A h)) to the logits before the softcap).  The Embedding
        adapter is initialised as peft initialises embeddings whatever init_lora_weights says: A = 0, B ~ N(0, 1) --
        stated from memory of peft's reset_lora_parameters (peft is not a dependency and was not available to check
        against).  The generator walk continues after Ego3D: spatial_embed_tokens (B only draws), then lm_head (A only
        draws), so the 58 adapters of "spatialvla-linear" are the same bits under one seed in all three sets.

        modules_to_save: None, [] or ["spatial_embed_tokens"] (also the string): the reference's --adapt_emb
        --adpt_feature recipe, LoRA everywhere plus the spatial table trained in full (spatial_embed_tokens.weight
        keeps requires_grad=True; Fn.EmbedMergeFn's backward produces its gradient) and stored in the adapter file.
        Valid with any target set that does not itself adapt spatial_embed_tokens (both together: ValueError)."""
        self._refuse_lora_under_fp8_decode("add_lora")
        if not isinstance(r, int) or r % 8 != 0 or not 8 <= r <= 64:
            raise ValueError(f"add_lora: r must be a multiple of 8 in [8, 64], got {r!r}")
        if isinstance(target_modules, str):
            if target_modules not in LORA_SETS:
                raise NotImplementedError(f"add_lora: target_modules={target_modules!r}: 'gemma2-linear' (q_proj, "
                                          "k_proj, v_proj, o_proj, gate_proj, up_proj, down_proj of the Gemma2 decoder "
                                          "layers), 'spatialvla-linear' (those plus the SigLIP, projector and Ego3D "
                                          "linears: the set the reference's lora_target='linear' resolves to), "
                                          "'spatialvla-linear+emb' (plus spatial_embed_tokens) and "
                                          "'spatialvla-linear+emb+h' (plus lm_head) are built")
            targets = set(LORA_SETS[target_modules])
        else:
            targets = set(target_modules)
        for t in sorted(targets - set(LORA_TARGETS_EMB_H)):
            raise NotImplementedError(f"add_lora: target module {t!r} is not built (only {', '.join(LORA_TARGETS)} of "
                                      "the Gemma2 decoder layers, or the reference's 'linear', 'linear+emb' or "
                                      "'linear+emb+h' name lists)")
        emb, head = SPATIAL_TABLE in targets, "lm_head" in targets
        if (emb or head) and targets not in (set(LORA_TARGETS_EMB), set(LORA_TARGETS_EMB_H)):
            raise NotImplementedError(f"add_lora: {sorted(targets & {SPATIAL_TABLE, 'lm_head'})}: spatial_embed_tokens "
                                      "and lm_head are adapted only as the reference's 'linear+emb' / 'linear+emb+h' "
                                      "lists: pass 'spatialvla-linear+emb', 'spatialvla-linear+emb+h' or exactly those "
                                      "names")
        if emb and self.spatial_embed_tokens is None:
            raise ValueError("add_lora: the model has no spatial_embed_tokens (config.use_spatial_token is off)")
        save_table = self._modules_to_save_arg(modules_to_save, "add_lora")
        if save_table and emb:
            raise ValueError("add_lora: spatial_embed_tokens is both a LoRA target and in modules_to_save; train the "
                             "table in full (modules_to_save) or through its adapter, not both")
        if save_table and self.spatial_embed_tokens is None:
            raise ValueError("add_lora: modules_to_save names spatial_embed_tokens, which the model does not have")
        targets -= {SPATIAL_TABLE, "lm_head"}
        vision = bool(targets - set(LORA_TARGETS))
        if vision and targets != set(LORA_TARGETS_FULL):
            raise NotImplementedError(f"add_lora: {sorted(targets - set(LORA_TARGETS))}: the vision side (SigLIP, "
                                      "projector, Ego3D) is adapted as a whole, together with the Gemma2 projections: "
                                      "pass 'spatialvla-linear' or exactly the reference's 13 names; missing "
                                      f"{sorted(set(LORA_TARGETS_FULL) - targets)}")
        if not vision and targets != set(LORA_TARGETS):
            raise NotImplementedError("add_lora: the seven Gemma2 projections are adapted together; missing "
                                      f"{sorted(set(LORA_TARGETS) - targets)}")
        if init != "gaussian":
            raise NotImplementedError(f"add_lora: init={init!r} (the reference uses init_lora_weights='gaussian')")
        if self.has_lora:
            raise RuntimeError("add_lora: adapters are already attached (merge_lora() first)")
        if any(getattr(l.mlp, "_svla_fp8", None) is not None for l in self.language_model.model.layers):
            raise NotImplementedError("add_lora: enable_fp8_projections() is on; attach the adapters to the bf16 "
                                      "model, then enable_fp8_lora() runs the frozen base projections in fp8")
        gen = torch.Generator(device="cpu")
        if seed is not None:
            gen.manual_seed(int(seed))
        else:
            gen.seed()
        for p in self.parameters():
            p.requires_grad_(False)
        for _, lin in self._lora_all_linears(vision):
            w = lin.weight
            A = (torch.randn(r, w.shape[1], generator=gen) / r).to(torch.bfloat16).to(w.device)
            B = torch.zeros(w.shape[0], r, dtype=torch.bfloat16, device=w.device)
            lin.lora = LoRAAdapter(A, B, r, lora_alpha)
        if emb:  # peft's Embedding initialisation: A = 0, B ~ N(0, 1)
            w = self.spatial_embed_tokens.weight
            A = torch.zeros(r, w.shape[0], dtype=torch.bfloat16, device=w.device)
            B = torch.randn(w.shape[1], r, generator=gen).to(torch.bfloat16).to(w.device)
            self.spatial_embed_tokens.lora = LoRAEmbeddingAdapter(A, B, r, lora_alpha)
        if head:
            w = self.language_model.lm_head.weight
            A = (torch.randn(r, w.shape[1], generator=gen) / r).to(torch.bfloat16).to(w.device)
            B = torch.zeros(w.shape[0], r, dtype=torch.bfloat16, device=w.device)
            self.language_model.lm_head.lora = LoRAAdapter(A, B, r, lora_alpha)
        if save_table:
            self.spatial_embed_tokens.weight.requires_grad_(True)
        self.__dict__["_svla_modules_to_save"] = save_table
        self.clear_decode_cache()

    @torch.no_grad()
    def merge_lora(self):
        """peft's merge_and_unload: W <- bf16(W + bf16(s B A)) on every adapted linear, Gemma2 and vision side
        (svla_lora_up, summed mode, C = W, T = B), then the adapters are removed and every layer runs its original
        Functions again.  The lm_head adapter folds the same way (M = V rows); the Embedding adapter folds
        W_sp[id, :] += s (B A)^T[id, :] through small transposed temporaries (C = W_sp, T = A^T [na, r], S = B^T
        [r, H]).  A modules_to_save table simply stays as the weight; the flag is cleared and the table frozen like the
        rest.  Irreversible."""
        if not self.has_lora:
            raise RuntimeError("merge_lora: no adapters attached")
        self.enable_fp8_lora(False)  # the e4m3 copies are of the unmerged base weights: the merge reads bf16
        self.language_model.enable_fp8_lora_decode(False)  # and so are the decode copies
        for _, lin in self._lora_all_linears():
            ad = lin.lora
            w = lin.weight.data
            if w.dtype != torch.bfloat16 or not w.is_cuda:
                raise RuntimeError("merge_lora runs on the GPU kernels: move the model to the GPU in bf16 first")
            if w.shape[1] % 8 != 0:  # Ego3D head.0 (204 columns): svla_lora_up needs N % 8 == 0 -- a padded temporary
                Kp = K.round_up(w.shape[1], 8)
                wp = torch.zeros(w.shape[0], Kp, dtype=w.dtype, device=w.device)
                wp[:, :w.shape[1]] = w
                Ap = torch.zeros(ad.r, Kp, dtype=w.dtype, device=w.device)
                Ap[:, :w.shape[1]] = ad.A.data
                K.lora_up(wp, ad.B.data, [Ap], ad.r, summed=True, alpha=ad.scaling)
                w.copy_(wp[:, :w.shape[1]])
            else:
                K.lora_up(w, ad.B.data, [ad.A.data], ad.r, summed=True, alpha=ad.scaling)
            del lin.lora
        ad = self._emb_adapter
        if ad is not None:
            w = self.spatial_embed_tokens.weight.data
            if w.dtype != torch.bfloat16 or not w.is_cuda:
                raise RuntimeError("merge_lora runs on the GPU kernels: move the model to the GPU in bf16 first")
            K.lora_up(w, ad.A.data.t().contiguous(), [ad.B.data.t().contiguous()], ad.r, summed=True, alpha=ad.scaling)
            del self.spatial_embed_tokens.lora
        ad = self._head_adapter
        if ad is not None:
            K.lora_up(self.language_model.lm_head.weight.data, ad.B.data, [ad.A.data], ad.r, summed=True,
                      alpha=ad.scaling)
            del self.language_model.lm_head.lora
        if self.__dict__.get("_svla_modules_to_save"):
            self.spatial_embed_tokens.weight.requires_grad_(False)
            self.__dict__["_svla_modules_to_save"] = False
        Fn.WEIGHT_EPOCH[0] += 1
        self.clear_decode_cache()

    def save_lora(self, save_directory: str):
        """The adapters in peft's on-disk layout: adapter_model.safetensors with keys
        base_model.model.<module path>.lora_A.weight / .lora_B.weight and adapter_config.json; every attached adapter,
        module paths as in the reference's module tree (target_modules lists the reference's names for the attached
        set).  The Embedding adapter is base_model.model.spatial_embed_tokens.lora_embedding_A / .lora_embedding_B (no
        ".weight"), the lm_head adapter base_model.model.language_model.lm_head.lora_A.weight / .lora_B.weight, and a
        modules_to_save table base_model.model.spatial_embed_tokens.weight (peft strips "modules_to_save." and the
        adapter name when it saves -- stated from memory of peft, which is not a dependency; load_lora accepts the
        unstripped spellings too)."""
        import json
        from safetensors.torch import save_file
        if not self.has_lora:
            raise RuntimeError("save_lora: no adapters attached")
        os.makedirs(save_directory, exist_ok=True)
        tensors, ad = {}, None
        for path, lin in self._lora_all_linears() + ([("language_model.lm_head", self.language_model.lm_head)]
                                                      if self._head_adapter is not None else []):
            ad = lin.lora
            tensors[f"base_model.model.{path}.lora_A.weight"] = ad.A.detach().to("cpu").contiguous()
            tensors[f"base_model.model.{path}.lora_B.weight"] = ad.B.detach().to("cpu").contiguous()
        emb = self._emb_adapter
        if emb is not None:
            tensors[f"base_model.model.{SPATIAL_TABLE}.lora_embedding_A"] = emb.A.detach().to("cpu").contiguous()
            tensors[f"base_model.model.{SPATIAL_TABLE}.lora_embedding_B"] = emb.B.detach().to("cpu").contiguous()
        mts = self.lora_modules_to_save
        if mts:
            tensors[f"base_model.model.{SPATIAL_TABLE}.weight"] = \
                self.spatial_embed_tokens.weight.detach().to("cpu").contiguous()
        save_file(tensors, os.path.join(save_directory, "adapter_model.safetensors"), metadata={"format": "pt"})
        cfg = {"peft_type": "LORA", "r": ad.r, "lora_alpha": ad.lora_alpha,
               "target_modules": list(LORA_SETS[self.lora_targets]),
               "init_lora_weights": "gaussian", "lora_dropout": 0.0, "bias": "none", "fan_in_fan_out": False,
               "modules_to_save": mts or None, "inference_mode": True, "task_type": None}
        with open(os.path.join(save_directory, "adapter_config.json"), "w") as f:
            json.dump(cfg, f, indent=2, sort_keys=True)

    def load_lora(self, load_directory: str):
        """Attach the adapters of a save_lora() / peft directory: a file holding exactly one of the four sets --
        the Gemma2 set ("gemma2-linear"), the full set of the reference's default recipe ("spatialvla-linear": Gemma2,
        SigLIP, projector, Ego3D), that plus the spatial_embed_tokens Embedding adapter ("spatialvla-linear+emb"), or
        that plus the lm_head adapter ("spatialvla-linear+emb+h") -- with or without a modules_to_save spatial table
        (base_model.model.spatial_embed_tokens.weight, or peft's unstripped .modules_to_save.weight /
        .modules_to_save.default.weight); whichever it holds is attached.  Raises, listing the keys, for adapters of
        other modules, any other subset, or ranks that differ between modules; the model is then left as it was."""
        import json
        import re
        from safetensors.torch import load_file
        self._refuse_lora_under_fp8_decode("load_lora")
        with open(os.path.join(load_directory, "adapter_config.json")) as f:
            cfg = json.load(f)
        if cfg.get("peft_type", "LORA") != "LORA":
            raise NotImplementedError(f"load_lora: peft_type {cfg.get('peft_type')!r}")
        cfg_table = self._modules_to_save_arg(cfg.get("modules_to_save"), "load_lora")
        if float(cfg.get("lora_dropout") or 0.0) != 0.0:
            raise NotImplementedError("load_lora: lora_dropout != 0 is not built")
        tensors = load_file(os.path.join(load_directory, "adapter_model.safetensors"))
        gemma, vis = dict(self._lora_linears()), dict(self._lora_vision_linears())
        head_path = "language_model.lm_head"
        mine = {**gemma, **vis, head_path: self.language_model.lm_head}
        found, foreign, table = {}, [], None
        for k, v in tensors.items():
            m = re.match(r"^base_model\.model\.(.+)\.lora_([AB])(?:\.default)?\.weight$", k)
            if m is not None and m.group(1) in mine:
                found.setdefault(m.group(1), {})[m.group(2)] = v
                continue
            m = re.match(rf"^base_model\.model\.{SPATIAL_TABLE}\.lora_embedding_([AB])(?:\.default)?$", k)
            if m is not None and self.spatial_embed_tokens is not None:
                found.setdefault(SPATIAL_TABLE, {})[m.group(1)] = v
                continue
            if self.spatial_embed_tokens is not None and re.match(
                    rf"^base_model\.model\.{SPATIAL_TABLE}(?:\.modules_to_save(?:\.default)?)?\.weight$", k):
                if table is not None:
                    foreign.append(k)  # the table twice under two spellings
                table = v
                continue
            foreign.append(k)
        if foreign:
            raise ValueError("load_lora: adapters for modules outside the Gemma2 q/k/v/o/gate/up/down projections, the "
                             "SigLIP / projector / Ego3D linears, spatial_embed_tokens (lora_embedding_A/B) and lm_head "
                             f"(or unknown keys) are not built: {sorted(foreign)}")
        emb, head = SPATIAL_TABLE in found, head_path in found
        full = any(p in vis for p in found) or emb or head
        want = ("spatialvla-linear+emb+h" if head else "spatialvla-linear+emb" if emb else
                "spatialvla-linear" if full else "gemma2-linear")
        lin_paths = dict(gemma)
        if full:
            lin_paths.update(vis)
        if head:
            lin_paths[head_path] = self.language_model.lm_head
        need = list(lin_paths) + ([SPATIAL_TABLE] if emb or head else [])
        missing = [p for p in need if set(found.get(p, {})) != {"A", "B"}]
        if missing:
            have = sorted(k for k in tensors if ".lora_" in k)
            names = [m + (".lora_embedding_A" if m == SPATIAL_TABLE else ".lora_A.weight") for m in missing]
            raise ValueError("load_lora: the file must hold exactly the Gemma2 set, the full set (Gemma2, SigLIP, "
                             "projector, Ego3D), the full set with spatial_embed_tokens, or that with lm_head; no "
                             f"complete adapter for {names}; the file holds {have}")
        if emb and (table is not None or cfg_table):
            raise ValueError("load_lora: spatial_embed_tokens is both adapted (lora_embedding_A/B) and saved in full "
                             f"(modules_to_save); the file holds {sorted(tensors)}")
        if cfg_table != (table is not None):
            raise ValueError(f"load_lora: adapter_config.json says modules_to_save={cfg.get('modules_to_save')!r} but "
                             f"the file {'holds' if table is not None else 'does not hold'} a spatial_embed_tokens "
                             f"table; keys: {sorted(k for k in tensors if '.lora_' not in k)}")
        ranks = {p: int(ab["A"].shape[0]) for p, ab in found.items()}
        if len(set(ranks.values())) != 1:
            raise ValueError("load_lora: ranks differ between modules: "
                             f"{ {k + ('.lora_embedding_A' if k == SPATIAL_TABLE else '.lora_A.weight'): r for k, r in sorted(ranks.items())} }")
        r = next(iter(ranks.values()))
        for p, lin in lin_paths.items():
            a, b = found[p]["A"], found[p]["B"]
            if tuple(a.shape) != (r, lin.weight.shape[1]) or tuple(b.shape) != (lin.weight.shape[0], r):
                raise ValueError(f"load_lora: {p}: shapes {tuple(a.shape)} / {tuple(b.shape)} do not fit the projection")
        if emb:
            w = self.spatial_embed_tokens.weight
            a, b = found[SPATIAL_TABLE]["A"], found[SPATIAL_TABLE]["B"]
            if tuple(a.shape) != (r, w.shape[0]) or tuple(b.shape) != (w.shape[1], r):
                raise ValueError(f"load_lora: {SPATIAL_TABLE}: shapes {tuple(a.shape)} / {tuple(b.shape)} do not fit "
                                 "the table")
        if table is not None and tuple(table.shape) != tuple(self.spatial_embed_tokens.weight.shape):
            raise ValueError(f"load_lora: {SPATIAL_TABLE}.weight: shape {tuple(table.shape)} does not fit the table")
        if not self.has_lora:
            self.add_lora(r, cfg.get("lora_alpha", r), target_modules=want, seed=0,
                          modules_to_save=[SPATIAL_TABLE] if table is not None else None)
        elif self.lora_targets != want or bool(self.lora_modules_to_save) != (table is not None):
            raise ValueError(f"load_lora: the file holds the {want!r} set"
                             f"{' with' if table is not None else ' without'} a modules_to_save table, the attached "
                             f"adapters are {self.lora_targets!r} with modules_to_save={self.lora_modules_to_save} "
                             "(merge_lora() first, or load into a fresh model)")
        pairs = [(lin.lora, found[p]) for p, lin in lin_paths.items()]
        if emb:
            pairs.append((self.spatial_embed_tokens.lora, found[SPATIAL_TABLE]))
        with torch.no_grad():
            for ad, ab in pairs:
                if ad.r != r:
                    raise ValueError(f"load_lora: attached adapters have rank {ad.r}, the file has {r}")
                ad.lora_alpha = float(cfg.get("lora_alpha", r))
                ad.scaling = ad.lora_alpha / r
                ad.A.copy_(ab["A"].to(ad.A.dtype))
                ad.B.copy_(ab["B"].to(ad.B.dtype))
            if table is not None:
                self.spatial_embed_tokens.weight.copy_(table.to(self.spatial_embed_tokens.weight.dtype))
        self.clear_decode_cache()

    def clear_decode_cache(self):
        """Drop every persistent decode state (KV caches, captured prefill/decode graphs and their memory pool).
        The graphs hold raw pointers to the weights they were captured with, so anything that rebinds parameter
        storage (TrainEngine's flat buffers, load_state_dict with assign, .to()) must call this."""
        self.__dict__["_svla_decode_states"] = {}
        self.__dict__.pop("_svla_fp8_decode_memo", None)
        self.__dict__.pop("_svla_fp8_lora_decode_memo", None)

    @staticmethod
    def _prompt_positions(valid: torch.Tensor) -> torch.Tensor:
        """Per-sequence positions of a (possibly padded) prompt, as the reference's generate derives them:
        attention_mask.cumsum(-1) - 1, pads set to 1 (modeling_gemma2.py:1039-1042), then + 1
        (modeling_spatialvla.py:473-474).  valid: bool [B, L]."""
        pos = valid.to(torch.int64).cumsum(-1) - 1
        return pos.masked_fill(~valid, 1) + 1

    def _decode_state(self, B: int, capacity: int, dev):
        """Persistent decode state per (batch, bucketed capacity): the KV cache, the static token buffer the captured
        graphs read, the graphs themselves keyed by cache position (one private memory pool shared by all of a
        state's graphs), and one side stream for their eager warm-ups.  Reused across predict_action calls, so a
        control loop replays the same graphs every call; at most DECODE_STATES_MAX states are kept (LRU)."""
        from collections import OrderedDict
        states = self.__dict__.get("_svla_decode_states")
        if not isinstance(states, OrderedDict):
            states = self.__dict__["_svla_decode_states"] = OrderedDict()
        cap = -(-capacity // self.DECODE_CAPACITY_STEP) * self.DECODE_CAPACITY_STEP
        key = (B, cap, str(dev))
        st = states.get(key)
        # the graphs hold raw pointers: to the weights (rebound by TrainEngine) and, with fp8 projections, to the
        # e4m3 weight copies, which the next eager forward after an optimizer step (WEIGHT_EPOCH) frees and rebuilds
        fp8 = any(getattr(l.mlp, "_svla_fp8", None) is not None for l in self.language_model.model.layers)
        # ... and to the LoRA adapters (rebound by TrainEngine / load_lora), with the path the switch selects
        # ... and, with the weight-only fp8 decode (alone or under adapters), to its e4m3 copies: the switch and the
        # copies' identity
        wptr = (self.language_model.lm_head.weight.data_ptr(), Fn.WEIGHT_EPOCH[0] if fp8 else -1, self._adapter_key(),
                self._fp8_decode_key(), self._fp8_lora_decode_key())
        if self.batched_decode:  # ... and the batched-decode switch selects other kernels: a sixth element while on
            wptr += ("batched",)
        if self.sampled_decode:  # ... and the sampler follows every head: graphs with and without it are never mixed
            wptr += ("sampled",)
        if st is not None and st["wptr"] != wptr:  # weights were rebound since capture: the graphs are stale
            states.pop(key)
            st = None
        if st is None:
            while len(states) >= self.DECODE_STATES_MAX:
                states.popitem(last=False)
            st = {"cache": self.new_cache(B, cap), "graphs": {}, "prefill": {}, "wptr": wptr,
                  "tok": torch.zeros(B, 1, dtype=torch.int64, device=dev),
                  # greedy bookkeeping read / written inside the step graphs: finished rows, eos / pad ids (-1 = no
                  # eos), every generated token at its cache position
                  "fin": torch.zeros(B, 1, dtype=torch.bool, device=dev),
                  "eos": torch.full((1, 1), -1, dtype=torch.int64, device=dev),
                  "pad": torch.zeros(1, 1, dtype=torch.int64, device=dev),
                  "toks": torch.zeros(B, cap + 1, dtype=torch.int64, device=dev),
                  "npad": torch.zeros(B, 1, dtype=torch.int64, device=dev),  # pads in each prompt (static input)
                  "cls": KVMask(torch.ones(B, 1, dtype=torch.uint8, device=dev)),
                  "pool": torch.cuda.graph_pool_handle() if dev.type == "cuda" else None,
                  "side": torch.cuda.Stream(device=dev) if dev.type == "cuda" else None}
            if self.sampled_decode:
                st["sample"] = self._sample_buffers(B, cap, dev, self.SAMPLE_MAX_RANGES)
            states[key] = st
        states.move_to_end(key)
        return st

    def _prefill_body(self, st, x):
        """Vision tower + Ego3D/Zoe + Gemma2 prefill over the prompt (filling the cache) + the first greedy token."""
        ids, cache = x["ids"], st["cache"]
        feats = (self.get_image_features(x["pv"], x["intr"], x["kinv"], x.get("depth")) if x["pv"] is not None
                 else None)
        pos = self._prompt_positions(x["cls"] != 2)  # per-sequence positions of a padded batch (1..P unpadded)
        strict, self.strict_checks = self.strict_checks, False  # checked on the host by predict_action
        try:
            hidden = self._merge_inputs(ids, feats)
        finally:
            self.strict_checks = strict
        h, _ = self.language_model.model(hidden, KVMask(x["cls"]), pos, cache=cache)
        stash = {}
        tgt = torch.full((ids.shape[0],), -1, dtype=torch.int64, device=ids.device)
        logits, _ = self.language_model.head(h[:, -1:].contiguous(), tgt, stash)
        if "sample" in st:  # the first token, stored at cache position P
            return self._sample(st["sample"], logits, ids.shape[1])
        return stash["argmax"]

    def _prefill_graph(self, st, x):
        """The prefill as one HIP graph per (prompt length, with/without image): ~2000 launches (SigLIP, the frozen
        Zoe forward, 26 Gemma2 layers) whose host cost at B=1 rivals their GPU time.  Inputs are copied into the
        graph's static buffers; shapes, the cache and the positions are baked in."""
        cache = st["cache"]
        key = (x["ids"].shape[1], x["pv"] is not None)
        if key in st["prefill"] and st["prefill"][key] is None:
            return self._prefill_body(st, x)
        g = st["prefill"].get(key)
        if g is None:
            static = {k: (v.clone() if v is not None else None) for k, v in x.items()}
            side = st["side"]
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # eager warm-up: lazy kernel attributes, GEMM workspaces, Zoe caches
                self._prefill_body(st, static)
            cache.seen_tokens = 0
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            try:
                # captured on the warm-up stream, where the eager warm-up ran (lazy kernel attributes, weight caches)
                with torch.cuda.graph(graph, pool=st["pool"], stream=side):
                    out = self._prefill_body(st, static)
            except RuntimeError as e:  # an op of the prefill cannot be captured: run this shape eagerly from now on
                cache.seen_tokens = 0
                torch.cuda.synchronize()
                st["prefill"][key] = None
                import traceback
                where = [f"{fr.filename.split('/')[-1]}:{fr.lineno} {fr.name}" for fr in traceback.extract_tb(e.__traceback__)]
                warnings.warn(f"prefill graph capture failed at {' <- '.join(reversed(where[-6:]))}: "
                              f"{str(e).splitlines()[0]}; prefill runs eagerly")
                return self._prefill_body(st, x)
            cache.seen_tokens = 0
            g = st["prefill"][key] = (graph, static, out)
        graph, static, out = g
        for k, v in x.items():
            if v is not None:
                static[k].copy_(v)
        graph.replay()
        return out

    def _decode_body(self, st, p0):
        """One decode step at cache position p0: the token in st["tok"] -> argmax of its logits [B]."""
        tok, cache = st["tok"], st["cache"]
        # 1-indexed (:372, :473-474); a sequence with n pads in its prompt is n positions behind its cache row
        pos = (p0 + 1) - st["npad"]
        h, _ = self.language_model.model(self._merge_inputs(tok, None), st["cls"], pos, cache=cache)
        stash = {}
        tgt = torch.full((tok.shape[0],), -1, dtype=torch.int64, device=tok.device)
        logits, _ = self.language_model.head(h[:, -1:].contiguous(), tgt, stash, decode=True)
        if "sample" in st:  # the token stored at cache position p0 + 1
            return self._sample(st["sample"], logits, p0 + 1)
        return stash["argmax"]

    def _greedy_bookkeep(self, st, p0, am):
        """The greedy loop's per-token update on the device (so a run of steps needs no host round trip): rows that
        already emitted eos get pad, newly finished rows are marked, the token is fed to the next step and kept at
        its cache position p0 + 1 (reference generate: unfinished_sequences / pad_token_id handling).  With the
        sampler on, `am` is its (token, logprob, logprob_raw): the log-probabilities are kept at the same position
        (0 for the pads of finished rows) and the generated-token counter advances."""
        if "sample" in st:
            am, lp, lpr = am
            sb = st["sample"]
            sb["lps"][:, :, p0 + 1].copy_(torch.where(st["fin"].view(1, -1), 0.0, torch.stack((lp, lpr))))
            sb["step"].add_(1)
        nxt = torch.where(st["fin"], st["pad"], am.view(-1, 1))
        st["fin"].logical_or_(nxt == st["eos"])
        st["tok"].copy_(nxt)
        st["toks"][:, p0 + 1:p0 + 2].copy_(nxt)

    def _decode_step_graph(self, st, p0):
        """The decode step as a HIP graph (torch.cuda.CUDAGraph on ROCm), captured once per cache position: a
        B=1 step is ~300 small launches whose host-side cost exceeds their GPU time, and a graph replays them
        as one submission.  Positions, cache rows and sequence lengths are baked into each graph."""
        cache = st["cache"]
        g = st["graphs"].get(p0)
        if g is None:
            side = st["side"]
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # eager warm-up (lazy kernel attributes); rewrites row p0 identically
                saved = (st["tok"].clone(), st["fin"].clone())
                step = st["sample"]["step"].clone() if "sample" in st else None
                self._greedy_bookkeep(st, p0, self._decode_body(st, p0))
                st["tok"].copy_(saved[0])
                st["fin"].copy_(saved[1])
                if step is not None:
                    st["sample"]["step"].copy_(step)
            cache.seen_tokens = p0
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, pool=st["pool"], stream=side):  # on the warm-up stream, as the prefill
                out = self._decode_body(st, p0)
                self._greedy_bookkeep(st, p0, out)
            cache.seen_tokens = p0
            g = st["graphs"][p0] = (graph, out)
        g[0].replay()
        cache.seen_tokens = p0 + 1
        return g[1]

    @torch.no_grad()
    def predict_action(self, model_inputs, max_new_tokens: int = 256, eos_token_id: Optional[int] = None,
                       do_sample: bool = False, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                       seed: Optional[int] = None, allowed_ranges=None, return_logprobs: bool = False):
        """Greedy decode with a KV cache (reference :484-492 -> generate(max_new_tokens=256, do_sample=False)
        with HybridCache).  Prefill: the prompt (image features merged, positions 1..P) attends bidirectionally
        (:294) and fills the cache; decode: one token per step at position P+i+1 (:473-474), no pixel values
        after step 0 (:475-476), attending to the prompt and every earlier generated token.  Stops when every
        sequence has emitted eos or after max_new_tokens.

        With enable_sampled_decode() (the arguments below raise without it): do_sample draws every token by
        svla_sample_rows under temperature / top_k (0 = off) / top_p (1 = off), HF generate's warpers; seed: an
        explicit seed makes the call reproducible on its own, None takes a fresh one per call from torch's default
        generator (so torch.manual_seed makes a run of calls reproducible).  allowed_ranges: (lo, hi) token-id pairs
        applied cyclically to the generated-token index (SpatialVLAProcessor.action_token_ranges(): translation,
        rotation, gripper), also for greedy calls; eos is then never allowed, so the loop runs max_new_tokens steps --
        pass three times the number of actions.  return_logprobs: the result is (tokens, logprobs [B, n] fp32 under the
        distribution sampled from, logprobs_raw [B, n] fp32 under the unconstrained softmax at temperature 1)."""
        self._require_merged("predict_action")
        self._wait_all_params()
        sa = self._sample_args("predict_action", do_sample, temperature, top_k, top_p, seed, allowed_ranges,
                               return_logprobs)
        ids, pv, intr, am, dev = self._predict_inputs(model_inputs)
        eos = eos_token_id if eos_token_id is not None else self.config.text_config.eos_token_id
        if sa is not None and sa["ranges"]:
            eos = None
        B, P = ids.shape
        graphs = self.decode_graphs and dev.type == "cuda"
        st = self._decode_state(B, P + max_new_tokens, dev)
        cache = st["cache"]
        cache.seen_tokens = 0
        cls = self._prompt_classes(am, B, P, dev)
        st["npad"].copy_((cls == 2).sum(-1, keepdim=True))
        if pv is not None and self.strict_checks:  # reference :379-385, checked before any graph replay
            vc = self.config.vision_config
            n_img = B * (vc.image_size // vc.patch_size) ** 2
            n_tok = int((model_inputs["input_ids"] == self.config.image_token_index).sum())
            if n_tok != n_img:
                raise ValueError("Number of images does not match number of special image tokens in the input text. "
                                 f"Got {n_tok} image tokens in the text but {n_img} tokens from image embeddings.")
        # inv(K) (reference :221): the closed-form HIP inverse, captured into the prefill graph with the rest
        kinv = None
        # the frozen Zoe forward is captured with the rest of the prefill: every convolution of it runs on libsvla
        # (zoe_fast), no vendor library creates handles lazily under the capture
        prefill = {"ids": ids, "pv": pv, "intr": intr, "cls": cls, "kinv": kinv}
        sb = st.get("sample")
        if sb is not None:
            self._write_sample_params(sb, sa)
        first = self._prefill_graph(st, prefill) if graphs else self._prefill_body(st, prefill)
        if sb is not None:
            first, lp, lpr = first
            sb["lps"][:, :, P].copy_(torch.stack((lp, lpr)))
            sb["step"].fill_(1)
        cache.seen_tokens = P
        # the per-token update runs on the device (_greedy_bookkeep); the host reads the finished flags only every
        # EOS_CHECK_EVERY steps and cuts the output where the last row finished -- the tokens and the length are the
        # step-by-step loop's
        st["eos"].fill_(-1 if eos is None else int(eos))
        st["pad"].fill_(max(self.pad_token_id, 0))
        nxt = first.view(B, 1)
        st["fin"].copy_(nxt == st["eos"])
        st["tok"].copy_(nxt)
        st["toks"][:, P:P + 1].copy_(nxt)
        steps = 0
        while steps < max_new_tokens - 1:
            if eos is not None and steps % self.EOS_CHECK_EVERY == 0 and bool(st["fin"].all()):
                break
            p0 = cache.seen_tokens
            if graphs:
                self._decode_step_graph(st, p0)
            else:
                self._greedy_bookkeep(st, p0, self._decode_body(st, p0))
                cache.seen_tokens = p0 + 1
            steps += 1
        toks = st["toks"][:, P:P + steps + 1].clone()
        K.check_decode_mlp_timeouts("predict_action")
        if eos is not None:  # the step-by-step loop's length: up to the token where the last row finished
            hit = toks == eos
            if bool(hit.any(1).all()):
                n = toks.shape[1]
                first_eos = torch.where(hit, torch.arange(n, device=dev), n).min(1).values
                toks = toks[:, :int(first_eos.max()) + 1]
        if return_logprobs:
            lps = sb["lps"][:, :, P:P + toks.shape[1]].clone()
            return toks, lps[0], lps[1]
        return toks

    # ------------------------------------------------------------------ HF generate() surface
    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, inputs_embeds=None, cache_position=None,
                                      position_ids=None, pixel_values=None, intrinsic=None, attention_mask=None,
                                      token_type_ids=None, use_cache=True, num_logits_to_keep=None, labels=None,
                                      **kwargs):
        """Reference :445-482: the language model's hook (slicing to the uncached tokens, per-sequence positions),
        positions + 1 (PaliGemma positions are 1-indexed), pixel values only at the first step, intrinsic passed
        through.  The prefill's bidirectional prefix mask (:478-480) is built by forward() from the 2-D mask."""
        model_inputs = self.language_model.prepare_inputs_for_generation(
            input_ids, past_key_values=past_key_values, inputs_embeds=inputs_embeds, attention_mask=attention_mask,
            position_ids=position_ids, cache_position=cache_position, use_cache=use_cache,
            num_logits_to_keep=num_logits_to_keep, **kwargs)
        if model_inputs.get("position_ids") is not None:
            model_inputs["position_ids"] += 1
        if int(cache_position[0]) == 0:
            model_inputs["pixel_values"] = pixel_values
        model_inputs["token_type_ids"] = token_type_ids if int(cache_position[0]) == 0 and labels is not None else None
        model_inputs["intrinsic"] = intrinsic
        return model_inputs

    @torch.no_grad()
    def generate(self, input_ids=None, pixel_values=None, intrinsic=None, attention_mask=None,
                 max_new_tokens: Optional[int] = None, do_sample: Optional[bool] = None, eos_token_id=None,
                 pad_token_id=None, generation_config=None, temperature: Optional[float] = None,
                 top_k: Optional[int] = None, top_p: Optional[float] = None, seed: Optional[int] = None, **kwargs):
        """Greedy `generate` as the reference's predict_action calls it (:491, HF generate with do_sample=False over a
        HybridCache): the loop runs prepare_inputs_for_generation -> forward(past_key_values=Gemma2KVCache) per step
        and returns prompt + new tokens; finished sequences get pad_token_id, the loop stops once every sequence
        emitted eos.  Every step is eager here; predict_action is the graph-replayed fast path with the same tokens.
        do_sample=True needs enable_sampled_decode(): every step's token is then drawn by svla_sample_rows under
        temperature / top_k / top_p (HF's defaults: 1.0 / 50 / 1.0, or the generation_config's), keyed by `seed` (None:
        one from torch's default generator) and the token's position."""
        # HF precedence: explicit arguments override the generation_config, which overrides the defaults
        if generation_config is not None:
            if max_new_tokens is None:
                max_new_tokens = getattr(generation_config, "max_new_tokens", None)
            if do_sample is None:
                do_sample = getattr(generation_config, "do_sample", None)
            eos_token_id = getattr(generation_config, "eos_token_id", None) if eos_token_id is None else eos_token_id
            pad_token_id = getattr(generation_config, "pad_token_id", None) if pad_token_id is None else pad_token_id
            temperature = getattr(generation_config, "temperature", None) if temperature is None else temperature
            top_k = getattr(generation_config, "top_k", None) if top_k is None else top_k
            top_p = getattr(generation_config, "top_p", None) if top_p is None else top_p
        max_new_tokens = 256 if max_new_tokens is None else int(max_new_tokens)
        do_sample = bool(do_sample)
        if int(kwargs.pop("num_beams", 1)) != 1:
            raise NotImplementedError("generate: greedy decoding and sampling only (no beam search)")
        if do_sample and not self.sampled_decode:
            raise NotImplementedError("generate: greedy decoding only (the reference calls do_sample=False); "
                                      "do_sample=True needs enable_sampled_decode()")
        sa = None
        if do_sample:  # HF's defaults: temperature 1.0, top_k 50, top_p 1.0
            sa = self._sample_args("generate", True, 1.0 if temperature is None else temperature,
                                   50 if top_k is None else top_k, 1.0 if top_p is None else top_p, seed, None)
        kwargs.pop("token_type_ids", None)
        for k in ("output_attentions", "output_hidden_states", "return_dict_in_generate", "use_cache"):
            kwargs.pop(k, None)
        if kwargs:
            raise TypeError(f"generate: unsupported arguments {sorted(kwargs)}")
        self._require_merged("generate")
        self._wait_all_params()
        eos = eos_token_id if eos_token_id is not None else self.config.text_config.eos_token_id
        if isinstance(eos, (list, tuple)):
            eos = eos[0] if eos else None
        pad = pad_token_id if pad_token_id is not None else max(self.pad_token_id, 0)
        dev = self.language_model.lm_head.weight.device
        ids = input_ids.to(dev)
        B, P = ids.shape
        am = (attention_mask.to(dev) if attention_mask is not None
              else torch.ones(B, P, dtype=torch.int64, device=dev))
        pv = pixel_values.to(dev, torch.bfloat16) if pixel_values is not None else None
        intr = intrinsic.to(dev, torch.bfloat16) if intrinsic is not None else None
        cache = self.new_cache(B, P + max_new_tokens)
        cache_position = torch.arange(P, device=dev)
        finished = torch.zeros(B, dtype=torch.bool, device=dev)
        if sa is not None:
            sb = self._sample_buffers(B, 0, dev, 1)
            self._write_sample_params(sb, sa)
        for _ in range(max_new_tokens):
            mi = self.prepare_inputs_for_generation(ids, past_key_values=cache, cache_position=cache_position,
                                                    pixel_values=pv, intrinsic=intr, attention_mask=am)
            mi.pop("cache_position")
            out = self(**mi, return_dict=True)
            if sa is not None:  # the step's last-position logits [B, V] (row stride: the padded vocabulary)
                nxt = self._sample(sb, out.logits[:, -1], ids.shape[1])[0]
            else:
                nxt = self.action_argmax().view(B, -1)[:, -1]
            if eos is not None:
                nxt = torch.where(finished, torch.full_like(nxt, pad), nxt)
                finished = finished | (nxt == eos)
            ids = torch.cat([ids, nxt[:, None]], 1)
            am = torch.cat([am, torch.ones(B, 1, dtype=am.dtype, device=dev)], 1)
            cache_position = cache_position[-1:] + 1
            if eos is not None and bool(finished.all()):
                break
        K.check_decode_mlp_timeouts("generate")
        return ids

    @torch.no_grad()
    def predict_action_uncached(self, model_inputs, max_new_tokens: int = 256, eos_token_id: Optional[int] = None):
        """The same greedy decode as full re-forwards over prompt + generated tokens (no cache): prompt keys
        class 0, generated keys class 1.  Kept as the parity reference of the cached path."""
        self._wait_all_params()
        ids, pv, intr, am, dev = self._predict_inputs(model_inputs)
        eos = eos_token_id if eos_token_id is not None else self.config.text_config.eos_token_id
        B, P = ids.shape
        feats = self.get_image_features(pv, intr) if pv is not None else None
        finished = torch.zeros(B, 1, dtype=torch.bool, device=dev)
        out = []
        cur = ids
        for _ in range(max_new_tokens):
            if eos is not None and out and bool(finished.all()):
                break
            Lc = cur.shape[1]
            cls = torch.ones(B, Lc, dtype=torch.uint8, device=dev)
            cls[:, :P] = self._prompt_classes(am, B, P, dev)
            pos = self._prompt_positions(cls != 2)  # generated tokens: the attention mask extended by ones
            h, _ = self.language_model.model(self._merge_inputs(cur, feats), KVMask(cls.contiguous()), pos)
            nxt, finished = self._next_token(h, finished, eos)
            out.append(nxt)
            cur = torch.cat([cur, nxt], 1)
        return torch.cat(out, 1)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, **kwargs):
        model = super().from_pretrained(pretrained_model_name_or_path, *model_args, **kwargs)
        if model.config.use_spatial_token:  # reference :524-525
            model.language_model.model.embed_tokens.weight.data[-model.config.spatial_token_num:] = \
                model.spatial_embed_tokens.weight.data
        return model
