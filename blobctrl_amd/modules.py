"""Drop-in module shells that keep the reference's nn.Module call signatures on top of the HIP plans.

  * UNet2DConditionModel.forward(sample, timestep, encoder_hidden_states, down_block_add_samples=[...],
        mid_block_add_sample=..., up_block_add_samples=[...], return_dict=False) -> (sample,)
        (D/models/unets/unet_2d_condition.py:1039-1057; the residual lists are consumed with pop(0) like :1217,1230,1313)
  * BlobNetModel.forward(sample, timestep, conditioning_scale: float, return_dict=False)
        -> (list[12], Tensor, list[15])            (blobctrl/models/blobnet.py:720-734, 941-945)
Tensors cross this boundary as NCHW torch tensors (fp32 or fp16) exactly like the reference; inside, everything is
NHWC fp16 and runs through libblobctrl_hip.  These shells are the module-level boundary; the captured-loop engine
(pipeline.py) bypasses them and chains the plans directly.
"""
from collections import OrderedDict
from typing import List, Optional

import torch

from . import _lib
from .engine import IpAdapter, Residuals, TrunkConfig, TrunkPlan, freeu_enabled
from .launch import Recorder, run_graphed
from .weights import LoraAdapters, PackedTrunk, lora_scale_of, pad8


def _stream():
    return torch.cuda.current_stream().cuda_stream


class ModelConfig(dict):
    """`module.config` with attribute AND mapping access, like diffusers' FrozenDict (pipe:957 reads `unet.config.in_channels`,
    pipe:993 `unet.config.time_cond_proj_dim`)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class _TrunkModule(LoraAdapters, torch.nn.Module):
    """An `nn.Module` (DiffusionPipeline.register_modules, D/pipelines/pipeline_utils.py:788, accepts it; `.parameters()`, `.dtype`,
    `.device`, `.eval()`, `.to()` behave) whose forward runs a compiled launch plan.  The weights are the packed fp16 / fp32 arenas;
    they are exposed as two frozen Parameters that SHARE the arenas' storage.  `.to()` / `.half()` / `.float()` are no-ops: the layouts
    are fixed at construction (device = the one given to the constructor)."""

    def __init__(self, state_dict, config: TrunkConfig, device="cuda:0", lazy: bool = False):
        """`lazy=True` (what `from_pretrained` uses): the reference-schema state dict stays on the host and is packed on first
        use, so that the script's post-load edits - the conv_in surgery (inf:233-249), `load_lora_weights` (inf:270-273) - are
        cheap host operations; any later edit drops the packed copy and every cached plan (`_invalidate`)."""
        super().__init__()
        self._device = torch.device(device)
        self.trunk_config = config
        self._sd = None if isinstance(state_dict, PackedTrunk) else OrderedDict(state_dict)
        self._packed = state_dict if isinstance(state_dict, PackedTrunk) else None
        self._init_lora()
        self._lora_scale = 1.0                  # the scale the packed copy is (or will be) made for: set_lora_scale
        self._version = 0
        self._plans = {}
        self._make_config()
        if not lazy and self._packed is None:
            if self._device.type != "cuda":
                raise _lib.BlobCtrlHipError("blobctrl_amd modules run on MI355X only; there is no CPU fallback")
            self.weights                         # pack now

    def _make_config(self):
        config = self.trunk_config
        latent = config.out_channels if config.out_channels else 4
        self.config = ModelConfig(
            # the reference script leaves unet.config.in_channels at the LATENT channel count (4) although conv_in has 5 inputs
            # (scripts/blobctrl_inference.py:233-249); BlobNet: in_channels=4, conditioning_channels=1+F (bn config)
            in_channels=latent if config.is_blobnet or config.in_channels in (latent, latent + 1) else config.in_channels,
            conv_in_channels=config.in_channels, out_channels=config.out_channels, block_out_channels=tuple(config.block_out_channels),
            layers_per_block=config.layers_per_block, attention_head_dim=config.num_heads, norm_num_groups=config.norm_num_groups,
            cross_attention_dim=config.cross_attention_dim, time_cond_proj_dim=config.time_cond_proj_dim, sample_size=64,
            conditioning_channels=(config.in_channels - latent) if config.is_blobnet else None,
            encoder_hid_dim_type="ip_image_proj" if self.__dict__.get("ip_adapters") else None)

    # ---- weights: packed lazily from the host state dict + the active LoRA adapters
    def effective_state_dict(self, lora_scale: float = 1.0):
        """The host state dict with every ACTIVE adapter merged (W + lora_scale * weight * (alpha / r) * B A, weights.merge_lora).
        Without argument: scale 1.0, whatever scale the packed copy was made for."""
        if self._sd is None:
            raise _lib.BlobCtrlHipError("this module was built from packed weights: no host state dict to edit")
        return super().effective_state_dict(lora_scale)

    @property
    def weights(self) -> PackedTrunk:
        if self._packed is None:
            _lib.load()
            self._packed = PackedTrunk(self.effective_state_dict(self._lora_scale), self._device, self.trunk_config.block_out_channels)
        return self._packed

    @property
    def packed_fp16(self):
        return self.weights.h_arena

    @property
    def packed_fp32(self):
        return self.weights.f_arena

    def parameters(self, recurse: bool = True):
        """The packed fp16 / fp32 arenas as two frozen Parameters sharing the arenas' storage."""
        w = self.weights
        return iter([torch.nn.Parameter(w.h_arena, requires_grad=False), torch.nn.Parameter(w.f_arena, requires_grad=False)])

    def named_parameters(self, prefix: str = "", recurse: bool = True, remove_duplicate: bool = True):
        return iter(zip((prefix + "packed_fp16", prefix + "packed_fp32"), self.parameters()))

    def _invalidate(self):
        """The host weights changed: drop the packed copy and every plan compiled against it (their graphs hold its addresses)."""
        if self._device.type == "cuda" and (self._packed is not None or self._plans):
            torch.cuda.synchronize(self._device)
        for P in self._plans.values():
            P.rec.close()
        self._plans = {}
        self._packed = None
        self._version += 1

    # ---- LoRA (D/loaders/unet.py:271-340 semantics: W + (alpha / r) * B A per target module; merged when the weights are packed)
    # the registry itself (load_lora_adapter, set_adapters, unload_lora, delete_adapters, disable_lora, enable_lora) is weights.LoraAdapters;
    # every edit of it drops the packed copy
    def _lora_changed(self):
        self._invalidate()

    def load_lora_adapter(self, lora, alphas, adapter_name="default", weight: float = 1.0):
        if self._sd is None:
            raise _lib.BlobCtrlHipError("this module was built from packed weights: LoRA must be merged before packing")
        super().load_lora_adapter(lora, alphas, adapter_name, weight)

    def set_lora_scale(self, lora_scale: float = 1.0):
        """The per-call LoRA scale (`cross_attention_kwargs={"scale": s}`, scale_lora_layers of the reference: every active adapter's
        weight times s, in all LoRA layers).  The packed copy is made for one (adapters, scale) state: a scale that changes the merged
        weights drops it like `set_adapters` does, and it stays at that scale until a call asks for another.  With nothing to scale - no
        adapter merged - nothing is dropped."""
        lora_scale = float(lora_scale)
        if self._sd is not None and self._lora_state(lora_scale) != self._lora_state(self._lora_scale):
            self._invalidate()
        self._lora_scale = lora_scale

    @property
    def device(self):
        return self._device

    @property
    def dtype(self):
        """fp32 while the module still holds its host state dict and has not been packed (a freshly loaded checkpoint: the script's
        conv_in surgery `Conv2d(..., dtype=unet.dtype)` then stays in fp32 like the reference's, inf:233-249); fp16 - the compute
        dtype of the packed layouts - once packed."""
        return torch.float32 if (self._sd is not None and self._packed is None) else torch.float16

    def to(self, *a, **k):
        return self

    def _apply(self, fn, *a, **k):          # .cuda() / .half() / .float(): the packed layouts stay as built
        return self

    def _to_nhwc(self, rec, x: torch.Tensor, cpad: int) -> torch.Tensor:
        B, C, H, W = x.shape
        x = x.contiguous()
        if x.dtype not in (torch.float32, torch.float16):
            x = x.float()
        out = torch.empty(B, H * W, cpad, dtype=torch.float16, device=self.device)
        _lib.check(rec.lib.bc_nchw_to_nhwc_f16(x.data_ptr(), int(x.dtype == torch.float32), B, C, H * W, cpad,
                                               out.data_ptr(), _stream()), "bc_nchw_to_nhwc_f16")
        return out

    def _to_nchw(self, rec, t: torch.Tensor, B, C, H, W, dtype) -> torch.Tensor:
        out = torch.empty(B, C, H, W, dtype=dtype, device=self.device)
        _lib.check(rec.lib.bc_nhwc_to_nchw(t.data_ptr(), B, C, H * W, t.shape[-1], out.data_ptr(),
                                           int(dtype == torch.float32), _stream()), "bc_nhwc_to_nchw")
        return out


class BlobNetModel(_TrunkModule):
    def __init__(self, state_dict, config: TrunkConfig, device="cuda:0", lazy: bool = False):
        assert config.is_blobnet
        super().__init__(state_dict, config, device, lazy)

    @classmethod
    def from_pretrained(cls, path, device="cuda:0", **_ignored):
        """`BlobNetModel.from_pretrained(blobnet_path, ignore_mismatched_sizes=True)` (inf:252): a directory with
        config.json + diffusion_pytorch_model.safetensors, or the .safetensors file itself."""
        from .checkpoint import load_blobnet
        sd, cfg = load_blobnet(path)
        return cls(sd, cfg, device, lazy=True)

    def _plan(self, B, H, W):
        key = (B, H, W)
        if key not in self._plans:
            rec = Recorder(self.device)
            P = type("Plan", (), {})()
            P.rec = rec
            P.x_in = rec.zeros(B, H * W, pad8(self.trunk_config.in_channels))
            P.t = rec.zeros(1, dtype=torch.float32)
            P.idx = rec.zeros(1, dtype=torch.int32)
            P.scale = rec.zeros(1, dtype=torch.float32)
            P.seg = rec.begin("blobnet")
            plan = TrunkPlan(rec, self.weights, self.trunk_config, B, H, W)
            plan.record_time(P.t, P.idx)
            P.res = plan.record_forward(P.x_in, None, zero_scale=(1.0, P.scale, P.idx))
            P.shapes = plan.feat_shapes
            self._plans[key] = P
        return self._plans[key]

    @torch.no_grad()
    def forward(self, sample: torch.Tensor, timestep, conditioning_scale: float = 1.0, return_dict: bool = False, **kw):
        if not isinstance(conditioning_scale, float):
            raise TypeError("conditioning_scale must be a Python float (pipeline_blobnet.py:395-396)")
        if return_dict:
            raise NotImplementedError("return_dict=True is broken in the reference (bn:947-956); use return_dict=False")
        B, C, H, W = sample.shape
        if C != self.trunk_config.in_channels:
            raise ValueError(f"expected {self.trunk_config.in_channels} input channels, got {C}")
        # through the dispatcher (torch.ops.blobctrl.blobnet_forward, ops.py): profilers and fake-tensor tracing see the call
        from . import ops
        outs = torch.ops.blobctrl.blobnet_forward(sample, float(timestep), conditioning_scale, ops.register(self))
        nd = len(ops.blobnet_output_shapes(self.trunk_config, B, H, W)[0])
        return list(outs[:nd]), outs[nd], list(outs[nd + 1:])

    def _forward_impl(self, sample: torch.Tensor, timestep: float, conditioning_scale: float):
        """Body of torch.ops.blobctrl.blobnet_forward: one graph replay of the recorded trunk."""
        B, C, H, W = sample.shape
        P = self._plan(B, H, W)
        P.x_in.copy_(self._to_nhwc(P.rec, sample, P.x_in.shape[-1]))
        P.t.fill_(float(timestep))
        P.scale.fill_(conditioning_scale)
        run_graphed(P.seg, self.device)
        dt = sample.dtype if sample.dtype in (torch.float16, torch.float32) else torch.float32
        sd, sm, su = P.shapes
        down = [self._to_nchw(P.rec, r, B, c, h, w, dt) for r, (c, h, w) in zip(P.res.down, sd)]
        mid = self._to_nchw(P.rec, P.res.mid, B, sm[0], sm[1], sm[2], dt)
        up = [self._to_nchw(P.rec, r, B, c, h, w, dt) for r, (c, h, w) in zip(P.res.up, su)]
        return down, mid, up



class UNet2DConditionModel(_TrunkModule):
    def __init__(self, state_dict, config: TrunkConfig, device="cuda:0", lazy: bool = False):
        assert not config.is_blobnet
        super().__init__(state_dict, config, device, lazy)
        self.__dict__["freeu"] = None          # (s1, s2, b1, b2) after enable_freeu
        self.__dict__.setdefault("ip_adapters", [])        # loaded IP-Adapters: device weights + the scale table of each
        self.__dict__["pag"] = None            # (chunks of the batch, block prefixes) after set_pag_attn_processors

    @classmethod
    def from_pretrained(cls, path, subfolder=None, extra_in_channels=0, lora_path=None, lora_scale=1.0, device="cuda:0", **_ignored):
        """`UNet2DConditionModel.from_pretrained(sd15_path, subfolder="unet")` (inf:229-232): the file's own 4-channel UNet, held on
        the host until first use, so that the script's next statements - the conv_in 4 -> 5 surgery through `unet.conv_in`
        (inf:233-249) and `pipeline.load_lora_weights` (inf:270-273) - work on it unchanged.  `extra_in_channels=1` /
        `lora_path=` do both in this call instead."""
        import os
        from .checkpoint import load_unet
        sd, cfg = load_unet(os.path.join(path, subfolder) if subfolder else path, extra_in_channels, lora_path, lora_scale)
        return cls(sd, cfg, device, lazy=True)

    # ---- FreeU (unet_2d_condition.py:839-870): the reference sets s1 / s2 / b1 / b2 on every up block; here the four values are module
    # state that the plans read (this module's own, and the loop engine's through the pipeline)
    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """Enables the FreeU mechanism (https://arxiv.org/abs/2309.11497) in up_blocks.0 (s1, b1) and up_blocks.1 (s2, b2).  As in the
        reference, a value of 0.0 or None among the four leaves the plain network running."""
        self.__dict__["freeu"] = (s1, s2, b1, b2)

    def disable_freeu(self):
        """Disables the FreeU mechanism."""
        self.__dict__["freeu"] = None

    # ---- PAG (D/pipelines/pag/pag_utils.py `_set_pag_attn_processor`): the reference puts PAGCFGIdentitySelfAttnProcessor2_0 (batch = [uncond |
    # cond | perturbed]) or PAGIdentitySelfAttnProcessor2_0 ([cond | perturbed]) on the named attn1 modules; here it is module state that the plans read
    def set_pag_attn_processors(self, pag_applied_layers, do_classifier_free_guidance: bool = True):
        """Perturb the self-attentions `pag_applied_layers` names (a string or a list of strings, matched as PAGMixin matches them; ValueError
        for an id that matches nothing): in those blocks the last third of the batch - the last half with do_classifier_free_guidance False
        - takes its own V as attention output.  forward then needs a batch that divides by 3 (by 2)."""
        from . import pag
        self.__dict__["pag"] = (3 if do_classifier_free_guidance else 2, pag.resolve_layers(self.trunk_config, pag_applied_layers))

    def unset_pag_attn_processors(self):
        """Back to the plain self-attention everywhere: the plans every other call uses."""
        self.__dict__["pag"] = None

    # ---- IP-Adapter (D/loaders/unet.py:823-853: IPAdapterAttnProcessor2_0 in every attn2, encoder_hid_proj = the image projections)
    def load_ip_adapter_weights(self, state_dicts):
        """`unet._load_ip_adapter_weights`: one adapter or a list, each the original {"image_proj", "ip_adapter"} dict or a .safetensors
        file (checkpoint.load_ip_adapter).  Base adapters and IP-Adapter Plus (weights.ip_adapter_layout); every scale starts at 1.0 as in the reference.  The weights live beside
        the packed trunk: nothing is re-packed, and the adapter-less plans stay what they were."""
        from .checkpoint import load_ip_adapter
        from .weights import convert_ip_adapter, ip_adapter_on_device, ip_attn2_prefixes
        if self._sd is None:
            raise _lib.BlobCtrlHipError("this UNet was built from packed weights: IP-Adapter weights are laid out against its state dict")
        prefixes = ip_attn2_prefixes(self._sd.keys())
        host = [convert_ip_adapter(sd, prefixes, self.trunk_config.cross_attention_dim) for sd in load_ip_adapter(state_dicts)]
        self._drop_ip_plans()
        self.__dict__["ip_adapters"] = [ip_adapter_on_device(h, self._device) for h in host]
        self._make_config()

    def unload_ip_adapter(self):
        """Back to the adapter-less UNet: config.encoder_hid_dim_type is None again and forward takes no image_embeds."""
        self._drop_ip_plans()
        self.__dict__["ip_adapters"] = []
        self._make_config()

    def set_ip_adapter_scale(self, scale):
        """A float for every adapter, or one entry per adapter: a float, or a list with one value per attn2 processor in
        `attn_processors` order.  Only the device scale tables are rewritten - recorded plans and their graphs read them on replay."""
        ads = self.__dict__.get("ip_adapters") or []
        if not ads:
            raise ValueError("no IP-Adapter is loaded")
        scales = [scale] * len(ads) if not isinstance(scale, (list, tuple)) else list(scale)
        if len(scales) != len(ads):
            raise ValueError(f"Cannot assign {len(scales)} scales to {len(ads)} IP-Adapter.")
        for ad, s in zip(ads, scales):
            n = ad["scales"].numel()
            vals = [float(s)] * n if not isinstance(s, (list, tuple)) else [float(v) for v in s]
            if len(vals) != n:
                raise ValueError(f"a per-block scale list has one value per attn2 processor ({n}), got {len(vals)}")
            ad["scales"].copy_(torch.tensor(vals, dtype=torch.float32))

    def _drop_ip_plans(self):
        """Plans recorded with adapters point at their weights and scale tables: they go with them."""
        self.__dict__["_ip_version"] = self.__dict__.get("_ip_version", 0) + 1      # (the pipeline's loop engine follows: pipeline.engine)
        drop = [k for k in self._plans if any(isinstance(x, tuple) and x[:1] == ("ip",) for x in k)]
        if drop and self._device.type == "cuda":
            torch.cuda.synchronize(self._device)
        for k in drop:
            self._plans.pop(k).rec.close()

    def _check_image_embeds(self, added_cond_kwargs, B):
        """unet_2d_condition.py process_encoder_hidden_states: with adapters loaded, `image_embeds` - a list with one [B][n_images][embed_dim]
        tensor per adapter - is required; without one it is not taken."""
        ads = self.__dict__.get("ip_adapters") or []
        embeds = (added_cond_kwargs or {}).get("image_embeds")
        if not ads:
            if embeds is not None:
                raise ValueError("image_embeds were passed in added_cond_kwargs, but no IP-Adapter is loaded (load_ip_adapter_weights)")
            return None
        if embeds is None:
            raise ValueError(f"{type(self)} has the config param `encoder_hid_dim_type` set to 'ip_image_proj' which requires the keyword "
                             "argument `image_embeds` to be passed in  `added_conditions`")
        if torch.is_tensor(embeds):
            embeds = [embeds.unsqueeze(1) if embeds.ndim == 2 else embeds]
        if len(embeds) != len(ads):
            raise ValueError(f"image_embeds holds {len(embeds)} tensors for {len(ads)} loaded IP-Adapters")
        from .weights import ip_adapter_embed_dim
        for e, ad in zip(embeds, ads):
            width = ip_adapter_embed_dim(ad)
            if ad.get("layout") == "plus":                 # hidden states: [batch][images][S][embed_dims]
                if e.ndim != 4 or e.shape[0] != B or e.shape[3] != width:
                    raise ValueError(f"image_embeds of an IP-Adapter Plus must be [batch = {B}][images][tokens][{width}], got {tuple(e.shape)}")
            elif e.ndim != 3 or e.shape[0] != B or e.shape[2] != width:
                raise ValueError(f"image_embeds of an adapter must be [batch = {B}][images][{width}], got {tuple(e.shape)}")
        return list(embeds)

    # ---- `unet.conv_in` as the script uses it (inf:233-249): reads .weight / .bias / .out_channels, assigns a wider Conv2d
    @property
    def conv_in(self):
        if self._sd is None:
            raise _lib.BlobCtrlHipError("this UNet was built from packed weights: conv_in is not editable")
        w, b = self._sd["conv_in.weight"], self._sd.get("conv_in.bias")
        conv = torch.nn.Conv2d(w.shape[1], w.shape[0], kernel_size=3, stride=1, padding=1, bias=b is not None)
        with torch.no_grad():
            conv.weight.copy_(w)
            if b is not None:
                conv.bias.copy_(b)
        return conv

    def __setattr__(self, name, value):
        if name == "conv_in" and isinstance(value, torch.nn.Module):
            if self._sd is None:
                raise _lib.BlobCtrlHipError("this UNet was built from packed weights: conv_in is not editable")
            w = value.weight.detach().float().cpu()
            if w.ndim != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[0] != self._sd["conv_in.weight"].shape[0]:
                raise ValueError(f"conv_in must be a 3x3 convolution with {self._sd['conv_in.weight'].shape[0]} output channels")
            self._sd["conv_in.weight"] = w.clone()
            if value.bias is not None:
                self._sd["conv_in.bias"] = value.bias.detach().float().cpu().clone()
            import dataclasses
            self.trunk_config = dataclasses.replace(self.trunk_config, in_channels=w.shape[1])     # (the caller's config object is not touched)
            self._make_config()
            self._invalidate()
            return
        super().__setattr__(name, value)

    def _res_shapes(self, H, W):
        boc = self.trunk_config.block_out_channels
        nb = len(boc)
        down = [(boc[0], H, W)]
        h, w = H, W
        for i in range(nb):
            down += [(boc[i], h, w)] * self.trunk_config.layers_per_block
            if i < nb - 1:
                h, w = (h + 1) // 2, (w + 1) // 2
                down.append((boc[i], h, w))
        mid = (boc[-1], h, w)
        # up: mirror of the down resolutions
        sizes = []
        hh, ww = H, W
        for i in range(nb):
            sizes.append((hh, ww))
            if i < nb - 1:
                hh, ww = (hh + 1) // 2, (ww + 1) // 2
        rev = list(reversed(boc))
        up = []
        for i in range(nb):
            hh, ww = sizes[nb - 1 - i]
            up += [(rev[i], hh, ww)] * (self.trunk_config.layers_per_block + 1)
            if i < nb - 1:
                up.append((rev[i],) + sizes[nb - 2 - i])
        return down, mid, up

    def _plan(self, B, H, W, T, Dc, with_res, cond=False, freeu=False, ip=(), ip_masked=False, pag=None):
        """`cond`: the plan takes a `timestep_cond` (fp16 [B][pad8(time_cond_proj_dim)]) and adds cond_proj of it to the sinusoid; a
        plan of its own, so that calls without one keep the launches they always recorded.  `freeu`: likewise a plan of its own, with
        bc_freeu in up_blocks.0 / up_blocks.1 reading (s1, s2, b1, b2) from the plan buffer P.freeu.  `ip_masked`: the call brings
        `ip_adapter_masks` - a plan of its own again, with bc_attention_ip_masked behind every attn2 and one fp16 mask buffer per adapter
        and attention level (P.ip_adapters[i].mask_bufs); the key says "masked", never what the masks hold.  `pag` = (chunks, block
        prefixes): a plan of its own whose attn1 in those blocks is the identity on V for the last B / chunks images."""
        key = (B, H, W, T, Dc, with_res) + (("cond",) if cond else ()) + (("freeu",) if freeu else ()) + ((("ip",) + tuple(ip),) if ip else ()) + \
            ((("ip", "masked"),) if ip and ip_masked else ()) + ((("pag", pag[0]) + tuple(pag[1]),) if pag else ())
        if key not in self._plans:
            rec = Recorder(self.device)
            P = type("Plan", (), {})()
            P.rec = rec
            P.x_in = rec.zeros(B, H * W, pad8(self.trunk_config.in_channels))
            P.ctx = rec.zeros(B, T, Dc)
            P.t = rec.zeros(1, dtype=torch.float32)
            P.idx = rec.zeros(1, dtype=torch.int32)
            residuals = None
            if with_res:
                sd, sm, su = self._res_shapes(H, W)
                mk = lambda s: rec.zeros(B, s[1] * s[2], s[0])
                residuals = Residuals([mk(s) for s in sd], mk(sm), [mk(s) for s in su], bmod=B)
                P.res_shapes = (sd, sm, su)
            P.residuals = residuals
            P.seg = rec.begin("unet")
            plan = TrunkPlan(rec, self.weights, self.trunk_config, B, H, W)
            if pag:
                if B % pag[0]:
                    raise ValueError(f"PAG attention processors are set for a batch of {pag[0]} chunks; this batch is {B}")
                plan.pag_layers, plan.pag_images = frozenset(pag[1]), B // pag[0]
            if freeu:
                P.freeu = plan.freeu_params = rec.zeros(4, dtype=torch.float32)
            if ip:
                # `ip` = images per adapter, the part of the adapter configuration a call can change; the adapter count and the embedding
                # width are fixed by what is loaded, and load / unload drop every plan that carries an `ip` entry (_drop_ip_plans).  Scales
                # are no part of the key: the launches read them from the adapters' device tables
                ads = self.__dict__["ip_adapters"]
                made = [IpAdapter.for_plan(rec, ad, B, entry, masked=bool(ip_masked), mask_name=f"ip_mask{i}")
                        for i, (entry, ad) in enumerate(zip(ip, ads))]                            # (a Plus adapter's entry: (images, S))
                plan.ip_adapters, P.ip_embeds = [m[0] for m in made], [m[1] for m in made]
                P.ip_adapters = plan.ip_adapters
            plan.record_context(P.ctx, T)
            if cond:
                P.cond = rec.zeros(B, pad8(self.trunk_config.time_cond_proj_dim))
                plan.record_time(P.t, P.idx, cond=P.cond)
            else:
                plan.record_time(P.t, P.idx)
            P.eps = plan.record_forward(P.x_in, residuals)
            self._plans[key] = P
        return self._plans[key]

    def _fill_residual(self, P, buf: torch.Tensor, r: torch.Tensor, shape):
        """Place an NCHW residual (the right-hand square slice the pipeline passes, pipe:1085-1087) into the canvas."""
        C, H, W = shape
        B = r.shape[0]
        ws = r.shape[-1]
        tmp = self._to_nhwc(P.rec, r, C)
        buf.view(B, H, W, C)[:, :, W - ws:, :].copy_(tmp.view(B, H, ws, C))

    @torch.no_grad()
    def forward(self, sample, timestep, encoder_hidden_states, timestep_cond=None, cross_attention_kwargs=None,
                down_block_add_samples: Optional[List[torch.Tensor]] = None, mid_block_add_sample=None,
                up_block_add_samples: Optional[List[torch.Tensor]] = None, added_cond_kwargs=None,
                return_dict: bool = False, **kw):
        B, C, H, W = sample.shape
        if C != self.trunk_config.in_channels:
            raise ValueError(f"expected {self.trunk_config.in_channels} input channels, got {C}")
        is_blobnet = (down_block_add_samples is not None and mid_block_add_sample is not None
                      and up_block_add_samples is not None)                        # unet_2d_condition.py:1200
        # unet_2d_condition.py:1152 -> embeddings.py:576-579: a UNet with time_cond_proj_dim adds cond_proj(timestep_cond) to the sinusoid;
        # without a timestep_cond it runs without the add, as the reference does
        dim = self.trunk_config.time_cond_proj_dim
        if timestep_cond is not None:
            if dim is None:
                raise ValueError("timestep_cond was given, but this UNet has no time_embedding.cond_proj (config.time_cond_proj_dim is None)")
            if tuple(timestep_cond.shape) != (B, dim):
                raise ValueError(f"timestep_cond must have shape {(B, dim)} (batch, time_cond_proj_dim), got {tuple(timestep_cond.shape)}")
        # "ip_adapter_masks" leaves the dict before the LoRA scale is read; without a loaded adapter nothing reads it (the reference's
        # quiet_attn_parameters, attention_processor.py:480)
        from . import ip_masks
        cross_attention_kwargs, masks = ip_masks.split_kwargs(cross_attention_kwargs)
        self.set_lora_scale(lora_scale_of(cross_attention_kwargs))          # (a change of scale re-packs: the plans below are then new ones)
        # the image embeddings reach the body beside the dispatcher's fixed schema, as module state of this one call
        self.__dict__["_image_embeds"] = embeds = self._check_image_embeds(added_cond_kwargs, B)
        self.__dict__["_ip_masks"] = ip_masks.check_masks(masks, [int(e.shape[1]) for e in embeds]) if embeds and masks is not None else None
        # through the dispatcher (torch.ops.blobctrl.unet_forward, ops.py); `timestep_cond` is the op's optional trailing argument
        from . import ops
        extra = () if timestep_cond is None else (timestep_cond,)
        try:
            eps = torch.ops.blobctrl.unet_forward(sample, float(timestep), encoder_hidden_states,
                                                  list(down_block_add_samples) if is_blobnet else [], mid_block_add_sample if is_blobnet else None,
                                                  list(up_block_add_samples) if is_blobnet else [], ops.register(self), *extra)
        finally:
            self.__dict__["_image_embeds"] = self.__dict__["_ip_masks"] = None      # (state of this one call: a later direct op call sees none)
        if is_blobnet:                                   # the reference consumes the two lists with pop(0) (:1217, 1230, 1313)
            del down_block_add_samples[:]
            del up_block_add_samples[:]
        dt = sample.dtype if sample.dtype in (torch.float16, torch.float32) else torch.float32
        return (eps.to(dt),)

    def _forward_impl(self, sample, timestep, encoder_hidden_states, down_block_add_samples, mid_block_add_sample, up_block_add_samples,
                      timestep_cond=None):
        """Body of torch.ops.blobctrl.unet_forward: eps [B][4][H][W] fp32."""
        B, C, H, W = sample.shape
        is_blobnet = mid_block_add_sample is not None
        T, Dc = encoder_hidden_states.shape[1:]
        freeu = self.__dict__.get("freeu")
        embeds, masks = self.__dict__.get("_image_embeds"), self.__dict__.get("_ip_masks")
        P = self._plan(B, H, W, T, Dc, is_blobnet, cond=timestep_cond is not None, freeu=freeu_enabled(freeu),
                       ip=tuple(int(e.shape[1]) if e.ndim == 3 else (int(e.shape[1]), int(e.shape[2])) for e in embeds) if embeds else (),
                       ip_masked=bool(embeds) and masks is not None, pag=self.__dict__.get("pag"))
        for buf, e in zip(getattr(P, "ip_embeds", ()), embeds or ()):
            buf.copy_(e.to(self.device, torch.float16).reshape(buf.shape))
        if embeds and masks is not None:
            from . import ip_masks
            ip_masks.fill_plan_masks(P.ip_adapters, masks, self.device)
        if freeu_enabled(freeu):
            P.freeu.copy_(torch.tensor([float(v) for v in freeu], dtype=torch.float32))
        if timestep_cond is not None:
            P.cond.zero_()
            P.cond[:, : timestep_cond.shape[1]].copy_(timestep_cond.to(self.device, torch.float16))
        P.x_in.copy_(self._to_nhwc(P.rec, sample, P.x_in.shape[-1]))
        P.ctx.copy_(encoder_hidden_states.to(self.device, torch.float16))
        P.t.fill_(float(timestep))
        if is_blobnet:
            sd, sm, su = P.res_shapes
            if len(down_block_add_samples) != len(sd) or len(up_block_add_samples) != len(su):
                raise ValueError("wrong number of BlobNet residuals")
            for buf, s in zip(P.residuals.down, sd):
                self._fill_residual(P, buf, down_block_add_samples.pop(0), s)     # lists are consumed (:1217,1230)
            self._fill_residual(P, P.residuals.mid, mid_block_add_sample, sm)
            for buf, s in zip(P.residuals.up, su):
                self._fill_residual(P, buf, up_block_add_samples.pop(0), s)        # (:1313)
        run_graphed(P.seg, self.device)
        out = torch.empty(B, self.trunk_config.out_channels, H, W, dtype=torch.float32, device=self.device)
        out.copy_(P.eps.view(B, H, W, self.trunk_config.out_channels).permute(0, 3, 1, 2))
        return out

