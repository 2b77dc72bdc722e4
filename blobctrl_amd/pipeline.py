"""The blob-conditioned denoising loop on MI355X: host-side mirror of StableDiffusionBlobNetPipeline.__call__.

Mirrors blobctrl/pipelines/pipeline_blobnet.py:743-1166 for the hot-path part:
same keyword names and meaning (`num_inference_steps`, `guidance_scale`, `generator`, `latents`,
`blobnet_conditioning_scale` (must be a Python float, pipe:395-396), `blobnet_control_guidance_start/end`,
`output_type`), same error behaviour for bad arguments.  The VAE either side of the loop is optional:
with `vae=blobctrl_amd.vae.AutoencoderKL(...)` the call also accepts `fg_image` / `bg_image` (pipe:970-971) and returns decoded
images for `output_type="pt" | "np"` (pipe:1132-1146); with `text_encoder=blobctrl_amd.clip_text.CLIPTextModel(...)`,
`encode_prompt(prompt_ids, negative_prompt_ids)` produces the prompt embeddings (tokenisation stays on the host).

Execution model: one static launch plan per (batch, canvas, steps) configuration -
    prologue (once per edit): cross-attention K/V of the prompt embeddings
    step A (BlobNet active):  assemble BlobNet input -> BlobNet (batch B, CFG halves share it) -> assemble UNet input
                              -> UNet (batch 2B, BlobNet residuals added in GEMM epilogues) -> crop + CFG + scheduler step
    step I (BlobNet inactive, cond_scale * keep[i] == 0): UNet only
each captured once into a hipGraph and replayed per step; per-step scalars (timestep, scheduler coefficients,
conditioning scale) live in device tables indexed by a device-side step counter.
"""
import os
from collections import namedtuple
from typing import List, Optional, Union

import torch

from . import _lib
from .edit_plan import PlanSpec, record_plan
from .engine import TrunkConfig, freeu_enabled
from .schedulers import OPTION_KINDS, draw_variance_noise, randn_tensor, stack_request_tables, table_class
from .weights import PackedTrunk, lora_scale_of
from . import ip_masks
from . import pag as pag_mod


def get_guidance_scale_embedding(w: torch.Tensor, embedding_dim: int = 512, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The `timestep_cond` of a distilled LCM UNet (pipe:456-483): w = guidance_scale - 1, one entry per sample -> [len(w), embedding_dim],
    columns [sin(a_k) | cos(a_k) | 0 if embedding_dim is odd], a_k = 1000 w * exp(-ln(1e4) k / (half - 1)), half = embedding_dim // 2.
    Host work in fp32 torch with the reference's operation order, so the values are the reference's bit for bit."""
    if w.dim() != 1:
        raise ValueError("w must be one-dimensional (one guidance weight per sample)")
    half = embedding_dim // 2
    rate = torch.log(torch.tensor(10000.0)) / (half - 1)
    freq = torch.exp(torch.arange(half, dtype=dtype) * -rate)
    angle = (w * 1000.0).to(dtype)[:, None] * freq[None, :]
    out = torch.zeros(w.shape[0], embedding_dim, dtype=angle.dtype)
    out[:, :half] = torch.sin(angle)
    out[:, half:2 * half] = torch.cos(angle)
    return out


def blobnet_keep(num_steps, start, end):
    """pipe:1006-1012."""
    return [1.0 - float(i / num_steps < start or (i + 1) / num_steps > end) for i in range(num_steps)]


class EditSetup(namedtuple("EditSetup", "requests tables n stochastic third_order scaled coef t_rows scale_rows evals")):
    """What the arguments of an edit come to (`BlobCtrlEngine._setup`), for `denoise` to run and `compile_plan` to save.  A call without
    lists is the case "one table, shared by every image" of a call with lists, which has a table per request:
    requests: whether any argument was a list - the plan form; tables: the table objects, one or B; n: the loop length (the longest
    table's evaluations); stochastic, third_order, scaled: the step form and input scaling of the plan (`PlanSpec`);
    coef: [n][16] with the guidance scale in column 11, or [B][n][16] (`stack_request_tables`); t_rows: [n][1 or B] fp32, the timestep of
    every step and table; scale_rows: [n][Bi], conditioning scale * keep of every step and image; evals: evaluations per table."""

    @property
    def active(self):
        """Per step, whether it runs BlobNet: when any image's conditioning scale is not 0 in it."""
        return [any(v != 0.0 for v in row) for row in self.scale_rows]

    @property
    def segments(self):
        return ["step_active" if a else "step_inactive" for a in self.active]

    def plan_spec(self, B, h, w, T, ctx_dim, *, per_request, single, freeu=False, ip=(), ip_masked=False, pag=(), blend=False):
        """The PlanSpec of this set-up: the loop length, the step form, the input scaling and the request form are the set-up's, the rest
        is the call's."""
        return PlanSpec(B, h, w, T, ctx_dim, self.n, per_request, self.stochastic, self.third_order, self.scaled, single, freeu,
                        self.requests, ip, ip_masked, pag, blend)


class _PreviewVAE:
    """Per-step previews with a tiny decoder held next to the pipeline (what diffusers users do with `AutoencoderTiny` inside
    `callback_on_step_end`): `load_preview_vae` / `unload_preview_vae` / `preview`, shared by the engine and the pipeline.  Additive: no edit,
    plan or launch of the loop changes."""
    preview_vae = None                                                # blobctrl_amd.tiny_vae.AutoencoderTiny, or None

    def load_preview_vae(self, path_or_state_dict):
        """A TAESD checkpoint folder (config.json + diffusion_pytorch_model.safetensors) or a state dict -> `self.preview_vae`."""
        from .tiny_vae import AutoencoderTiny
        if isinstance(path_or_state_dict, (str, os.PathLike)):
            self.preview_vae = AutoencoderTiny.from_pretrained(os.fspath(path_or_state_dict), device=str(self.device))
        else:
            self.preview_vae = AutoencoderTiny(path_or_state_dict, device=str(self.device))
        return self.preview_vae

    def unload_preview_vae(self):
        self.preview_vae = None

    def _preview_loop_streams(self):
        return ()

    def preview(self, latents: torch.Tensor, output_type: str = "pil"):
        """The image of the latents a `callback_on_step_end` receives (already scaled; TAESD's scaling factor is 1).  "uint8": the device
        tensor [B][8h][8w][3] of AutoencoderTiny.preview; "pt" / "np" / "pil": AutoencoderTiny.decode through
        VaeImageProcessor.postprocess.  Enqueued on the caller's current stream with no host synchronisation; the loop's streams are made to
        wait for the READ of `latents` (not for the decoder), so a callback may hand over the loop's own latent buffer and return."""
        if self.preview_vae is None:
            raise ValueError("no preview VAE is loaded: call load_preview_vae(path_or_state_dict) first")
        if output_type not in ("pil", "np", "pt", "uint8"):
            raise ValueError(f"preview: output_type {output_type!r} (pil, np, pt or uint8)")
        tiny = self.preview_vae
        if output_type == "uint8":
            out = tiny.preview(latents)
        else:
            out = tiny.decode(latents, return_dict=False)[0]
        if tiny.input_read is not None:
            for st in self._preview_loop_streams():
                st.wait_event(tiny.input_read)
        if output_type == "uint8":
            return out
        proc = getattr(self, "image_processor", None)
        if proc is None:
            from .image_processor import VaeImageProcessor
            proc = VaeImageProcessor(vae_scale_factor=8, do_convert_rgb=True)
        return proc.postprocess(out, output_type=output_type, do_denormalize=[True] * out.shape[0])


class BlobCtrlEngine(_PreviewVAE):
    """The denoising hot path on MI355X at tensor level (prompt embeddings, image latents, scores, DINO feature in; latents out):
    static launch plans per (batch, canvas, steps), hipGraph replay, two streams.  `StableDiffusionBlobNetPipeline` below wraps it
    with the reference pipeline's constructor and `__call__` signature."""

    def __init__(self, unet_state_dict, blobnet_state_dict, unet_config: TrunkConfig, blobnet_config: TrunkConfig,
                 device="cuda:0", scheduler: str = "unipc", use_graphs: bool = True, vae=None, text_encoder=None,
                 max_cached_plans: int = 4, compile_only: bool = False):
        """`compile_only=True` (device may then be "cpu"): the engine only COMPILES plans into `.bcplan` files (`compile_plan`) for the
        C plan runtime (bc_plan_load / bc_step); nothing can be executed and no GPU is touched."""
        self.device = torch.device(device)
        self.compile_only = compile_only
        if self.device.type != "cuda" and not compile_only:
            raise _lib.BlobCtrlHipError("blobctrl_amd runs on MI355X only (device must be cuda:N); there is no CPU fallback")
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
        self.lib = _lib.load()
        self.unet_cfg, self.blob_cfg = unet_config, blobnet_config
        # either reference-schema state dicts (packed here) or already-packed / broadcast replicas (dist.broadcast_packed)
        self.unet_w = unet_state_dict if isinstance(unet_state_dict, PackedTrunk) else \
            PackedTrunk(unet_state_dict, self.device, unet_config.block_out_channels)
        self.blob_w = blobnet_state_dict if isinstance(blobnet_state_dict, PackedTrunk) else \
            PackedTrunk(blobnet_state_dict, self.device, blobnet_config.block_out_channels)
        self.scheduler_kind = scheduler
        self.scheduler_params = (1000, 0.00085, 0.012)               # (num_train_timesteps, beta_start, beta_end): SD-1.5 values
        self.use_graphs = use_graphs and not os.environ.get("BC_NO_GRAPHS")    # diagnostics: eager launches from the host loop
        if self.device.type == "cuda":
            # (stream priorities were measured and do nothing on this part: DESIGN 9)
            self.stream = torch.cuda.Stream(device=self.device)
            self.side_stream = torch.cuda.Stream(device=self.device)     # BlobNet branch runs here, concurrently with the UNet
            self.side_stream2 = torch.cuda.Stream(device=self.device)    # (BC_SPLIT_CFG: the cond half of the UNet batch)
        self.two_streams = not os.environ.get("BC_ONE_STREAM")
        self.loop_graph = os.environ.get("BC_LOOP_GRAPH", "1") != "0"     # whole-edit graph (one launch per edit) vs one graph per step
        self._plans = {}                                              # (batch, canvas, steps, ...) -> plan, least recently used first
        # plan / graph cache traffic (bench.py prints it: C4's eight per-request batches of a rank must replay ONE captured whole-edit graph)
        self.cache_stats = dict(plans_recorded=0, plan_hits=0, loop_graph_captures=0, loop_graph_hits=0)
        self.max_cached_plans = max(1, int(max_cached_plans))         # a 512^2 batch-1 plan holds ~2.5 GB of activations
        self.max_loop_graphs = 4                                      # whole-edit graphs kept per plan (one per active / inactive pattern)
        self._sched_cache = {}
        self.feat_dim = blobnet_config.in_channels - 5
        self.vae = vae                                                # optional blobctrl_amd.vae.AutoencoderKL
        self.text_encoder = text_encoder                              # optional blobctrl_amd.clip_text.CLIPTextModel
        self.ip_adapters = []                                         # loaded IP-Adapters (set_ip_adapters): device weights + scale tables

    # ------------------------------------------------------------------------------------------------ IP-Adapter
    def set_ip_adapters(self, adapters):
        """The loaded IP-Adapters, as UNet2DConditionModel.load_ip_adapter_weights lays them out on the device (proj_w, proj_b, norm_w,
        norm_b, kv per attn2 block, the fp32 scale table); [] = none.  Plans recorded with adapters point at their weights and scale
        tables and go with them; adapter-less plans stay.  Scales are device data: rewriting a table records nothing."""
        drop = [k for k in self._plans if any(isinstance(x, tuple) and x[:1] == ("ip",) for x in k)]
        if drop and self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for k in drop:
            self._plans.pop(k).rec.close()
        self.ip_adapters = list(adapters or [])

    def _ip_layout(self, embeds, Bu, B, duplicated, pag=False):
        """`ip_adapter_image_embeds` of a call -> (plan entry per adapter, [fp16-able tensor] per adapter).  One tensor per loaded adapter,
        batch = the UNet batch ([negative, positive] halves with classifier-free guidance): 3D [Bu][images][embed_dim] for a base adapter
        (entry: images), 4D [Bu][images][S][embed_dims] - the image encoder's hidden states - for an IP-Adapter Plus (entry: (images, S)).
        `duplicated`: the plan runs the positive prompts in both halves, so B rows are taken twice.  `pag`: a PAG plan runs B perturbed
        images behind the `Bu` the call brings; they take the rows of the positive chunk again (_prepare_perturbed_attention_guidance)."""
        if embeds is None:
            if self.ip_adapters:
                raise ValueError(f"{len(self.ip_adapters)} IP-Adapter(s) are loaded: pass `ip_adapter_image_embeds` (one tensor per adapter), or unload them")
            return (), []
        if not self.ip_adapters:
            raise ValueError("`ip_adapter_image_embeds` were passed, but no IP-Adapter is loaded (load_ip_adapter)")
        if not isinstance(embeds, (list, tuple)) or len(embeds) != len(self.ip_adapters):
            raise ValueError(f"`ip_adapter_image_embeds` must be a list with one tensor per loaded IP-Adapter ({len(self.ip_adapters)})")
        from .weights import ip_adapter_embed_dim
        out = []
        for e, ad in zip(embeds, self.ip_adapters):
            width = ip_adapter_embed_dim(ad)
            if ad.get("layout") == "plus":                 # hidden states of the image encoder: [batch][images][S][embed_dims]
                if e.ndim != 4 or e.shape[3] != width:
                    raise ValueError(f"an IP-Adapter Plus takes hidden states [batch][images][tokens][{width}], got {tuple(e.shape)}")
            elif e.ndim != 3 or e.shape[2] != width:
                raise ValueError(f"an adapter's image embeddings must be [batch][images][{width}], got {tuple(e.shape)}")
            if duplicated and e.shape[0] == B:
                e = torch.cat([e, e], 0)
            if e.shape[0] != Bu:
                raise ValueError(f"`ip_adapter_image_embeds` hold {e.shape[0]} rows, the UNet batch of this call is {Bu} "
                                 "(with classifier-free guidance: the negative and the positive halves)")
            out.append(torch.cat([e, e[-B:]], 0) if pag else e)
        return tuple(int(e.shape[1]) if e.ndim == 3 else (int(e.shape[1]), int(e.shape[2])) for e in out), out

    # ------------------------------------------------------------------------------------------------ planning
    def _plan(self, spec):
        """The plan of a PlanSpec (edit_plan.py): the cached one, or recorded now - the least recently used plan then makes room."""
        spec.validate()
        key = spec.key(self.ip_adapters)
        if key in self._plans:
            self._plans[key] = self._plans.pop(key)                   # mark as most recently used
            self.cache_stats["plan_hits"] += 1
            return self._plans[key]
        self.cache_stats["plans_recorded"] += 1
        while len(self._plans) >= self.max_cached_plans:              # evict the least recently used plan and its graphs
            old = self._plans.pop(next(iter(self._plans)))
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            old.rec.close()                                           # graphs and events of the evicted plan
        P = self._plans[key] = record_plan(self, spec)
        return P

    def set_scheduler(self, kind, params=None):
        """`kind` "unipc" | "ddim" | "dpmsolver" | "euler" | "euler_ancestral" | "heun" | "lcm"; `params` = (num_train_timesteps, beta_start,
        beta_end) of the scheduler's configuration (the drop-in scheduler objects accept non-default betas: the engine must tabulate the
        SAME alphas); for "dpmsolver" and the three sigma-space kinds a fourth entry holds the table's options as (key, value) pairs (the
        scheduler object's `table_params()`; missing = diffusers' defaults)."""
        if kind not in ("unipc", "ddim") + OPTION_KINDS:
            raise NotImplementedError(f"scheduler {kind!r} has no coefficient table (UniPC, DDIM, DPM-Solver, Euler, Euler-ancestral, "
                                      "Heun and LCM have)")
        self.scheduler_kind = kind
        if params is not None:
            p = (int(params[0]), float(params[1]), float(params[2]))
            if kind in OPTION_KINDS and len(params) > 3:
                p += (tuple(sorted((str(k), v) for k, v in dict(params[3]).items())),)
            self.scheduler_params = p

    def _scheduler_table(self, n, eta=0.0, timesteps=None):
        """Coefficient tables depend only on (scheduler, its configuration, steps, DDIM eta, caller timesteps)."""
        euler = self.scheduler_kind == "euler"                         # (its timesteps are float32 in the reference: nothing rounds them)
        ts = None if timesteps is None else tuple(float(t) if euler else int(t) for t in timesteps)
        key = (self.scheduler_kind, self.scheduler_params, n, float(eta)) + ((ts,) if ts is not None else ())
        sched = self._sched_cache.get(key)
        if sched is None:
            nt, b0, b1 = self.scheduler_params[:3]
            has_options = self.scheduler_kind in OPTION_KINDS             # (none of these kinds has an eta: their tables take none)
            if ts is not None and self.scheduler_kind not in ("dpmsolver", "euler", "lcm"):
                raise NotImplementedError(f"custom `timesteps` are not tabulated for {self.scheduler_kind}: pass num_inference_steps, or "
                                          "use DPMSolverMultistepScheduler / EulerDiscreteScheduler / LCMScheduler")
            opts = dict(self.scheduler_params[3]) if has_options and len(self.scheduler_params) > 3 else {}
            sched = table_class(self.scheduler_kind)(num_train_timesteps=nt, beta_start=b0, beta_end=b1, **opts)
            if ts is not None:
                sched.set_timesteps(timesteps=list(ts))
            elif eta and not has_options:                                     # (DPM-Solver has no eta: its table takes none)
                sched.set_timesteps(n, eta=float(eta))
            else:
                sched.set_timesteps(n)
            self._sched_cache[key] = sched
        return sched

    def _single_pass(self, single_pass, guidance_off):
        """Whether an edit runs on a single-pass plan (the UNet once per request): the caller's `single_pass`, or by default exactly
        when guidance is off and the scheduler is LCM or the UNet is a distilled one (time_cond_proj_dim) - every other call keeps the plan it
        always had."""
        if single_pass is None:
            return bool(guidance_off and (self.scheduler_kind == "lcm" or self.unet_cfg.time_cond_proj_dim is not None))
        if single_pass and not guidance_off:
            raise ValueError("single_pass=True needs guidance off (guidance_scale <= 1 or do_classifier_free_guidance=False): "
                             "classifier-free guidance reads two UNet outputs per sample")
        return bool(single_pass)

    @staticmethod
    def _step_form(sched, stochastic):
        """(stochastic, third_order) of the plan a table runs on: the noise step for DDIM eta > 0, SDE-DPM-Solver++ and Euler-ancestral,
        the third-order step when a row uses column 13, the plain step otherwise."""
        third = bool((sched.table()[:, 13] != 0).any())
        return bool(stochastic or getattr(sched, "sde", False)), third

    def _check_eta(self, eta):
        """eta > 0 is stochastic DDIM; UniPC and DPM-Solver have no eta (their step takes none, so the reference ignores it: refused
        here)."""
        if eta < 0:
            raise NotImplementedError(f"eta = {eta}: a negative eta is not a DDIM variance")
        if eta != 0.0 and self.scheduler_kind != "ddim":
            raise NotImplementedError(f"eta != 0 is supported with DDIM only (stochastic DDIM); the {self.scheduler_kind} scheduler "
                                      "has no eta")
        return eta > 0

    @staticmethod
    def variance_noise(num_steps, batch, h, w, generator=None, device="cuda", draws=None):
        """The per-step `variance_noise` of a stochastic DDIM edit, [num_steps, batch, 4, h, w] fp32: drawn as DDIMScheduler.step draws
        it (one randn_tensor per step, in step order; a CPU generator on the CPU, a list of generators one sample each, None = the global
        RNG of `device`).  `draws` (an LCM table's): the steps that draw at all - LCMScheduler's last step does not, its slice is zero."""
        return draw_variance_noise(num_steps, (batch, 4, h, w), generator, device, draws)

    def set_weights(self, unet_w=None, blob_w=None):
        """New packed weights (LoRA loaded / unloaded, conv_in edited): every cached plan and its graphs hold the old addresses."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for P in self._plans.values():
            P.rec.close()
        self._plans = {}
        if unet_w is not None:
            self.unet_w = unet_w
        if blob_w is not None:
            self.blob_w = blob_w
            self.feat_dim = self.blob_cfg.in_channels - 5

    def _capture(self, P):
        if P.captured or not self.use_graphs:
            return
        s, side = self._streams()
        # warm-up run outside capture (module loading, attribute setting) then capture each segment once
        torch.cuda.synchronize(self.device)
        P.prologue.run(s)
        for seg in (P.step_active, P.step_inactive):
            with torch.cuda.stream(self.stream):
                P.step_idx.zero_()
            seg.run(s, side, self._extra())
        torch.cuda.synchronize(self.device)
        for seg in (P.step_active, P.step_inactive):
            seg.capture(s, side, self._extra())
        torch.cuda.synchronize(self.device)
        P.captured = True

    def _join_caller(self):
        """The engine works on private non-blocking streams: make them wait for whatever the caller has enqueued on ITS current
        stream (inputs produced by splat_features / Dinov2Model / torch ops are asynchronous) before reading any input."""
        cur = torch.cuda.current_stream(self.device)
        for st in (self.stream, self.side_stream, self.side_stream2):
            st.wait_stream(cur)

    def _streams(self):
        s = self.stream.cuda_stream
        return s, (self.side_stream.cuda_stream if self.two_streams else s)

    def _extra(self):
        return (self.side_stream2.cuda_stream if self.two_streams else self.stream.cuda_stream,)

    def _preview_loop_streams(self):
        return (self.stream, self.side_stream, self.side_stream2) if self.device.type == "cuda" else ()

    # ------------------------------------------------------------------------------------------------ call
    def check_inputs(self, blobnet_conditioning_scale, start, end, num_inference_steps):
        if isinstance(blobnet_conditioning_scale, (list, tuple)):                   # per-request batch (extension)
            if not all(isinstance(v, float) for v in blobnet_conditioning_scale):
                raise TypeError("per-request `blobnet_conditioning_scale` must be a list of `float`.")
        elif not isinstance(blobnet_conditioning_scale, float):                     # pipe:395-396
            raise TypeError("For single blobnet: `blobnet_conditioning_scale` must be type `float`.")
        if start >= end:                                                            # pipe:424-427
            raise ValueError(f"control guidance start: {start} cannot be larger or equal to control guidance end: {end}.")
        if start < 0.0:
            raise ValueError(f"control guidance start: {start} can't be smaller than 0.")
        if end > 1.0:
            raise ValueError(f"control guidance end: {end} can't be larger than 1.0.")
        if num_inference_steps < 1:
            raise ValueError("num_inference_steps must be >= 1")

    def encode_prompt(self, prompt_ids: torch.Tensor, negative_prompt_ids: torch.Tensor, clip_skip: Optional[int] = None):
        """pipe:508-687 after tokenisation: token ids [B, 77] of the prompt and of the negative prompt -> prompt_embeds
        [2B, 77, D] = cat(negative, positive) (pipe:937-949), ready for `__call__`."""
        if self.text_encoder is None:
            raise ValueError("this pipeline was built without a text encoder: pass prompt_embeds, or text_encoder=...")
        if prompt_ids.shape != negative_prompt_ids.shape:
            raise ValueError("prompt_ids and negative_prompt_ids must have the same shape")
        self._join_caller()
        with torch.cuda.stream(self.stream):
            emb = self.text_encoder(torch.cat([negative_prompt_ids, prompt_ids], 0), clip_skip=clip_skip)[0]
        self.stream.synchronize()
        return emb

    # ---- VAE slicing / tiling: forwarded to the VAE; encode_latents / decode_latents / denoise pick them up through vae.encode / vae.decode
    def _vae_switch(self, name, *a):
        if self.vae is None:
            raise ValueError("this pipeline was built without a VAE: there is nothing to slice or tile")
        getattr(self.vae, name)(*a)

    def enable_vae_slicing(self):
        self._vae_switch("enable_slicing")

    def disable_vae_slicing(self):
        self._vae_switch("disable_slicing")

    def enable_vae_tiling(self):
        self._vae_switch("enable_tiling")

    def disable_vae_tiling(self):
        self._vae_switch("disable_tiling")

    def encode_latents(self, image: torch.Tensor, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """pipe:300-309: image [1,3,H,W] in [-1,1] -> posterior sample * scaling_factor, [1,4,H/8,W/8] fp32."""
        if self.vae is None:
            raise ValueError("this pipeline was built without a VAE: pass fg_image_latents / bg_image_latents, or vae=...")
        self._join_caller()
        with torch.cuda.stream(self.stream):
            lat = self.vae.encode(image).latent_dist.sample(generator, scale=self.vae.config.scaling_factor)
        self.stream.synchronize()
        return lat

    def decode_latents(self, latents: torch.Tensor, output_type: str = "pt"):
        """pipe:1132-1146: vae.decode(latents / scaling_factor) then VaeImageProcessor.postprocess with denormalisation
        ((x/2+0.5).clamp(0,1); "pt" = [B,3,H,W] tensor, "np" = [B,H,W,3] numpy)."""
        if self.vae is None:
            raise ValueError("this pipeline was built without a VAE: use output_type='latent', or pass vae=...")
        self._join_caller()
        with torch.cuda.stream(self.stream):
            img = self.vae.decode(latents / self.vae.config.scaling_factor, return_dict=False)[0]
            img = (img / 2 + 0.5).clamp(0, 1)
        self.stream.synchronize()
        return img if output_type == "pt" else img.permute(0, 2, 3, 1).cpu().float().numpy()

    # ------------------------------------------------------------------------------------------------ per-request values
    @staticmethod
    def _listed(**kw):
        """Names of the call arguments that were given per request: a list (for `timesteps`, a list of lists)."""
        out = [k for k, v in kw.items() if k != "timesteps" and isinstance(v, (list, tuple))]
        ts = kw.get("timesteps")
        if ts is not None and len(ts) > 0 and isinstance(ts[0], (list, tuple)):
            out.append("timesteps")
        return out

    def _request_values(self, B, per_request, blobnet_conditioning_scale, req_scales, num_inference_steps, guidance_scale, start, end, eta,
                        timesteps):
        """The values behind every table of a call: (any argument was a list, steps or timestep lists, guidance scales, window starts,
        window ends, etas).  A call with lists (a request batch) has B entries each, validated here - a scalar argument means the same
        for every request; every refusal of such a call is raised here or by the tables built from these values, before a plan is
        recorded.  A call without lists has one entry each: its own arguments (and its eta checked; its callers check the rest)."""
        given = dict(num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, blobnet_control_guidance_start=start,
                     blobnet_control_guidance_end=end, eta=eta, timesteps=timesteps)
        listed = self._listed(**given)
        for k in listed:
            if not per_request:
                raise ValueError(f"{k}: a list of per-request values needs a request batch (fg_image_latents with a leading dimension "
                                 f"B > 1, one entry per request); this call is one edit of B = {B}")
            if len(given[k]) != B:
                raise ValueError(f"{k}: expected {B} values (one per request, B = {B}), got {len(given[k])}")
        for k in ("guidance_scale", "blobnet_control_guidance_start", "blobnet_control_guidance_end"):
            if k in listed and not all(isinstance(v, float) for v in given[k]):
                raise TypeError(f"per-request `{k}` must be a list of `float`.")
        if "num_inference_steps" in listed and not all(isinstance(v, int) and not isinstance(v, bool) for v in num_inference_steps):
            raise TypeError("per-request `num_inference_steps` must be a list of `int`.")
        per = {k: list(v) if k in listed else [v] * (B if listed else 1) for k, v in given.items()}
        if timesteps is not None:                                # (an edit has len(timesteps) steps; num_inference_steps is not used)
            per["num_inference_steps"] = [list(t) for t in per["timesteps"]]
        if listed:
            self.check_inputs(blobnet_conditioning_scale, 0.0, 1.0, 1)          # (the type of the conditioning scales)
        for b in range(B if listed else 0):
            st = per["num_inference_steps"][b]
            try:
                self.check_inputs(req_scales[b], per["blobnet_control_guidance_start"][b], per["blobnet_control_guidance_end"][b],
                                  len(st) if isinstance(st, list) else st)
            except ValueError as e:
                raise ValueError(f"request {b}: {e}") from None
        etas = [float(v) for v in per["eta"]]
        for v in etas:
            self._check_eta(v)
        return bool(listed), per["num_inference_steps"], per["guidance_scale"], per["blobnet_control_guidance_start"], \
            per["blobnet_control_guidance_end"], etas

    def _request_tables(self, steps, etas):
        """The table object of every request - of a call without lists: its one - (cached like any other table) and the step form of the
        plan they run on together: a noise row or a third-order row in any of them puts the whole batch on that form."""
        tables = [self._scheduler_table(len(st) if isinstance(st, list) else st, eta, st if isinstance(st, list) else None)
                  for st, eta in zip(steps, etas)]
        forms = [self._step_form(t, eta > 0) for t, eta in zip(tables, etas)]
        return tables, any(f[0] for f in forms), any(f[1] for f in forms)

    @staticmethod
    def _guidance_on(guidance_scale):
        """Whether classifier-free guidance is on (pipe:494-497): the scale - any of them, in a call with a list - is above 1."""
        if isinstance(guidance_scale, (list, tuple)):
            return all(isinstance(v, (int, float)) for v in guidance_scale) and max(guidance_scale) > 1.0
        return guidance_scale > 1.0

    def _setup(self, B, per_request, blobnet_conditioning_scale, req_scales, num_inference_steps, timesteps, guidance_scale, start, end, eta,
               guidance_off):
        """The EditSetup of a call, scalar or with lists (`req_scales`: the conditioning scale of every image).  With lists every
        request runs its own table rows, timesteps, window and guidance scale, left-aligned in a loop of the longest request's
        evaluations; behind its last row a request is finished: the step leaves it alone and its conditioning scale is 0."""
        requests, steps, gs, starts, ends, etas = self._request_values(B, per_request, blobnet_conditioning_scale, req_scales,
                                                                       num_inference_steps, guidance_scale, start, end, eta, timesteps)
        gs = [1.0 if guidance_off else float(v) for v in gs]
        if requests:                                             # (a request at or below 1 beside guided ones: its eps is its conditional half)
            gs = [max(1.0, v) for v in gs]
        tables, stochastic, third_order = self._request_tables(steps, etas)
        coef, t_rows, evals = stack_request_tables(tables, gs)
        n = max(evals)                                           # network evaluations (Heun: 2 * num_inference_steps - 1, pipe:1025 loops over them)
        per_image = 1 if requests else len(req_scales)           # (a call without lists: the one table and window serve every image)
        keeps = [blobnet_keep(e, s_, e_) + [0.0] * (n - e) for e, s_, e_ in zip(evals * per_image, starts * per_image, ends * per_image)]
        scale_rows = [[sc * k[i] for sc, k in zip(req_scales, keeps)] for i in range(n)]
        return EditSetup(requests, tables, n, stochastic, third_order, tables[0].scales_input, coef if requests else coef[0], t_rows,
                         scale_rows, evals)

    def _check_timestep_cond(self, timestep_cond, B):
        dim = self.unet_cfg.time_cond_proj_dim
        if timestep_cond is not None and dim is None:
            raise ValueError("timestep_cond was given, but this UNet has no time_embedding.cond_proj (config.time_cond_proj_dim is None)")
        if timestep_cond is not None and tuple(timestep_cond.shape) != (B, dim):
            raise ValueError(f"timestep_cond must have shape {(B, dim)} (batch, time_cond_proj_dim), got {tuple(timestep_cond.shape)}")

    @staticmethod
    def _check_variance_noise(S, variance_noise, image_shape, generator=None, compiling=False):
        """A caller's `variance_noise`: only for a plan with a noise step, never beside a generator, [S.n, *image_shape]."""
        if variance_noise is None:
            return
        shape = (S.n,) + tuple(image_shape)
        if compiling:
            if not S.stochastic or tuple(variance_noise.shape) != shape:
                raise ValueError(f"variance_noise needs eta > 0 (or an SDE scheduler) and shape {shape}")
            return
        if not S.stochastic:
            raise ValueError("variance_noise is only used with eta > 0 (DDIM), an SDE-DPM-Solver++, an Euler-ancestral or an LCM "
                             "scheduler")
        if generator is not None:
            raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` or"
                             " `variance_noise` stays `None`.")
        if tuple(variance_noise.shape) != shape:
            steps = "longest request's steps" if S.requests else "steps"
            raise ValueError(f"variance_noise must have shape {shape} ({steps}, batch, 4, h, w), got {tuple(variance_noise.shape)}")

    def _draw_noise(self, S, B, h, w, generator, device):
        """variance_noise [S.n][B][4][h][w], drawn as the reference's scheduler.step draws it (scheduling_ddim.py:455-458 /
        dpmsolver_multistep.py:979-982).  A call with lists and a list of generators (one per request): request b draws what it would
        draw alone - one [1, 4, h, w] slice per step of its own, in step order, skipping the steps its table does not draw for (`draws`,
        LCM) - and zeros behind its end.  Every other call: one [B, 4, h, w] draw per step of the loop (a step draws when any table
        draws in it)."""
        draws = [(list(getattr(t, "draws", None) or [True] * e) + [False] * (S.n - e)) for t, e in zip(S.tables, S.evals)]
        if S.requests and isinstance(generator, list) and len(generator) > 1:
            zero = torch.zeros(1, 4, h, w, dtype=torch.float32, device=device)
            per = [torch.cat([randn_tensor((1, 4, h, w), generator[b], device) if d else zero for d in draws[b]], 0) for b in range(B)]
            return torch.stack(per, 1)
        return self.variance_noise(S.n, B, h, w, generator, device, [any(d[i] for d in draws) for i in range(S.n)])

    @staticmethod
    def _write_tables(P, S, freeu, pag_scales=(0.0, 0.0)):
        """The tables of an edit into the plan's buffers; returns the buffers written (what `compile_plan` saves with their contents).
        `pag_scales` = (pag_scale, pag_adaptive_scale) of a PAG plan: `pag_table` takes _get_pag_scale of every evaluation's timestep."""
        f32 = torch.float32
        if S.requests:
            P.t_rows_blob.copy_(S.t_rows)
            P.t_rows_unet.copy_(S.t_rows if P.single else torch.cat([S.t_rows, S.t_rows], 1))   # (images b and B + b: the CFG pair of request b)
        else:
            P.t_table.copy_(S.t_rows[:, 0])
        P.coef.copy_(S.coef)                                     # (column 11, the guidance scale, is read by the captured step kernel)
        P.scale_table.copy_(torch.tensor(S.scale_rows, dtype=f32).reshape(-1))
        if P.freeu is not None:
            P.freeu.copy_(torch.tensor([float(v) for v in freeu], dtype=f32))
        if P.pag_table is not None:
            P.pag_table.copy_(torch.tensor(pag_mod.pag_table(S.t_rows[:, 0].tolist(), *pag_scales), dtype=f32))
        return [t for t in (P.t_rows_blob, P.t_rows_unet, P.t_table, P.coef, P.scale_table, P.freeu, P.pag_table) if t is not None]

    @staticmethod
    def _mark_stored(P, tables, variance_noise):
        """What a plan file saves with its contents: the constants of the configuration (`tables`) and a `variance_noise` the caller
        gave; without one the buffer is zero-filled workspace (a C host fills it through bc_plan_buffer before each edit)."""
        for t in tables:
            P.rec._workspace.discard(t.untyped_storage().data_ptr())
        if P.variance_noise is not None:
            key = P.variance_noise.untyped_storage().data_ptr()
            if variance_noise is not None:
                P.variance_noise.copy_(variance_noise.to(P.variance_noise.device, torch.float32))
                P.rec._workspace.discard(key)
            else:
                P.variance_noise.zero_()
                P.rec._workspace.add(key)

    def _prompt_layout(self, prompt_embeds, latents, guidance_on, do_classifier_free_guidance, single_pass, pag=False):
        """The layout of `prompt_embeds` and the plan form it asks for: (prompt_embeds as the plan's `ctx` takes them, B, T, ctx_dim,
        single, guidance_off).  `guidance_on`: the call's guidance scale (any of them, in a request batch with its own) is above 1.
        `pag`: the call runs perturbed-attention guidance - with guidance off the UNet batch is [cond | perturbed] whatever `single_pass`
        says (the `single` form of a PAG plan; the duplicated form would be [cond | cond | perturbed] at scale 1), and the prompts of the
        perturbed chunk, a copy of the conditional ones, go behind the others."""
        if do_classifier_free_guidance is None:
            do_classifier_free_guidance = guidance_on and self.unet_cfg.time_cond_proj_dim is None      # (pipe:497)
            if not do_classifier_free_guidance:
                if latents is None:
                    raise ValueError("guidance_scale <= 1 without `latents`: pass do_classifier_free_guidance=False (prompt_embeds = "
                                     "positive prompts only) or =True (negative and positive halves) - the layout cannot be inferred")
                do_classifier_free_guidance = prompt_embeds.shape[0] != latents.shape[0]
        guidance_off = not guidance_on or not do_classifier_free_guidance
        single = True if (pag and guidance_off) else self._single_pass(single_pass, guidance_off)
        if not do_classifier_free_guidance and not single:
            prompt_embeds = torch.cat([prompt_embeds, prompt_embeds], 0)
        B2, T, Dc = prompt_embeds.shape
        if single and not do_classifier_free_guidance:
            B = B2                                                   # the positive prompts only, as the reference holds them
        else:
            if B2 % 2:
                raise ValueError("prompt_embeds must hold the negative and positive halves (classifier-free guidance)")
            B = B2 // 2
            if single:
                prompt_embeds = prompt_embeds[B:]                    # (both halves given, scale <= 1: eps is the positive half's)
        if pag:
            prompt_embeds = torch.cat([prompt_embeds, prompt_embeds[-B:]], 0)
        return prompt_embeds, B, T, Dc, single, guidance_off

    @staticmethod
    def _request_batch(B, fg_image_latents, bg_image_latents, gs_score, dino_feats, blobnet_conditioning_scale, generator):
        """(per_request, Bi, conditioning scale of every image) of a call, with the shape checks of a request batch."""
        per_request = fg_image_latents.dim() == 4 and fg_image_latents.shape[0] > 1
        Bi = B if per_request else 1
        if per_request:
            for name, t_ in (("fg_image_latents", fg_image_latents), ("bg_image_latents", bg_image_latents), ("gs_score", gs_score),
                             ("dino_feats", dino_feats)):
                if t_ is not None and t_.shape[0] != B:
                    raise ValueError(f"request batch: {name} must have leading dimension {B} (one per request), got {t_.shape[0]}")
        req_scales = list(blobnet_conditioning_scale) if isinstance(blobnet_conditioning_scale, (list, tuple)) else \
            [blobnet_conditioning_scale] * Bi
        if len(req_scales) != Bi:
            raise ValueError(f"blobnet_conditioning_scale: expected {Bi} values, got {len(req_scales)}")
        if isinstance(generator, list) and len(generator) != B:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {B}. Make sure the batch size matches the length of the generators.")
        return per_request, Bi, req_scales

    def _fill_inputs(self, P, start, fg_image_latents, bg_image_latents, fg, bg, dino_feats, prompt_embeds, timestep_cond):
        """The per-edit inputs every plan form takes, into the plan's buffers (on the engine's stream)."""
        dev, Bi = self.device, P.Bi
        h, w = P.latents.shape[-2:]
        P.latents.copy_(start)
        P.fg_lat.copy_(fg_image_latents.to(dev, torch.float32).reshape(Bi, 4, h, w))
        P.bg_lat.copy_(bg_image_latents.to(dev, torch.float32).reshape(Bi, 4, h, w))
        P.fg_score.copy_(fg.to(dev, torch.float32).reshape(Bi, h, w))
        P.bg_score.copy_(bg.to(dev, torch.float32).reshape(Bi, h, w))
        if self.feat_dim > 0:
            if dino_feats is None:
                raise ValueError("dino_feats is required (BlobNet conditioning channels)")
            P.feat.copy_(dino_feats.to(dev, torch.float32).reshape(Bi, self.feat_dim))
            if P.collapse:
                P.feat16[:, : self.feat_dim].copy_(P.feat)
        P.ctx.copy_(prompt_embeds.to(dev, torch.float16))
        if P.timestep_cond is not None:
            P.timestep_cond.zero_()
            if timestep_cond is not None:                # (both CFG halves of a sample take the sample's embedding)
                tc = timestep_cond.to(dev, torch.float16)
                P.timestep_cond[:, : tc.shape[1]].copy_(torch.cat([tc] * (P.timestep_cond.shape[0] // tc.shape[0]), 0))

    def _pag_layers(self, pag_scale, pag_adaptive_scale, pag_applied_layers, listed=False):
        """The PAG part of a call's plan key: the sorted block prefixes when perturbed-attention guidance is active, else ()."""
        for name, v in (("pag_scale", pag_scale), ("pag_adaptive_scale", pag_adaptive_scale)):
            if isinstance(v, (list, tuple)):
                raise NotImplementedError(f"{name}: a list of per-request values is not supported - a PAG plan reads one `pag_table`, shared by "
                                          "every request of the batch")
        if isinstance(pag_applied_layers, str):
            pag_applied_layers = (pag_applied_layers,)
        if not pag_mod.is_active(pag_scale, pag_applied_layers):
            return ()
        if listed:
            raise NotImplementedError("perturbed-attention guidance with per-request schedules (a list for num_inference_steps, guidance_scale, "
                                      "the control window, eta or timesteps): bc_pag_scheduler_step reads one coefficient table and one pag_table")
        known = {n[: -len("transformer_blocks.0.attn1")] for n in pag_mod.self_attention_names(self.unet_cfg)}
        layers = tuple(sorted(set(pag_applied_layers)))
        for p in layers:
            if p not in known:
                raise ValueError(f"pag_applied_layers: {p!r} is no self-attention block prefix of this UNet (pag.resolve_layers turns layer ids "
                                 f"such as 'mid' into prefixes such as 'mid_block.attentions.0.')")
        return layers

    @staticmethod
    def _blend_on(blend_image_latents, blend_mask, listed=False):
        """Whether a call is a masked edit: both blend arguments, or neither."""
        if (blend_image_latents is None) != (blend_mask is None):
            raise ValueError("blend_image_latents and blend_mask go together: the latents to keep and where to keep them (pass both or neither)")
        if blend_mask is not None and listed:
            raise NotImplementedError("a masked edit (blend) with per-request schedules (a list for num_inference_steps, guidance_scale, the "
                                      "control window, eta or timesteps): bc_blend_scheduler_step reads one coefficient table and one blend_table")
        return blend_mask is not None

    @staticmethod
    def _check_blend(image, mask, B, h, w):
        """The blend arguments of `denoise` against the edit's (B, h, w): image [1 or B][4][h][w]; mask float [1 or B][1 or none][h][w], or
        uint8 on the device [1 or B][8h][8w].  Returns (image, mask with the optional channel axis dropped)."""
        if not torch.is_tensor(image) or image.ndim != 4 or image.shape[0] not in (1, B) or tuple(image.shape[1:]) != (4, h, w):
            raise ValueError(f"blend_image_latents must be a tensor [1 or {B}][4][{h}][{w}], got "
                             f"{tuple(image.shape) if torch.is_tensor(image) else type(image).__name__}")
        if not torch.is_tensor(mask):
            raise ValueError(f"blend_mask must be a tensor, got {type(mask).__name__}")
        if mask.dtype == torch.uint8:
            if mask.device.type != "cuda":
                raise _lib.BlobCtrlHipError("a uint8 blend_mask is reduced to latent resolution on the device (bc_blend_mask): there is no CPU "
                                            "fallback - pass a device tensor, or a float mask at latent resolution")
            if mask.ndim != 3 or mask.shape[0] not in (1, B) or tuple(mask.shape[1:]) != (8 * h, 8 * w):
                raise ValueError(f"a uint8 blend_mask must be [1 or {B}][{8 * h}][{8 * w}], got {tuple(mask.shape)}")
            return image, mask
        if not mask.is_floating_point():
            raise ValueError(f"blend_mask must be a float mask at latent resolution or a uint8 device mask at image resolution, not {mask.dtype}")
        if mask.ndim == 4 and mask.shape[1] == 1:
            mask = mask[:, 0]
        if mask.ndim != 3 or mask.shape[0] not in (1, B) or tuple(mask.shape[1:]) != (h, w):
            raise ValueError(f"a float blend_mask must be [1 or {B}][1 or none][{h}][{w}], got {tuple(mask.shape)}")
        return image, mask

    def _fill_blend(self, P, noise, image, mask, rows):
        """The per-edit operands of a blend plan, on the engine's (current) stream; one image / mask entry is repeated over the batch."""
        dev, f32 = self.device, torch.float32
        P.blend_noise.copy_(noise.to(dev, f32))
        P.blend_image.copy_(image.to(dev, f32).expand_as(P.blend_image))
        if mask.dtype == torch.uint8:
            m = mask.contiguous()
            n, H, W = m.shape
            with torch.cuda.device(dev):
                _lib.check(self.lib.bc_blend_mask(m.data_ptr(), P.blend_mask.data_ptr(), n, H, W, torch.cuda.current_stream(dev).cuda_stream),
                           "bc_blend_mask")
            m.record_stream(torch.cuda.current_stream(dev))
            if n < P.blend_mask.shape[0]:
                P.blend_mask[1:].copy_(P.blend_mask[:1].expand_as(P.blend_mask[1:]))
        else:
            P.blend_mask.copy_(mask.to(dev, f32).expand_as(P.blend_mask))
        P.blend_table.copy_(rows)

    @torch.no_grad()
    def denoise(self, prompt_embeds: torch.Tensor, fg_image_latents: Optional[torch.Tensor] = None,
                 bg_image_latents: Optional[torch.Tensor] = None, gs_score: torch.Tensor = None, dino_feats: Optional[torch.Tensor] = None, num_inference_steps: int = 50,
                 guidance_scale: float = 7.5, generator: Optional[torch.Generator] = None,
                 latents: Optional[torch.Tensor] = None, blobnet_conditioning_scale: float = 1.0,
                 blobnet_control_guidance_start: float = 0.0, blobnet_control_guidance_end: float = 1.0,
                 output_type: str = "latent", callback_on_step_end=None, trace: Optional[list] = None,
                 teacher_latents: Optional[List[torch.Tensor]] = None, fg_image: Optional[torch.Tensor] = None,
                 bg_image: Optional[torch.Tensor] = None, return_sample: bool = False, eta: float = 0.0,
                 do_classifier_free_guidance: Optional[bool] = None, callback_self=None,
                 variance_noise: Optional[torch.Tensor] = None, timesteps: Optional[List[int]] = None,
                 single_pass: Optional[bool] = None, timestep_cond: Optional[torch.Tensor] = None, freeu=None,
                 ip_adapter_image_embeds: Optional[List[torch.Tensor]] = None, ip_adapter_masks: Optional[List[torch.Tensor]] = None,
                 pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0, pag_applied_layers=None,
                 blend_image_latents: Optional[torch.Tensor] = None, blend_mask: Optional[torch.Tensor] = None):
        """prompt_embeds [2B, T, D] = cat(negative, positive) (pipe:937-949); fg/bg_image_latents [1,4,h,w] already scaled
        by 0.18215 (pipe:300-309); gs_score [1,2,h,w] = (bg, fg) scores (pipe:974); dino_feats [1,1,F] (pipe:982).
        Instead of the latents, `fg_image` / `bg_image` [1,3,8h,8w] in [-1,1] may be given when the pipeline has a VAE.
        Returns the final latents [B,4,h,w] fp32 for `output_type="latent"` (pipe:1143), else the decoded, denormalised
        images ("pt" / "np", pipe:1132-1146).
        eta > 0 (DDIM only): stochastic DDIM.  The variance noise of every step is drawn from `generator` exactly as the reference's
        scheduler.step draws it (after the start latents when those are drawn here; a list = one generator per sample; None = the
        global RNG of the engine's device), or taken from `variance_noise` [num_inference_steps, B, 4, h, w].  It is drawn in fp32 (the
        engine keeps fp32 latents); a reference pipeline running in fp16 would draw fp16 noise.
        With an SDE-DPM-Solver++ scheduler (algorithm_type "sde-dpmsolver++") or the Euler-ancestral scheduler every step draws its noise
        the same way, eta staying 0.  The LCM scheduler draws for every step but the last (scheduling_lcm.py:578): the last slice of the
        plan's `variance_noise` is zero, and the last slice of a caller-given `variance_noise` is ignored (its coefficient is 0).
        `timesteps` (DPM-Solver, Euler and LCM only): the caller's timestep schedule, as the reference's set_timesteps(timesteps=) takes it; the
        edit then has len(timesteps) steps and `num_inference_steps` is not used.
        With a sigma-space scheduler (Euler, Euler-ancestral, Heun) the start latents are multiplied by the table's init_noise_sigma and
        the latents a callback / `teacher_latents` / `trace` see stay in the scheduler's sigma space, as in the reference; only what the
        networks read is divided by sqrt(sigma^2 + 1).  Heun runs 2 * num_inference_steps - 1 network evaluations (`self.timesteps`).
        `single_pass`: with guidance off (guidance_scale <= 1 or do_classifier_free_guidance=False) the reference runs the UNet once per
        request (pipe:1031).  True = do the same: a single-pass plan, the UNet at batch B on the positive prompts only.  False = the
        duplicated plan (both CFG halves hold the positive prompt, effective scale 1).  None = single-pass exactly when guidance is off
        and the scheduler is LCM or the UNet has time_cond_proj_dim; True with guidance on is an error.
        `timestep_cond` [B, time_cond_proj_dim] (a UNet with time_embedding.cond_proj only): `get_guidance_scale_embedding(guidance_scale
        - 1, dim)` of every sample (pipe:987-993); it is per-edit data of the plan, so another scale replays the same graph.  None: the
        UNet runs without the add.
        `freeu` = (s1, s2, b1, b2) or None: FreeU (UNet2DConditionModel.enable_freeu) in up_blocks.0 / up_blocks.1 of the UNet.  As in the
        reference any value of 0.0 or None among the four runs the plain network - the plan every other call uses.  The values are
        per-edit data of the FreeU plan: other values replay the same graph.
        `ip_adapter_image_embeds`: with IP-Adapters loaded (`set_ip_adapters`), one tensor [UNet batch][images][embed_dim] per adapter,
        as the reference's prepare_ip_adapter_image_embeds returns them: the negative and the positive halves with classifier-free
        guidance, one row per UNet image in a request batch too.  Per-edit data of the plan, like `prompt_embeds`.
        `ip_adapter_masks`: one tensor [1][images][H][W] per adapter, float or uint8, on the device or the host (the reference's
        cross_attention_kwargs["ip_adapter_masks"], checked as its processor checks them): the image prompt of image i acts where its mask
        is set.  Every UNet image shares them, in a request batch too, as the reference repeats one mask over the batch.  Per-edit data of
        the masked plan.  Ignored without a loaded adapter, as the reference's adapter-less processors ignore the key.
        `pag_scale`, `pag_adaptive_scale`, `pag_applied_layers`: perturbed-attention guidance (pag_utils.py PAGMixin).  The layers are block
        prefixes already resolved (pag.resolve_layers), e.g. ("mid_block.attentions.0.",).  Active when pag_scale > 0 and there is a layer
        (`do_perturbed_attention_guidance`): the UNet then runs a perturbed copy of every conditional image whose attn1 in those blocks is
        the identity on V, and eps gains pag_scale * (eps_cond - eps_perturbed) - with guidance off it is the only guidance, on the batch
        [cond | perturbed].  pag_adaptive_scale > 0: the scale of a step at timestep t is max(0, pag_scale - pag_adaptive_scale * (1000 -
        t)).  The scales are per-edit data of the PAG plan.  One setting per call, in a request batch too (per-request schedules and
        lists for these arguments are refused); inactive, the call is the call without these arguments.
        `blend_image_latents`, `blend_mask` (both or neither): a masked edit, the four-channel inpainting path of the reference stack
        (pipeline_stable_diffusion_inpaint.py:1272-1285).  After every step the latents where the mask is 0 are replaced by
        `blend_image_latents` noised to the next timestep with the edit's own start noise (the last step: by the image latents themselves),
        inside the step launch, so a callback and `teacher_latents` see blended latents.  blend_image_latents [1 or B][4][h][w], scaled
        like fg / bg_image_latents.  blend_mask: float [1 or B][1 or none][h][w] in [0, 1], 1 = repaint, used as it is (soft values
        blend); or a uint8 DEVICE mask [1 or B][8h][8w], binarised at 128 and read at the top-left pixel of every 8 x 8 cell
        (bc_blend_mask: the reference's mask_processor + prepare_mask_latents).  One entry is repeated over the batch, in a request batch
        too.  Per-edit data of the blend plan: another mask or image replays the same plan and graph.  Refused with per-request schedules
        and with the Heun scheduler.
        A list (one entry per request) for any of num_inference_steps, guidance_scale, the control window, eta or timesteps (a list of
        lists): the requests of a request batch run their own schedules, on the `requests` plan form.  Both kinds of call are one
        set-up (`_setup` -> EditSetup; a call without lists is "one table, shared by every image"), one plan, one run; `self.timesteps`
        is then a list of tensors, one per request."""
        if return_sample:
            # pipe:1052-1061 reads blobnet.conv_norm_out / conv_out, which BlobNetModel does not have (626-tensor schema): dead code
            raise NotImplementedError("return_sample=True is not supported (the reference path dereferences layers BlobNet lacks)")
        listed = self._listed(num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                              blobnet_control_guidance_start=blobnet_control_guidance_start,
                              blobnet_control_guidance_end=blobnet_control_guidance_end, eta=eta, timesteps=timesteps)
        pag = self._pag_layers(pag_scale, pag_adaptive_scale, pag_applied_layers, bool(listed))
        blend = self._blend_on(blend_image_latents, blend_mask, bool(listed))
        if not listed:                                           # (a call without lists refuses its eta before anything else)
            self._check_eta(float(eta))
        if output_type not in ("latent", "pt", "np"):
            raise ValueError(f"output_type must be 'latent', 'pt' or 'np', got {output_type!r}")
        if output_type != "latent" and self.vae is None:
            raise ValueError("this pipeline was built without a VAE: use output_type='latent', or pass vae=...")
        if gs_score is None:
            raise ValueError("gs_score is required")
        if fg_image_latents is None:
            if fg_image is None:
                raise ValueError("give fg_image_latents or fg_image")
            fg_image_latents = self.encode_latents(fg_image)
        if bg_image_latents is None:
            if bg_image is None:
                raise ValueError("give bg_image_latents or bg_image")
            bg_image_latents = self.encode_latents(bg_image)
        if not listed:                                           # (with lists: per request, once the batch is known - `_request_values`)
            self.check_inputs(blobnet_conditioning_scale, blobnet_control_guidance_start, blobnet_control_guidance_end,
                              num_inference_steps if timesteps is None else len(timesteps))
        # pipe:494-497: guidance_scale <= 1 switches classifier-free guidance OFF in the reference (prompt_embeds then holds the
        # positive prompt only and the UNet output is used as is).  The engine keeps its CFG-batch-2 plan: the positive embeddings
        # fill both halves and the effective scale is 1, eps_u + 1 * (eps_c - eps_u) = eps_c.
        # `do_classifier_free_guidance=False` (what the reference derives from guidance_scale <= 1) says explicitly that prompt_embeds
        # holds the positive prompts only; without the flag the layout is inferred from `latents` and refused when ambiguous.
        prompt_embeds, B, T, Dc, single, guidance_off = self._prompt_layout(prompt_embeds, latents, self._guidance_on(guidance_scale),
                                                                            do_classifier_free_guidance, single_pass, pag=bool(pag))
        h, w = fg_image_latents.shape[-2:]
        per_request, Bi, req_scales = self._request_batch(B, fg_image_latents, bg_image_latents, gs_score, dino_feats,
                                                          blobnet_conditioning_scale, generator)
        S = self._setup(B, per_request, blobnet_conditioning_scale, req_scales, num_inference_steps, timesteps, guidance_scale,
                        blobnet_control_guidance_start, blobnet_control_guidance_end, eta, guidance_off)
        self._check_timestep_cond(timestep_cond, B)
        self._check_variance_noise(S, variance_noise, (B, 4, h, w), generator)
        Bu = B if single else 2 * B
        ip, ip_embeds = self._ip_layout(ip_adapter_image_embeds, Bu, B, duplicated=not single and not pag and prompt_embeds.shape[0] == 2 * B and guidance_off,
                                             pag=bool(pag))
        if ip and ip_adapter_masks is not None:
            ip_adapter_masks = ip_masks.check_masks(ip_adapter_masks, [e if isinstance(e, int) else e[0] for e in ip])
        if blend:                                                # (shapes, and Heun's refusal, before a plan is recorded)
            blend_image_latents, blend_mask = self._check_blend(blend_image_latents, blend_mask, B, h, w)
            blend_rows = S.tables[0].blend_rows()
        P = self._plan(S.plan_spec(B, h, w, T, Dc, per_request=per_request, single=single, freeu=freeu_enabled(freeu), ip=ip,
                                   ip_masked=ip_adapter_masks is not None, pag=pag, blend=blend))
        dev = self.device
        self.timesteps = [t.timesteps for t in S.tables] if S.requests else S.tables[0].timesteps
        if latents is None:                                                          # pipe:438-453
            g0 = generator[0] if isinstance(generator, list) else generator
            latents = randn_tensor((B, 4, h, w), generator, g0.device if g0 is not None else "cpu")
        if S.stochastic and variance_noise is None:                                  # (after the latents)
            variance_noise = self._draw_noise(S, B, h, w, generator, dev)
        bg, fg = gs_score.unbind(dim=1)                                              # pipe:974
        self._join_caller()
        with torch.cuda.stream(self.stream):
            sigma = torch.tensor([t.init_noise_sigma for t in S.tables], dtype=torch.float32, device=dev)    # (one, or one per request)
            start = latents.to(dev, torch.float32) * sigma.view(-1, 1, 1, 1)
            self._fill_inputs(P, start, fg_image_latents, bg_image_latents, fg, bg, dino_feats, prompt_embeds, timestep_cond)
            self._write_tables(P, S, freeu, (float(pag_scale), float(pag_adaptive_scale)))
            for buf, e in zip(P.ip_embeds, ip_embeds):
                buf.copy_(e.to(dev, torch.float16).reshape(buf.shape))
            if P.ip_masked:
                ip_masks.fill_plan_masks(P.ip_adapters, ip_adapter_masks, dev)
            if S.stochastic:
                P.variance_noise.copy_(variance_noise.to(dev, torch.float32))
            if blend:                                            # (the noise BEFORE init_noise_sigma: prepare_latents' second value)
                self._fill_blend(P, latents, blend_image_latents, blend_mask, blend_rows)
            P.step_idx.zero_()
            P.hist.zero_()
        if S.requests:
            live = [[i < e for e in S.evals] for i in range(S.n)]
            step_time = lambda i: torch.stack([t.timesteps[min(i, e - 1)] for t, e in zip(S.tables, S.evals)])
        else:
            P.guidance[0] = 1.0 if guidance_off else float(guidance_scale)
            live, step_time = None, lambda i: S.tables[0].timesteps[i].item()
        return self._run(P, S.n, S.active, start, output_type, teacher_latents, callback_on_step_end, callback_self, trace, step_time,
                         live=live)

    def _run(self, P, n, scales, start, output_type, teacher_latents, callback_on_step_end, callback_self, trace, step_time, live=None):
        """Run the edit whose inputs and tables are in the plan's buffers: `scales[i]` != 0 = step i runs BlobNet, `start` = the start
        latents as P.latents holds them, `step_time(i)` = what a callback is given as the timestep of step i.  `live` (a request batch
        with per-request schedules): per step, which requests still run - `teacher_latents` replace those and leave the others alone."""
        dev = self.device
        s, side = self._streams()
        if teacher_latents is None and callback_on_step_end is None and trace is None and not P.captured:
            self.stream.synchronize()
            self._capture(P)
            # captured segments left the step counter advanced by the warm-up runs: reset per-edit state
            with torch.cuda.stream(self.stream):
                P.latents.copy_(start)
                P.step_idx.zero_()
                P.hist.zero_()
        plain = teacher_latents is None and callback_on_step_end is None and trace is None
        if plain and self.use_graphs and self.loop_graph:
            # the WHOLE edit (prologue + n steps) as ONE hipGraph per (plan, active / inactive pattern): one launch per edit; the
            # per-step scalars (timestep, scheduler coefficients, conditioning scale) are read through the device step counter
            key = tuple(v != 0.0 for v in scales)
            g = P.loop_graphs.pop(key, None)
            self.cache_stats["loop_graph_hits" if g is not None else "loop_graph_captures"] += 1
            if g is None:
                torch.cuda.synchronize(self.device)
                while len(P.loop_graphs) >= self.max_loop_graphs:              # least recently used pattern: destroy its graph exec
                    P.rec.destroy_loop_graph(P.loop_graphs.pop(next(iter(P.loop_graphs))))
                segs = [P.prologue] + [P.step_active if a else P.step_inactive for a in key]
                g = P.rec.capture_loop(segs, s, side, self._extra())
            P.loop_graphs[key] = g                                             # (re-inserted: most recently used last)
            _lib.check(self.lib.bc_graph_launch(g, s), "bc_graph_launch")
            return self._result(P, output_type)
        P.prologue.run(s)
        for i in range(n):
            if teacher_latents is not None:
                with torch.cuda.stream(self.stream):
                    if live is None:
                        P.latents.copy_(teacher_latents[i].to(dev, torch.float32))
                    else:                                                          # (entries past a request's end are ignored)
                        for b in (b for b, on in enumerate(live[i]) if on):
                            P.latents[b].copy_(teacher_latents[i][b].to(dev, torch.float32))
            seg = P.step_active if scales[i] != 0.0 else P.step_inactive
            seg.run(s, side, self._extra())
            if trace is not None:
                self.stream.synchronize()
                trace.append((P.eps_guided.clone(), P.latents.clone()))
            if callback_on_step_end is not None:
                self.stream.synchronize()
                ret = callback_on_step_end(callback_self or self, i, step_time(i), {"latents": P.latents})
                if isinstance(ret, dict) and ret.get("latents") is not None and ret["latents"] is not P.latents:
                    with torch.cuda.stream(self.stream):                         # pipe:1112 `latents = callback_outputs.pop(...)`
                        P.latents.copy_(ret["latents"].to(dev, torch.float32))
        return self._result(P, output_type)

    def _result(self, P, output_type):
        """The final latents as a fresh tensor with ordinary stream semantics: the copy is enqueued behind the edit on the engine's
        stream and the CALLER's current stream is made to wait for it - no host synchronisation here, so the next edit's inputs and
        graph launch are enqueued while this edit's tail still runs (a host sync per edit drained the device for ~20 ms of a 550 ms
        edit).  Reading the tensor (`.cpu()`, `torch.cuda.synchronize()`) synchronises as for any torch op."""
        with torch.cuda.stream(self.stream):
            out = P.latents.clone()
        cur = torch.cuda.current_stream(self.device)
        cur.wait_stream(self.stream)
        out.record_stream(cur)                              # (allocated on the engine's stream, consumed on the caller's)
        return out if output_type == "latent" else self.decode_latents(out, output_type)

    @torch.no_grad()
    def __call__(self, prompt_embeds, fg_image_latents=None, bg_image_latents=None, gs_score=None, dino_feats=None, **kw):
        """`denoise(...)`; a plain tensor-level edit (explicit start latents, latent output, no callbacks / traces / images) goes through
        the dispatcher as torch.ops.blobctrl.denoise (ops.py), everything else calls `denoise` directly."""
        plain = {"num_inference_steps", "guidance_scale", "latents", "blobnet_conditioning_scale", "blobnet_control_guidance_start",
                 "blobnet_control_guidance_end", "eta", "variance_noise"}
        if not self._pag_layers(kw.get("pag_scale", 0.0), kw.get("pag_adaptive_scale", 0.0), kw.get("pag_applied_layers")):
            kw = {k: v for k, v in kw.items() if k not in ("pag_scale", "pag_adaptive_scale", "pag_applied_layers")}   # (inactive: today's call)
        sc = kw.get("blobnet_conditioning_scale", 1.0)
        # (ints and anything else take `denoise` directly, which raises the reference's TypeError for them)
        is_list = isinstance(sc, (list, tuple))
        sc_ok = isinstance(sc, float) or (is_list and len(sc) > 0 and all(isinstance(v, float) for v in sc))
        req = ("num_inference_steps", "guidance_scale", "blobnet_control_guidance_start", "blobnet_control_guidance_end")
        if any(isinstance(kw.get(k), (list, tuple)) for k in req + ("eta",)):
            # per-request values: torch.ops.blobctrl.denoise_requests, whose four list arguments hold one entry per request (a scalar is
            # repeated); whatever its schema cannot carry (eta, noise, a malformed list) takes `denoise`, which runs or refuses it
            B = fg_image_latents.shape[0] if torch.is_tensor(fg_image_latents) else 0
            v = {k: list(kw[k]) if isinstance(kw.get(k), (list, tuple)) else [kw.get(k, d)] * B
                 for k, d in zip(req, (50, 7.5, 0.0, 1.0))}
            ok = (B > 1 and all(len(x) == B for x in v.values()) and all(isinstance(x, int) and not isinstance(x, bool) for x in v[req[0]])
                  and all(isinstance(x, float) for k in req[1:] for x in v[k]))
            if (ok and set(kw) <= set(req) | {"latents", "blobnet_conditioning_scale"} and kw.get("latents") is not None
                    and bg_image_latents is not None and gs_score is not None and dino_feats is not None and sc_ok):
                from . import ops
                return torch.ops.blobctrl.denoise_requests(prompt_embeds, fg_image_latents, bg_image_latents, gs_score, dino_feats, kw["latents"],
                                                           v[req[0]], v[req[1]], [float(x) for x in sc] if is_list else [float(sc)] * B,
                                                           v[req[2]], v[req[3]], ops.register(self))
            return self.denoise(prompt_embeds, fg_image_latents, bg_image_latents, gs_score, dino_feats, **kw)
        if (set(kw) <= plain and kw.get("latents") is not None and fg_image_latents is not None and bg_image_latents is not None
                and gs_score is not None and dino_feats is not None and kw.get("guidance_scale", 7.5) > 1.0 and sc_ok):   # (else: denoise raises)
            from . import ops
            return torch.ops.blobctrl.denoise(prompt_embeds, fg_image_latents, bg_image_latents, gs_score, dino_feats, kw["latents"],
                                              int(kw.get("num_inference_steps", 50)), float(kw.get("guidance_scale", 7.5)),
                                              [float(v) for v in sc] if is_list else [float(sc)],
                                              float(kw.get("blobnet_control_guidance_start", 0.0)),
                                              float(kw.get("blobnet_control_guidance_end", 1.0)), ops.register(self), is_list,
                                              float(kw.get("eta", 0.0)), kw.get("variance_noise"))
        return self.denoise(prompt_embeds, fg_image_latents, bg_image_latents, gs_score, dino_feats, **kw)

    def compile_plan(self, path, B, h, w, T, ctx_dim, num_inference_steps, guidance_scale=7.5, blobnet_conditioning_scale=1.0,
                     blobnet_control_guidance_start=0.0, blobnet_control_guidance_end=1.0, eta=0.0, variance_noise=None, timesteps=None,
                     single_pass=None, freeu=None, pag_scale=0.0, pag_adaptive_scale=0.0, pag_applied_layers=None,
                     blend_image_latents=None, blend_mask=None):
        """Write the launch plan of one edit configuration as a relocatable `.bcplan` file for the C plan runtime
        (include/blobctrl_hip.h: bc_plan_load / bc_plan_buffer / bc_step / bc_plan_capture_loop): segments "prologue",
        "step_active", "step_inactive"; packed weights and the scheduler / guidance tables stored with their contents; the per-edit
        inputs are the NAMED buffers latents, fg_lat, bg_lat, fg_score, bg_score (fp32), feat (fp32) / feat16 (fp16, rank-1
        collapse), ctx (fp16 [2B][T][ctx_dim] = cat(negative, positive)); the result is read from `latents`.  Returns the per-step
        segment names (which steps run BlobNet).
        eta > 0 (DDIM): a stochastic plan with the named buffer `variance_noise` [n][B][4][h][w] fp32, saved with `variance_noise`'s
        contents when given (else zero-filled: a C host fills it through bc_plan_buffer before each edit).  An SDE-DPM-Solver++ scheduler
        or the Euler-ancestral scheduler gives the same stochastic plan; a third-order DPM-Solver++ table ends its steps in
        bc_cfg_scheduler_step3; a sigma-space table (Euler, Euler-ancestral, Heun) assembles its inputs with the `_scaled` entry points.
        `timesteps` (DPM-Solver, Euler and LCM only): the caller's schedule, n = len(timesteps).  Heun: 2 * num_inference_steps - 1 steps.
        `single_pass` as in `denoise` (guidance is off for guidance_scale <= 1, and always for a UNet with time_cond_proj_dim): a
        single-pass plan's `ctx` is [B][T][ctx_dim], the positive prompts, and its steps end in bc_scheduler_step_single.  A UNet with
        time_cond_proj_dim adds the named buffer `timestep_cond` (fp16 [B or 2B][pad8(dim)], zero-filled: the host writes the
        guidance-scale embedding of every UNet image into it before an edit).
        `freeu` = (s1, s2, b1, b2) as in `denoise`: a FreeU plan holds six BC_OP_FREEU launches per UNet forward, their basis tables, and
        the named buffer `freeu` (fp32 [4]) saved with these values; a host writes other values into it before an edit.
        A list (one entry per request, as `denoise` takes them; `blobnet_conditioning_scale` a float or a list of B) for any of
        num_inference_steps, guidance_scale, the control window, eta or timesteps compiles the mixed edit of a request batch of B, a
        `.bcplan` of file version 8: the same set-up (`_setup`) with a table per request.  Beside the per-request inputs of a request batch
        (fg_lat, bg_lat, fg_score, bg_score, feat / feat16 with a leading B) it holds, saved with their contents, `coef` [B][nmax][16],
        `t_rows_unet` [nmax][2B or B], `t_rows_blob` [nmax][B] and `scale_table` [nmax][B] instead of `t_table` / `coef` [n][16] /
        `scale_table` [n]; `variance_noise` [nmax][B][4][h][w] as above; the segment names returned are those of the nmax steps."""
        # (the three PAG arguments of `denoise`, taken so that a caller's keywords carry over: active PAG is refused, inactive is no PAG)
        if self._pag_layers(pag_scale, pag_adaptive_scale, pag_applied_layers):
            raise NotImplementedError("a plan with perturbed-attention guidance is recorded and replayed in-process only (bc_attention_identity "
                                      "and bc_pag_scheduler_step are not part of the .bcplan format): run `denoise`")
        if blend_image_latents is not None or blend_mask is not None:    # (the two blend arguments of `denoise`, taken for the same reason)
            raise NotImplementedError("a plan of a masked edit (blend) is recorded and replayed in-process only (bc_blend_scheduler_step is "
                                      "not part of the .bcplan format): run `denoise`")
        if self.ip_adapters:
            raise NotImplementedError("a plan with IP-Adapters loaded is recorded and replayed in-process only (bc_attention_ip is not part of "
                                      "the .bcplan format): unload them, or run `denoise`")
        listed = bool(self._listed(num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                   blobnet_control_guidance_start=blobnet_control_guidance_start,
                                   blobnet_control_guidance_end=blobnet_control_guidance_end, eta=eta, timesteps=timesteps))
        guidance_off = not self._guidance_on(guidance_scale) or self.unet_cfg.time_cond_proj_dim is not None      # (pipe:497)
        single = self._single_pass(single_pass, guidance_off)
        Bi = B if listed else 1
        req_scales = list(blobnet_conditioning_scale) if isinstance(blobnet_conditioning_scale, (list, tuple)) else \
            [blobnet_conditioning_scale] * Bi
        if len(req_scales) != Bi:
            raise ValueError(f"blobnet_conditioning_scale: expected {Bi} values, got {len(req_scales)}")
        # (a plan without lists stores the guidance scale it was given, at or below 1 too: what a C host's two `ctx` halves are mixed by)
        S = self._setup(B, listed and B > 1, blobnet_conditioning_scale, req_scales, num_inference_steps, timesteps, guidance_scale,
                        blobnet_control_guidance_start, blobnet_control_guidance_end, eta, guidance_off and listed)
        self._check_variance_noise(S, variance_noise, (B, 4, h, w), compiling=True)
        P = self._plan(S.plan_spec(B, h, w, T, ctx_dim, per_request=S.requests, single=single, freeu=freeu_enabled(freeu)))
        self._mark_stored(P, self._write_tables(P, S, freeu), variance_noise)
        P.rec.save(path)
        return S.segments

    # convenience for bench / tests ------------------------------------------------------------------
    def plan_for(self, B, h, w, T, ctx_dim, nsteps, per_request=False, stochastic=False, third_order=False, scaled=False, single=False,
                 freeu=False, requests=False, ip=(), ip_masked=False, pag=()):
        return self._plan(PlanSpec(B, h, w, T, ctx_dim, nsteps, per_request, stochastic, third_order, scaled, single, freeu, requests, ip, ip_masked, pag))


def _is_device_image(image):
    """uint8 [H][W][3] tensor: pixels as `blobctrl_amd.edit_inputs` leaves them on the device (a CPU one is refused there: no CPU fallback)."""
    return torch.is_tensor(image) and image.dtype == torch.uint8 and image.ndim == 3 and image.shape[-1] == 3


# ======================================================================================================================
# The reference's pipeline surface: same constructor keywords, same __call__ signature, same error behaviour,
# `.images` output - so that scripts/blobctrl_inference.py:191-205 runs unchanged on the MI355X modules.
# ======================================================================================================================
class StableDiffusionBlobNetPipelineOutput:
    """pipeline_blobnet.py:1163-1166 (`images`, `nsfw_content_detected`; tuple-like for `return_dict=False` callers)."""

    def __init__(self, images, nsfw_content_detected=None):
        self.images, self.nsfw_content_detected = images, nsfw_content_detected

    def __iter__(self):
        return iter((self.images, self.nsfw_content_detected))

    def __getitem__(self, i):
        return (self.images, self.nsfw_content_detected)[i]


class StableDiffusionBlobNetPipeline(_PreviewVAE):
    """Drop-in for blobctrl/pipelines/pipeline_blobnet.py:StableDiffusionBlobNetPipeline on MI355X.

    Components (pipe:206-243): `vae` = blobctrl_amd.vae.AutoencoderKL, `unet` / `blobnet` = blobctrl_amd.modules shells (any LoRA is
    merged when the UNet is packed), `tokenizer` = any callable with the CLIPTokenizer call contract (host side), `text_encoder` =
    blobctrl_amd.clip_text.CLIPTextModel, `scheduler` = blobctrl_amd.schedulers.UniPCMultistepScheduler | DDIMScheduler | DPMSolverMultistepScheduler | EulerDiscreteScheduler |
    EulerAncestralDiscreteScheduler | HeunDiscreteScheduler | LCMScheduler,
    `dinov2_processor` = image_processor.Dinov2ImageProcessor (or the HF processor), `dinov2` = blobctrl_amd.dinov2.Dinov2Model.
    The denoise loop itself is the captured-plan engine (BlobCtrlEngine): the module shells are not called per step."""

    _callback_tensor_inputs = ["latents", "image_embeds", "negative_image_embeds"]

    def __init__(self, vae, unet, tokenizer, text_encoder, blobnet, scheduler, safety_checker=None, dinov2_processor=None,
                 dinov2=None, requires_safety_checker: bool = False, use_graphs: bool = True, image_encoder=None, feature_extractor=None,
                 pag_applied_layers: Union[str, List[str]] = "mid"):
        from .image_processor import Dinov2ImageProcessor, VaeImageProcessor
        from .schedulers import TableScheduler
        if safety_checker is not None:
            raise NotImplementedError("the reference disables the safety checker (pipe:1133-1135); pass safety_checker=None")
        if not isinstance(scheduler, TableScheduler):
            raise TypeError("scheduler must be blobctrl_amd.schedulers.UniPCMultistepScheduler, DDIMScheduler, "
                            "DPMSolverMultistepScheduler, EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, HeunDiscreteScheduler "
                            "or LCMScheduler")
        self.vae, self.unet, self.blobnet, self.tokenizer, self.text_encoder = vae, unet, blobnet, tokenizer, text_encoder
        self.dinov2, self.dinov2_processor = dinov2, dinov2_processor if dinov2_processor is not None else Dinov2ImageProcessor()
        self.safety_checker = None
        # optional components, as in the reference (`_optional_components`): the CLIP vision tower of an IP-Adapter and its processor
        # (blobctrl_amd.clip_vision.CLIPVisionModelWithProjection, image_processor.CLIPImageProcessor); load_ip_adapter can load both
        self.image_encoder, self.feature_extractor = image_encoder, feature_extractor
        self._loaded_image_encoder = False      # load_ip_adapter loaded the encoder: unload_ip_adapter drops it again
        self._zero_image_states = {}            # (encoder, shape) -> hidden_states[-2] of an all-zero image: weights and shape only
        self.device = unet.device
        self._use_graphs = use_graphs
        self._engine, self._engine_versions = None, None
        self._scheduler = scheduler
        nblocks = len(getattr(vae.config, "block_out_channels", (0, 0, 0, 0))) if vae is not None else 4
        self.vae_scale_factor = 2 ** (nblocks - 1)                                                  # pipe:241
        self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor, do_convert_rgb=True)    # pipe:242
        self._guidance_scale, self._clip_skip, self._num_timesteps = 7.5, None, 0
        self._pag_scale, self._pag_adaptive_scale = 0.0, 0.0
        self.set_pag_applied_layers(pag_applied_layers)               # (the PAG pipelines' constructor argument and default: "mid")

    # ---- perturbed-attention guidance (D/pipelines/pag/pag_utils.py PAGMixin: the same names, defaults and errors)
    def set_pag_applied_layers(self, pag_applied_layers: Union[str, List[str]]):
        """The self-attention layers PAG perturbs: a layer name, a block name ("mid", "down_blocks.1"), a regex ("up_blocks.(1|2)") or a
        list of them; ValueError for anything that is no string.  Names are matched against the UNet when a call uses them."""
        self.pag_applied_layers = pag_mod.normalize_layers(pag_applied_layers)

    @property
    def pag_scale(self) -> float:
        return self._pag_scale

    @property
    def pag_adaptive_scale(self) -> float:
        return self._pag_adaptive_scale

    @property
    def do_pag_adaptive_scaling(self) -> bool:
        return self._pag_adaptive_scale > 0 and self._pag_scale > 0 and len(self.pag_applied_layers) > 0

    @property
    def do_perturbed_attention_guidance(self) -> bool:
        return self._pag_scale > 0 and len(self.pag_applied_layers) > 0

    # ---- construction as the scripts do it (inf:260-279)
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, unet=None, blobnet=None, dinov2_processor=None, dinov2=None,
                        vae=None, text_encoder=None, tokenizer=None, scheduler=None, safety_checker=None, torch_dtype=None,
                        device="cuda:0", image_encoder=None, feature_extractor=None, pag_applied_layers="mid", **_ignored):
        """`StableDiffusionBlobNetPipeline.from_pretrained(sd15_path, unet=, blobnet=, torch_dtype=, dinov2_processor=, dinov2=)`
        (inf:260-267; D/pipelines/pipeline_utils.py from_pretrained): components that are not passed are built from the sub-folders
        of the model directory - `vae/`, `text_encoder/`, `tokenizer/` (vocab.json + merges.txt), `scheduler/scheduler_config.json`,
        `unet/` - with this package's classes.  `torch_dtype` is accepted and ignored (the kernels compute in fp16 / fp32
        accumulate); the safety checker stays off as in the reference (pipe:1133-1135)."""
        import os
        from .clip_text import CLIPTextModel
        from .modules import UNet2DConditionModel
        from .schedulers import scheduler_from_config_dir
        from .vae import AutoencoderKL
        root = pretrained_model_name_or_path
        if not os.path.isdir(root):
            raise FileNotFoundError(f"{root}: not a local model directory (there is no hub download here)")
        sub = lambda name: os.path.isdir(os.path.join(root, name))
        dev = str(unet.device) if unet is not None else device
        if unet is None:
            unet = UNet2DConditionModel.from_pretrained(root, subfolder="unet", device=dev)
        if blobnet is None:
            raise ValueError("blobnet= is required (the SD-1.5 directory does not hold one; inf:252)")
        if vae is None and sub("vae"):
            vae = AutoencoderKL.from_pretrained(root, subfolder="vae", device=dev)
        if text_encoder is None and sub("text_encoder"):
            text_encoder = CLIPTextModel.from_pretrained(root, subfolder="text_encoder", device=dev)
        if tokenizer is None and sub("tokenizer"):
            from .clip_tokenizer import CLIPTokenizer
            tokenizer = CLIPTokenizer.from_pretrained(root, subfolder="tokenizer")
        if scheduler is None:
            scheduler = scheduler_from_config_dir(os.path.join(root, "scheduler"))
        return cls(vae=vae, unet=unet, tokenizer=tokenizer, text_encoder=text_encoder, blobnet=blobnet, scheduler=scheduler,
                   safety_checker=None, dinov2_processor=dinov2_processor, dinov2=dinov2, image_encoder=image_encoder,
                   feature_extractor=feature_extractor, pag_applied_layers=pag_applied_layers)

    def splat_features_from_scores(self, scores: torch.Tensor, features: torch.Tensor, size: Optional[int],
                                   channels_last: bool = True) -> torch.Tensor:
        """pipe:706-721 as a callable (the loop itself folds its rank-1 case into bc_assemble_input): float64 / float32 scores on the
        GPU, one bc_splat_from_scores launch."""
        from .splat import splat_features_from_scores
        return splat_features_from_scores(scores, features, size, channels_last=channels_last)

    @property
    def engine(self) -> BlobCtrlEngine:
        """The captured-plan loop engine over the CURRENT packed weights of `unet` / `blobnet`: built on first use, re-pointed (plans
        dropped) whenever a module's host weights changed (LoRA loaded / unloaded, conv_in surgery)."""
        versions = (self.unet._version, self.blobnet._version)
        if self._scheduler.kind is None:
            # the PNDM configuration holder a checkpoint directory ships (inf:276 replaces it): no loop engine behind it
            raise NotImplementedError(f"{type(self._scheduler).__name__} is a configuration holder here: assign a UniPCMultistepScheduler / "
                                      "DDIMScheduler (e.g. UniPCMultistepScheduler.from_config(pipe.scheduler.config)) before running the loop")
        if self._engine is None:
            kind = self._scheduler.kind
            self._engine = BlobCtrlEngine(self.unet.weights, self.blobnet.weights, self.unet.trunk_config, self.blobnet.trunk_config,
                                          device=str(self.unet.device), scheduler=kind, use_graphs=self._use_graphs, vae=self.vae,
                                          text_encoder=self.text_encoder)
            self._engine_versions = versions
        elif versions != self._engine_versions:
            self._engine.unet_cfg, self._engine.blob_cfg = self.unet.trunk_config, self.blobnet.trunk_config
            self._engine.set_weights(None, None)                     # frees the plans that point into the old arenas first
            self._engine.unet_w = self._engine.blob_w = None
            self._engine.set_weights(self.unet.weights, self.blobnet.weights)
            self._engine_versions = versions
        ip_version = self.unet.__dict__.get("_ip_version", 0)         # (the UNet's adapters were loaded or unloaded since: plans with them go)
        if getattr(self._engine, "_ip_version", 0) != ip_version:
            self._engine.set_ip_adapters(self.unet.__dict__.get("ip_adapters"))
            self._engine._ip_version = ip_version
        if self._scheduler.kind is not None:
            self._engine.set_scheduler(self._scheduler.kind, self._scheduler.table_params()
                                       if hasattr(self._scheduler, "table_params") else None)
        return self._engine

    def _preview_loop_streams(self):
        return self._engine._preview_loop_streams() if self._engine is not None else ()

    # ---- attribute plumbing the scripts touch (inf:276-279)
    @property
    def scheduler(self):
        return self._scheduler

    @scheduler.setter
    def scheduler(self, s):
        from .schedulers import TableScheduler
        if not isinstance(s, TableScheduler):
            raise TypeError("scheduler must be blobctrl_amd.schedulers.UniPCMultistepScheduler, DDIMScheduler, "
                            "DPMSolverMultistepScheduler, EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, HeunDiscreteScheduler "
                            "or LCMScheduler")
        self._scheduler = s

    def to(self, *a, **k):
        return self

    def set_progress_bar_config(self, **k):
        pass

    # ---- LoRA (D/loaders/lora_pipeline.py:60-117 -> D/loaders/unet.py:271-340, load_lora_into_text_encoder): one registry per model
    # (weights.LoraAdapters), merged when the UNet is packed / when the text encoder's device tensors are filled
    def _lora_models(self):
        return [m for m in (self.unet, self.text_encoder) if hasattr(m, "_adapters")]

    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, adapter_name=None, weight_name=None, **kwargs):
        """`pipeline.load_lora_weights(unet_lora_path, adapter_name="default")` (inf:270-273).  A directory (with
        `pytorch_lora_weights.safetensors` or `weight_name`), a .safetensors file, or a state dict, with diffusers keys or kohya /
        sd-scripts keys (`lora_unet_*` / `lora_te_*`, e.g. the published LCM-LoRA).  Keys under `unet.` go to the UNet
        (lora_pipeline.py:102-110), keys under `text_encoder.` to the text encoder, both under the same adapter name."""
        import os
        from .checkpoint import _model_file, read_safetensors, split_lora_state_dict
        src = pretrained_model_name_or_path_or_dict
        if isinstance(src, dict):
            raw, what = src, "state dict"
        else:
            what = os.path.join(src, weight_name) if weight_name and os.path.isdir(src) else src
            raw = read_safetensors(_model_file(what))
        mods = lambda sd, pre: [pre + k[: -len(".weight")] for k, v in sd.items() if k.endswith(".weight") and v.ndim >= 2]
        te_sd = getattr(self.text_encoder, "_sd", None)
        unet_part, te_part = split_lora_state_dict(raw, mods(self.unet._sd, "") if self.unet._sd is not None else None,
                                                   mods(te_sd, "text_model.") if te_sd is not None else None, what=str(what))
        if te_part is not None and te_sd is None:
            raise ValueError(f"{what} holds text-encoder LoRA tensors, but this pipeline was built without a text encoder "
                             "(text_encoder=None): it cannot apply them")
        name = adapter_name
        if name is None:
            name = f"default_{max(len(m._adapters) for m in self._lora_models())}"
        parts = [(m, part) for m, part in ((self.unet, unet_part), (self.text_encoder, te_part)) if part is not None]
        done = []
        try:
            for m, (lora, alphas) in parts:
                m.load_lora_adapter(lora, alphas, adapter_name=name)
                done.append(m)
        except Exception:                                       # (one adapter name means the same file in both models, or in neither)
            for m in done:
                m.delete_adapters([name])
            raise

    def set_adapters(self, adapter_names, adapter_weights=None):
        """`pipeline.set_adapters(["default"])` (inf:274): the active adapters and their weights (merged on the next call), in the UNet
        and in the text encoder; a model that does not hold one of the named adapters keeps the others."""
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        ws = adapter_weights if isinstance(adapter_weights, (list, tuple)) else [adapter_weights] * len(names)
        if len(ws) != len(names):
            raise ValueError(f"Length of adapter names {len(names)} is not equal to the length of their weights {len(ws)}.")
        known = set().union(*(m._adapters for m in self._lora_models()))
        if set(names) - known:
            raise ValueError(f"Adapter name(s) {set(names) - known} not in the list of present adapters: {known}.")
        for m in self._lora_models():
            mine = [(n, w) for n, w in zip(names, ws) if n in m._adapters]
            m.set_adapters([n for n, _ in mine], [w for _, w in mine])

    def fuse_lora(self, *a, **k):
        """Adapters are always merged into the packed weights: nothing to do."""

    def unload_lora_weights(self):
        for m in self._lora_models():
            m.unload_lora()

    def delete_adapters(self, adapter_names):
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        for m in self._lora_models():
            m.delete_adapters([n for n in names if n in m._adapters])

    def disable_lora(self):
        for m in self._lora_models():
            m.disable_lora()

    def enable_lora(self):
        for m in self._lora_models():
            m.enable_lora()

    def get_list_adapters(self):
        """{"unet": [names], "text_encoder": [names]}: the models that hold adapters (lora_base.py get_list_adapters)."""
        held = {"unet": self.unet, "text_encoder": self.text_encoder}
        return {k: list(m._adapters) for k, m in held.items() if getattr(m, "_adapters", None)}

    # ---- FreeU (D/pipelines/pipeline_utils.py:1905-1929, StableDiffusionMixin): forwarded to the UNet; the loop engine reads the state there
    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """Enables the FreeU mechanism (https://arxiv.org/abs/2309.11497): s1 / s2 attenuate the skip features of stage 1 / 2, b1 / b2
        amplify the backbone features."""
        if not hasattr(self, "unet") or self.unet is None:
            raise ValueError("The pipeline must have `unet` for using FreeU.")
        self.unet.enable_freeu(s1=s1, s2=s2, b1=b1, b2=b2)

    # ---- IP-Adapter (IPAdapterMixin, D/loaders/ip_adapter.py: load_ip_adapter / set_ip_adapter_scale / unload_ip_adapter)
    def load_ip_adapter(self, pretrained_model_name_or_path_or_dict, subfolder=None, weight_name=None, image_encoder_folder=None):
        """One adapter or a list (of paths, of dicts, or of weight names under one path): the original {"image_proj", "ip_adapter"} dict
        or a `.safetensors` file at path[/subfolder]/weight_name.  Every scale starts at 1.0.
        `image_encoder_folder` (default None: nothing is loaded, the call takes `ip_adapter_image_embeds`): with a path source and no
        `image_encoder` on the pipeline yet, CLIPVisionModelWithProjection is loaded from path/subfolder/folder - a folder that
        contains "/" is taken relative to path, as in the reference (D/loaders/ip_adapter.py:197-216) - and a pipeline without a
        `feature_extractor` gets a CLIPImageProcessor of the encoder's image size (:223-227).  A dict source with a folder is the
        reference's ValueError."""
        import os
        first = pretrained_model_name_or_path_or_dict[0] if isinstance(pretrained_model_name_or_path_or_dict, (list, tuple)) else \
            pretrained_model_name_or_path_or_dict
        if image_encoder_folder is not None and getattr(self, "image_encoder", None) is None:
            if isinstance(first, dict):
                raise ValueError("`image_encoder` cannot be loaded because `pretrained_model_name_or_path_or_dict` is a state dict.")
            from .clip_vision import CLIPVisionModelWithProjection
            sub0 = subfolder[0] if isinstance(subfolder, (list, tuple)) else subfolder
            folder = image_encoder_folder if image_encoder_folder.count("/") else os.path.join(*[x for x in (sub0, image_encoder_folder) if x])
            self.image_encoder = CLIPVisionModelWithProjection.from_pretrained(os.fspath(first), subfolder=folder, device=str(self.device))
            self._loaded_image_encoder = True
        if getattr(self, "image_encoder", None) is not None and getattr(self, "feature_extractor", None) is None:
            from .image_processor import CLIPImageProcessor
            size = self.image_encoder.config.image_size
            self.feature_extractor = CLIPImageProcessor(size=size, crop_size=size)
        many = isinstance(weight_name, (list, tuple)) or isinstance(pretrained_model_name_or_path_or_dict, (list, tuple))
        n = len(weight_name) if isinstance(weight_name, (list, tuple)) else len(pretrained_model_name_or_path_or_dict) if many else 1
        as_list = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n
        srcs = []
        for src, sub, name in zip(as_list(pretrained_model_name_or_path_or_dict), as_list(subfolder), as_list(weight_name)):
            if not isinstance(src, dict):
                src = os.path.join(*[x for x in (os.fspath(src), sub, name) if x])
            srcs.append(src)
        self.unet.load_ip_adapter_weights(srcs)                       # (`engine` takes them over on its next use)

    def ip_adapter_scale_lists(self, scale):
        """What `set_ip_adapter_scale(scale)` assigns: one list per adapter with a value per attn2 processor in `attn_processors` order
        (None where the argument leaves a processor as it is).  `scale`: a float or a per-block dict ({"down": {"block_2": [0.0, 1.0]},
        "up": ..., "mid": ...}; what a dict does not name is 0.0), or a list of those with one entry per adapter (a single entry serves
        every adapter) - D/loaders/ip_adapter.py:245-295 with _maybe_expand_lora_scales(default_scale=0.0)."""
        from .weights import ip_attn2_prefixes
        ads = self.unet.__dict__.get("ip_adapters") or []
        configs = list(scale) if isinstance(scale, list) else [scale]
        if len(configs) != len(ads):
            raise ValueError(f"Cannot assign {len(configs)} scale_configs to {len(ads)} IP-Adapter.")
        cfg = self.unet.trunk_config
        nb, per = len(cfg.block_out_channels), {"down": cfg.layers_per_block, "up": cfg.layers_per_block + 1}
        with_tf = {"down": list(range(nb - 1)), "up": list(range(1, nb))}             # SD layout: the last down / first up block has none
        prefixes = ip_attn2_prefixes(self.unet._sd.keys()) if self.unet._sd is not None else list(ads[0]["kv"])
        out = []
        for c in configs:
            if not isinstance(c, dict):
                out.append([float(c)] * len(prefixes))
                continue
            names = {}
            mid = c.get("mid", 0.0)
            if isinstance(mid, list):
                if len(mid) != 1:
                    raise ValueError(f"Expected 1 scales for mid, got {len(mid)}.")
                mid = mid[0]
            names["mid_block.attentions.0."] = mid
            for ud in ("up", "down"):
                blocks = c.get(ud, 0.0)
                if not isinstance(blocks, dict):
                    blocks = {f"block_{i}": blocks for i in with_tf[ud]}
                for i in with_tf[ud]:
                    v = blocks.get(f"block_{i}", 0.0)
                    v = [v] * per[ud] if not isinstance(v, list) else v * per[ud] if len(v) == 1 else v
                    if len(v) != per[ud]:
                        raise ValueError(f"Expected {per[ud]} scales for {ud}.block_{i}, got {len(v)}.")
                    for j, x in enumerate(v):
                        names[f"{ud}_blocks.{i}.attentions.{j}."] = x
                extra = [k for k in blocks if k not in {f"block_{i}" for i in with_tf[ud]}]
                if extra:
                    raise ValueError(f"Can't set scale for layer {ud}.{extra[0]}: this UNet has no attention there.")
            out.append([next((float(v) for k, v in names.items() if bp.startswith(k)), None) for bp in prefixes])
        return out

    def set_ip_adapter_scale(self, scale):
        """The reference's set_ip_adapter_scale: see `ip_adapter_scale_lists`.  Only the adapters' device scale tables are rewritten -
        recorded plans and whole-edit graphs read them on replay."""
        ads = self.unet.__dict__.get("ip_adapters") or []
        for ad, vals in zip(ads, self.ip_adapter_scale_lists(scale)):
            old = ad["scales"].cpu().tolist()
            ad["scales"].copy_(torch.tensor([o if v is None else v for o, v in zip(old, vals)], dtype=torch.float32))

    def unload_ip_adapter(self):
        """D/loaders/ip_adapter.py unload_ip_adapter: the UNet goes back to its adapter-less state, and an image encoder that
        load_ip_adapter loaded is dropped with the processor made for it (components the caller passed stay)."""
        self.unet.unload_ip_adapter()
        if getattr(self, "_loaded_image_encoder", False):
            self.image_encoder, self.feature_extractor, self._loaded_image_encoder = None, None, False
            self._zero_image_states = {}

    def encode_image(self, image, device, num_images_per_prompt, output_hidden_states=None):
        """pipe:248-270.  The reference's copy reads `self.clip_processor`, an attribute its class never sets; this reads
        `self.feature_extractor`, as StableDiffusionPipeline.encode_image - the function it was copied from - does.
        `image`: anything but a tensor goes through the processor on the host; a uint8 device image [H][W][3] (judged as
        `_is_device_image` judges `fg_image`) takes resample.clip_pixel_values, the same pixels without a host copy; a float tensor is
        taken as pixel values.  Returns (embeds, negative embeds): image_embeds and zeros, or with `output_hidden_states`
        hidden_states[-2] of the image and of an all-zero image.  The latter depends on the weights and the shape only: it is computed
        once per encoder and shape and kept."""
        if getattr(self, "image_encoder", None) is None:
            raise ValueError("encode_image needs an `image_encoder` (load_ip_adapter(..., image_encoder_folder=) or the component)")
        enc = self.image_encoder
        if _is_device_image(image) and image.is_cuda:
            from .resample import clip_pixel_values
            image = clip_pixel_values(image, self.feature_extractor)
        elif not torch.is_tensor(image) or image.dtype == torch.uint8:
            if torch.is_tensor(image):
                image = image.cpu().numpy()
            image = self.feature_extractor(image, return_tensors="pt").pixel_values
        image = image.to(device=device, dtype=torch.float32)
        if output_hidden_states:
            hidden = enc(image, output_hidden_states=True).hidden_states[-2].repeat_interleave(num_images_per_prompt, dim=0)
            key = (id(enc), tuple(image.shape))
            if key not in self._zero_image_states:
                self._zero_image_states[key] = enc(torch.zeros_like(image), output_hidden_states=True).hidden_states[-2]
            return hidden, self._zero_image_states[key].repeat_interleave(num_images_per_prompt, dim=0)
        embeds = enc(image).image_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        return embeds, torch.zeros_like(embeds)

    def prepare_ip_adapter_image_embeds(self, ip_adapter_image, ip_adapter_image_embeds, device, num_images_per_prompt,
                                        do_classifier_free_guidance):
        """D/pipelines/stable_diffusion/pipeline_stable_diffusion.py:508-552.  Given embeddings: with classifier-free guidance each
        tensor is chunked into its (negative, positive) halves, each half is repeated num_images_per_prompt times, and the halves are
        concatenated again.  Given `ip_adapter_image` - one image or a list of images per loaded adapter - and an `image_encoder`: every
        image goes through encode_image (hidden states for every adapter that is not a base one), an adapter's images are stacked to
        [1][images][...], and the negative half goes in front under classifier-free guidance."""
        if ip_adapter_image_embeds is None:
            if getattr(self, "image_encoder", None) is None:
                raise NotImplementedError("`ip_adapter_image` needs a CLIP vision tower, which this pipeline does not have: pass `ip_adapter_image_embeds`")
            ads = self.unet.__dict__.get("ip_adapters") or []
            images = ip_adapter_image if isinstance(ip_adapter_image, list) else [ip_adapter_image]
            if len(images) != len(ads):
                raise ValueError(f"`ip_adapter_image` must have same length as the number of IP Adapters. Got {len(images)} images and "
                                 f"{len(ads)} IP Adapters.")
            ip_adapter_image_embeds = []
            for per_adapter, ad in zip(images, ads):
                hidden = ad.get("layout", "base") != "base"
                pairs = [self.encode_image(im, device, 1, hidden) for im in (per_adapter if isinstance(per_adapter, (list, tuple)) else [per_adapter])]
                pos, neg = torch.cat([p for p, _ in pairs], 0)[None], torch.cat([n for _, n in pairs], 0)[None]
                ip_adapter_image_embeds.append(torch.cat([neg, pos], 0) if do_classifier_free_guidance else pos)
        out = []
        for e in ip_adapter_image_embeds:
            if do_classifier_free_guidance:
                if e.shape[0] % 2:
                    raise ValueError(f"with classifier-free guidance `ip_adapter_image_embeds` hold the negative and the positive halves; got {e.shape[0]} rows")
                neg, pos = e.chunk(2)
                e = torch.cat([torch.cat([neg] * num_images_per_prompt, 0), torch.cat([pos] * num_images_per_prompt, 0)], 0)
            else:
                e = torch.cat([e] * num_images_per_prompt, 0)
            out.append(e.to(device))
        return out

    def disable_freeu(self):
        """Disables the FreeU mechanism if enabled."""
        self.unet.disable_freeu()

    # ---- VAE slicing / tiling (D/pipelines/pipeline_utils.py:1873-1903, StableDiffusionMixin): forwarded to the VAE, which the engine shares
    def enable_vae_slicing(self):
        """Sliced VAE encode / decode: a batch goes through the VAE one sample at a time."""
        self.vae.enable_slicing()

    def disable_vae_slicing(self):
        """Back to encoding / decoding a batch in one step."""
        self.vae.disable_slicing()

    def enable_vae_tiling(self):
        """Tiled VAE encode / decode: inputs above the VAE's tile size are processed as overlapping tiles and blended."""
        self.vae.enable_tiling()

    def disable_vae_tiling(self):
        """Back to encoding / decoding an image in one step."""
        self.vae.disable_tiling()

    def get_active_adapters(self):
        out = []
        for m in self._lora_models():
            out += [n for n in m.active_adapters() if n not in out]
        return out

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1 and self.unet.config.time_cond_proj_dim is None                # pipe:494-497

    @property
    def clip_skip(self):
        return self._clip_skip

    @property
    def num_timesteps(self):
        return self._num_timesteps

    # ---- pipe:328-436
    def check_inputs(self, prompt, callback_steps, negative_prompt=None, prompt_embeds=None, negative_prompt_embeds=None,
                     ip_adapter_image=None, ip_adapter_image_embeds=None, blobnet_conditioning_scale=1.0, control_guidance_start=0.0,
                     control_guidance_end=1.0, callback_on_step_end_tensor_inputs=None):
        if callback_steps is not None and (not isinstance(callback_steps, int) or callback_steps <= 0):
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type {type(callback_steps)}.")
        if callback_on_step_end_tensor_inputs is not None and not all(k in self._callback_tensor_inputs
                                                                      for k in callback_on_step_end_tensor_inputs):
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but found "
                             f"{[k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to"
                             " only forward one of the two.")
        elif prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        elif prompt is not None and (not isinstance(prompt, str) and not isinstance(prompt, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt`: {negative_prompt} and `negative_prompt_embeds`:"
                             f" {negative_prompt_embeds}. Please make sure to only forward one of the two.")
        if prompt_embeds is not None and negative_prompt_embeds is not None and prompt_embeds.shape != negative_prompt_embeds.shape:
            raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                             f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds` {negative_prompt_embeds.shape}.")
        if not isinstance(blobnet_conditioning_scale, float):
            raise TypeError("For single blobnet: `blobnet_conditioning_scale` must be type `float`.")
        if not isinstance(control_guidance_start, (tuple, list)):
            control_guidance_start = [control_guidance_start]
        if not isinstance(control_guidance_end, (tuple, list)):
            control_guidance_end = [control_guidance_end]
        if len(control_guidance_start) != len(control_guidance_end):
            raise ValueError(f"`control_guidance_start` has {len(control_guidance_start)} elements, but `control_guidance_end` has "
                             f"{len(control_guidance_end)} elements. Make sure to provide the same number of elements to each list.")
        for start, end in zip(control_guidance_start, control_guidance_end):
            if start >= end:
                raise ValueError(f"control guidance start: {start} cannot be larger or equal to control guidance end: {end}.")
            if start < 0.0:
                raise ValueError(f"control guidance start: {start} can't be smaller than 0.")
            if end > 1.0:
                raise ValueError(f"control guidance end: {end} can't be larger than 1.0.")
        # pipe:422-436
        if ip_adapter_image is not None and ip_adapter_image_embeds is not None:
            raise ValueError("Provide either `ip_adapter_image` or `ip_adapter_image_embeds`. Cannot leave both `ip_adapter_image` and "
                             "`ip_adapter_image_embeds` defined.")
        if ip_adapter_image_embeds is not None:
            if not isinstance(ip_adapter_image_embeds, list):
                raise ValueError(f"`ip_adapter_image_embeds` has to be of type `list` but is {type(ip_adapter_image_embeds)}")
            elif ip_adapter_image_embeds[0].ndim not in [3, 4]:
                raise ValueError(f"`ip_adapter_image_embeds` has to be a list of 3D or 4D tensors but is {ip_adapter_image_embeds[0].ndim}D")
        if ip_adapter_image is not None and getattr(self, "image_encoder", None) is None:
            # without an image encoder (load_ip_adapter(..., image_encoder_folder=) or the `image_encoder` component) the embeddings
            # are the supported input
            raise NotImplementedError("`ip_adapter_image` needs a CLIP vision tower, which this pipeline does not have: encode the image "
                                      "yourself and pass `ip_adapter_image_embeds`")

    # ---- pipe:508-687
    def _tokenize(self, text, max_length):
        ids = self.tokenizer(text, padding="max_length", max_length=max_length, truncation=True, return_tensors="pt").input_ids
        return torch.as_tensor(ids, dtype=torch.int64)

    def encode_prompt(self, prompt, device, num_images_per_prompt, do_classifier_free_guidance, negative_prompt=None,
                      prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                      lora_scale: Optional[float] = None, clip_skip: Optional[int] = None):
        """pipe:508-687.  `lora_scale`: the scale of the text encoder's active adapters for this call (pipe:551-558); None = 1.0."""
        te_kw = {"lora_scale": 1.0 if lora_scale is None else float(lora_scale)} if hasattr(self.text_encoder, "_adapters") else {}
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        if prompt_embeds is None:
            if self.tokenizer is None or self.text_encoder is None:
                raise ValueError("this pipeline was built without tokenizer / text_encoder: pass prompt_embeds")
            ids = self._tokenize(prompt, getattr(self.tokenizer, "model_max_length", 77))
            prompt_embeds = self.text_encoder(ids.to(self.device), clip_skip=clip_skip, **te_kw)[0]
        prompt_embeds = prompt_embeds.to(self.device)
        bs_embed, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1).view(bs_embed * num_images_per_prompt, seq_len, -1)
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            if negative_prompt is None:
                uncond_tokens = [""] * batch_size
            elif prompt is not None and type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} !="
                                f" {type(prompt)}.")
            elif isinstance(negative_prompt, str):
                uncond_tokens = [negative_prompt]
            elif batch_size != len(negative_prompt):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`:"
                                 f" {prompt} has batch size {batch_size}. Please make sure that passed `negative_prompt` matches"
                                 " the batch size of `prompt`.")
            else:
                uncond_tokens = negative_prompt
            if self.tokenizer is None or self.text_encoder is None:
                raise ValueError("this pipeline was built without tokenizer / text_encoder: pass negative_prompt_embeds")
            ids = self._tokenize(uncond_tokens, prompt_embeds.shape[1])
            negative_prompt_embeds = self.text_encoder(ids.to(self.device), **te_kw)[0]
        if do_classifier_free_guidance:
            seq_len = negative_prompt_embeds.shape[1]
            negative_prompt_embeds = negative_prompt_embeds.to(self.device).repeat(1, num_images_per_prompt, 1)
            negative_prompt_embeds = negative_prompt_embeds.view(batch_size * num_images_per_prompt, seq_len, -1)
        return prompt_embeds, negative_prompt_embeds

    # ---- pipe:300-309 (the posterior sample draws from the GLOBAL generator there; `generator` makes it reproducible here)
    def encode_latents(self, image, device=None, dtype=None, prompt_embeds=None, height=512, width=512, generator=None):
        if self.vae is None:
            raise ValueError("this pipeline was built without a VAE: it cannot encode images")
        if _is_device_image(image):
            # pixels that are on the device already (blobctrl_amd.edit_inputs): the PIL branch of `preprocess`, bit for bit, at their own size
            from .edit_inputs import vae_input
            f = self.image_processor.config.vae_scale_factor
            want = tuple(v - v % f for v in (image.shape[0] if height is None else height, image.shape[1] if width is None else width))
            if tuple(image.shape[:2]) != tuple(want):
                raise ValueError(f"a uint8 device image of {tuple(image.shape[:2])} cannot be resized to {tuple(want)} on the device: hand "
                                 "the host path a PIL image (it resizes with lanczos), or build the inputs at (height, width)")
            image = vae_input(image)
        elif not torch.is_tensor(image):
            image = self.image_processor.preprocess(image, height=height, width=width)
        lat = self.engine.encode_latents(image.to(self.device, torch.float32), generator)
        return lat if prompt_embeds is None else lat.repeat(prompt_embeds.shape[0], 1, 1, 1)

    # ---- masked edits: the image and the mask of pipeline_stable_diffusion_inpaint.py (check_inputs, prepare_latents 709-712,
    # prepare_mask_latents, the mask_processor of its constructor)
    def _check_blend_inputs(self, image, mask_image, height, width):
        if (image is None) != (mask_image is None):
            raise ValueError("`image` and `mask_image` go together: the image to keep and where to keep it (white = repaint). Pass both or "
                             "neither.")
        if image is None:
            return
        if height % self.vae_scale_factor != 0 or width % self.vae_scale_factor != 0:
            raise ValueError(f"`height` and `width` have to be divisible by {self.vae_scale_factor} but are {height} and {width}.")
        if torch.is_tensor(mask_image):                            # (anything else: the mask processor's own type check)
            if mask_image.dtype != torch.uint8 or mask_image.ndim not in (2, 3) or tuple(mask_image.shape[-2:]) != (height, width):
                raise ValueError(f"a tensor `mask_image` is a uint8 device mask [H][W] or [n][H][W] of exactly (height, width) = "
                                 f"{(height, width)}, got {mask_image.dtype} {tuple(mask_image.shape)}")
        if torch.is_tensor(image) and not _is_device_image(image) and not (image.ndim == 4 and image.shape[1] == 4):
            raise ValueError(f"a tensor `image` is a uint8 device image [H][W][3] or latents [n][4][h][w], got {image.dtype} {tuple(image.shape)}")

    def prepare_blend_image_latents(self, image, height, width):
        """The latents a masked edit keeps: a tensor with 4 channels is taken as latents (inpaint:709-712), everything else is encoded."""
        if torch.is_tensor(image) and not _is_device_image(image):
            h, w = height // self.vae_scale_factor, width // self.vae_scale_factor
            if tuple(image.shape[2:]) != (h, w):
                raise ValueError(f"`image` given as latents must be [n][4][{h}][{w}] for height {height} and width {width}, got {tuple(image.shape)}")
            return image.to(self.device, torch.float32)
        return self.encode_latents(image, height=height, width=width)

    def prepare_blend_mask(self, mask_image, height, width, batch_size):
        """`mask_image` as the engine takes it: a device mask as it is ([n][H][W] uint8; bc_blend_mask reduces it), a host mask through
        the mask_processor and the nearest reduction of prepare_mask_latents -> fp32 [n][1][h][w], 1 = repaint."""
        if torch.is_tensor(mask_image):
            if mask_image.device.type != "cuda":
                raise _lib.BlobCtrlHipError("a tensor `mask_image` is reduced on the device (bc_blend_mask): there is no CPU fallback - pass a "
                                            "device tensor, a PIL image or a numpy array")
            mask = mask_image[None] if mask_image.ndim == 2 else mask_image
        else:
            from .image_processor import IPAdapterMaskProcessor         # (the settings of the reference's mask_processor)
            f = self.vae_scale_factor
            mask = IPAdapterMaskProcessor(vae_scale_factor=f).preprocess(mask_image, height=height, width=width)
            mask = mask[:, :, ::f, ::f].contiguous()                     # F.interpolate(size=(h, w)), nearest: the top-left pixel of a cell
        if mask.shape[0] not in (1, batch_size):
            raise ValueError("The passed mask and the required batch size don't match. Masks are supposed to be duplicated to"
                             f" a total batch size of {batch_size}, but {mask.shape[0]} masks were passed. Pass one mask, or one per image.")
        return mask

    # ---- pipe:690-703
    def encode_image_dinov2(self, image, device=None):
        if self.dinov2 is None:
            raise ValueError("this pipeline was built without dinov2: it cannot embed the foreground image")
        from .image_processor import Dinov2ImageProcessor
        if _is_device_image(image) and image.is_cuda and type(self.dinov2_processor) is Dinov2ImageProcessor:
            # this package's processor is Pillow's bicubic resize, a crop and a per-byte normalisation: `resample` does them where the pixels
            # are, to the same bytes, and nothing comes to the host
            from .resample import dinov2_pixel_values
            image = dinov2_pixel_values(image, self.dinov2_processor)
        elif _is_device_image(image):
            # any other processor object: the foreground canvas comes to the host (3 H W bytes) for its own preprocessing
            image = image.cpu().numpy()
        if not torch.is_tensor(image):
            image = self.dinov2_processor.preprocess(images=image, do_resize=True, return_tensors="pt", do_convert_rgb=True)["pixel_values"]
        emb = self.dinov2(pixel_values=torch.as_tensor(image).to(self.device, torch.float32)).pooler_output
        return emb.unsqueeze(1) if emb.ndim == 2 else emb

    # ---- pipe:438-453 + D/utils/torch_utils.py:38-83 (a CPU generator draws on the CPU, then the noise moves to the device)
    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        shape = (batch_size, num_channels_latents, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            if isinstance(generator, list):
                noise = torch.cat([torch.randn((1,) + shape[1:], generator=g_, device=g_.device, dtype=torch.float32).cpu()
                                   for g_ in generator], 0)
            else:
                gdev = generator.device if generator is not None else "cpu"
                noise = torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32)
        else:
            noise = latents
        noise = noise.to(self.device, torch.float32)
        return noise * self.scheduler.init_noise_sigma, noise

    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str]] = None, fg_image=None, bg_image=None, gs_score: torch.Tensor = None,
                 height: Optional[int] = 512, width: Optional[int] = 512, num_inference_steps: int = 50, timesteps: List[int] = None,
                 guidance_scale: float = 7.5, negative_prompt: Optional[Union[str, List[str]]] = None,
                 num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                 ip_adapter_image=None, ip_adapter_image_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 cross_attention_kwargs=None, blobnet_conditioning_scale: Union[float, List[float]] = 1.0,
                 blobnet_control_guidance_start: Union[float, List[float]] = 0.0,
                 blobnet_control_guidance_end: Union[float, List[float]] = 1.0, clip_skip: Optional[int] = None,
                 callback_on_step_end=None, callback_on_step_end_tensor_inputs: List[str] = ["latents"], return_sample: bool = False,
                 pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0, image=None, mask_image=None, **kwargs):
        """pipeline_blobnet.py:743-1166 with the same keyword names, defaults and error behaviour.  Returns
        StableDiffusionBlobNetPipelineOutput(images=..., nsfw_content_detected=None) or `(images, None)` for return_dict=False;
        `output_type` "pil" | "np" | "pt" | "latent".  Beyond the reference: `fg_image` / `bg_image` may be uint8 DEVICE tensors [H][W][3] of
        exactly (height, width), as `blobctrl_amd.edit_inputs` builds them; they give the latents the same pixels give as PIL images.
        `pag_scale` / `pag_adaptive_scale`: perturbed-attention guidance as in the reference's PAG pipelines, on the layers of
        `set_pag_applied_layers` (default "mid"); pag_scale = 0, the default, is the call without it.
        `image` / `mask_image` (both or neither): a masked edit as the reference stack's four-channel inpainting pipeline runs it
        (pipeline_stable_diffusion_inpaint.py:1272-1285) - where the mask is black the result keeps `image`: after every step those
        latents are `image`'s latents noised to the next timestep, and at the end `image`'s latents themselves.  `image`: PIL, numpy, a
        uint8 device tensor [H][W][3] (encoded through `encode_latents`, after fg_image and bg_image), or a tensor with 4 channels, taken
        as latents (inpaint:709-712).  `mask_image`, white = repaint: PIL or numpy through the reference's mask_processor (resized to
        (height, width), greyscale, binarised at 0.5) and prepare_mask_latents' nearest reduction; or a uint8 device tensor [H][W] or
        [n][H][W] of exactly (height, width), reduced on the device (bc_blend_mask) to the same values.  One mask or one per image."""
        callback_steps = kwargs.pop("callback_steps", None)
        if kwargs.pop("callback", None) is not None:
            raise NotImplementedError("`callback` is deprecated in the reference (pipe:868-875): use callback_on_step_end")
        if kwargs:
            raise TypeError(f"unexpected keyword arguments {sorted(kwargs)}")
        if timesteps is not None and getattr(self._scheduler, "kind", None) not in ("dpmsolver", "euler", "lcm"):
            # the reference's retrieve_timesteps (pipe:142-148) honours them only for schedulers whose set_timesteps takes them
            raise NotImplementedError("custom `timesteps` are not tabulated; pass num_inference_steps")
        # pipe:934-945, 1084: {"scale": s} scales every active adapter for this call, in the text encoder when it encodes the prompt and in
        # the UNet (BlobNet has no LoRA and never sees it).  The UNet re-packs when the scale differs from the packed one, and `engine`
        # below is re-pointed exactly as after `set_adapters`.
        # "ip_adapter_masks" (pipe:1084 -> IPAdapterAttnProcessor2_0) leaves the dict first: one tensor [1][images][H][W] per loaded adapter,
        # checked as the processor checks them once the image embeddings are known (`engine.denoise`).  Without a loaded adapter nothing
        # reads the key - in the reference it is one of `quiet_attn_parameters` - so it is dropped silently.
        cross_attention_kwargs, ip_adapter_masks = ip_masks.split_kwargs(cross_attention_kwargs)
        if not (self.unet.__dict__.get("ip_adapters") or []):
            ip_adapter_masks = None
        lora_scale = lora_scale_of(cross_attention_kwargs)
        # 0.1 align the control-guidance format (pipe:884-893)
        if not isinstance(blobnet_control_guidance_start, list) and isinstance(blobnet_control_guidance_end, list):
            blobnet_control_guidance_start = len(blobnet_control_guidance_end) * [blobnet_control_guidance_start]
        elif not isinstance(blobnet_control_guidance_end, list) and isinstance(blobnet_control_guidance_start, list):
            blobnet_control_guidance_end = len(blobnet_control_guidance_start) * [blobnet_control_guidance_end]
        elif not isinstance(blobnet_control_guidance_start, list) and not isinstance(blobnet_control_guidance_end, list):
            blobnet_control_guidance_start, blobnet_control_guidance_end = [blobnet_control_guidance_start], [blobnet_control_guidance_end]
        # 1. check inputs (pipe:897-909)
        self.check_inputs(prompt, callback_steps, negative_prompt, prompt_embeds, negative_prompt_embeds, ip_adapter_image,
                          ip_adapter_image_embeds, blobnet_conditioning_scale, blobnet_control_guidance_start,
                          blobnet_control_guidance_end, callback_on_step_end_tensor_inputs)
        if gs_score is None:
            raise ValueError("gs_score is required (pipe:974)")
        self._check_blend_inputs(image, mask_image, height, width)
        # 2. call parameters (pipe:912-922)
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        self._guidance_scale, self._clip_skip = guidance_scale, clip_skip
        if isinstance(pag_scale, (list, tuple)) or isinstance(pag_adaptive_scale, (list, tuple)):
            raise NotImplementedError("pag_scale / pag_adaptive_scale: one value per call (a PAG plan reads one pag_table, shared by the batch)")
        self._pag_scale, self._pag_adaptive_scale = pag_scale, pag_adaptive_scale
        pag_kw = {}
        if self.do_perturbed_attention_guidance:                     # (else: the call the pipeline always made)
            pag_kw = dict(pag_scale=float(pag_scale), pag_adaptive_scale=float(pag_adaptive_scale),
                          pag_applied_layers=pag_mod.resolve_layers(self.unet.trunk_config, self.pag_applied_layers))
        cfg = self.do_classifier_free_guidance
        self.unet.set_lora_scale(lora_scale)
        # 3. prompt (pipe:937-949)
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(prompt, self.device, num_images_per_prompt, cfg, negative_prompt,
                                                                   prompt_embeds=prompt_embeds,
                                                                   negative_prompt_embeds=negative_prompt_embeds, lora_scale=lora_scale,
                                                                   clip_skip=clip_skip)
        if cfg:
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds])
        # 5./6. timesteps and latents (pipe:953-968); the noise is drawn BEFORE the images are encoded, like the reference
        if timesteps is not None:                                    # retrieve_timesteps (pipe:142-151)
            self.scheduler.set_timesteps(timesteps=timesteps)
            num_inference_steps = len(self.scheduler.timesteps)
        else:
            self.scheduler.set_timesteps(num_inference_steps)
        self._num_timesteps = len(self.scheduler.timesteps)          # pipe:954 (Heun: 2 * num_inference_steps - 1)
        lat0, noise = self.prepare_latents(batch_size * num_images_per_prompt, self.unet.config.in_channels, height, width,
                                           prompt_embeds.dtype, self.device, generator, latents)
        # 7. image latents (pipe:970-971): fg first, then bg - the order in which the reference consumes the global generator
        fg_lat = self.encode_latents(fg_image, height=height, width=width)
        bg_lat = self.encode_latents(bg_image, height=height, width=width)
        # (the image a masked edit keeps is encoded last: every call without one consumes the generator as it always did)
        blend_kw = {}
        if mask_image is not None:
            blend_kw = dict(blend_image_latents=self.prepare_blend_image_latents(image, height, width),
                            blend_mask=self.prepare_blend_mask(mask_image, height, width, batch_size * num_images_per_prompt))
        # 9. DINOv2 feature of the foreground (pipe:982)
        dino = self.encode_image_dinov2(fg_image)
        # 12. loop (pipe:1025-1123) on the captured plans
        # 6.5 the guidance-scale embedding of a UNet with time_cond_proj_dim (pipe:987-993)
        timestep_cond = None
        if self.unet.config.time_cond_proj_dim is not None:
            w = torch.full((batch_size * num_images_per_prompt,), self.guidance_scale - 1, dtype=torch.float32)
            timestep_cond = get_guidance_scale_embedding(w, self.unet.config.time_cond_proj_dim)
        # 3.1 the image embeddings of the loaded IP-Adapters (pipe:923-930)
        ip_embeds = None
        if ip_adapter_image is not None or ip_adapter_image_embeds is not None:
            ip_embeds = self.prepare_ip_adapter_image_embeds(ip_adapter_image, ip_adapter_image_embeds, self.device,
                                                             batch_size * num_images_per_prompt, cfg)
            want = batch_size * num_images_per_prompt * (2 if cfg else 1)
            for e in ip_embeds:
                if e.ndim not in (3, 4) or e.shape[0] != want:           # (4D: the hidden states an IP-Adapter Plus takes)
                    raise ValueError(f"`ip_adapter_image_embeds`: after the chunk and repeat of prepare_ip_adapter_image_embeds a tensor is "
                                     f"{tuple(e.shape)}; the UNet batch of this call needs [{want}][images][embed_dim]")
        cb = None
        if callback_on_step_end is not None:
            def cb(_engine, i, t, kw):
                out = callback_on_step_end(self, i, t, {k: kw[k] for k in callback_on_step_end_tensor_inputs if k in kw})
                return out
        final = self.engine.denoise(prompt_embeds, fg_lat, bg_lat, gs_score.to(self.device), dino,
                                    num_inference_steps=num_inference_steps, guidance_scale=float(guidance_scale), latents=noise,
                                    blobnet_conditioning_scale=blobnet_conditioning_scale,
                                    blobnet_control_guidance_start=blobnet_control_guidance_start[0],
                                    blobnet_control_guidance_end=blobnet_control_guidance_end[0], output_type="latent",
                                    callback_on_step_end=cb, return_sample=return_sample, eta=eta, do_classifier_free_guidance=cfg,
                                    generator=generator, timesteps=timesteps, timestep_cond=timestep_cond,
                                    freeu=getattr(self.unet, "freeu", None), ip_adapter_image_embeds=ip_embeds,
                                    ip_adapter_masks=ip_adapter_masks, **pag_kw, **blend_kw)
        # pipe:1132-1166
        if output_type != "latent":
            if self.vae is None:
                raise ValueError("this pipeline was built without a VAE: use output_type='latent'")
            image = self.vae.decode(final / self.vae.config.scaling_factor, return_dict=False)[0]
        else:
            image = final
        image = self.image_processor.postprocess(image, output_type=output_type, do_denormalize=[True] * image.shape[0])
        if not return_dict:
            return (image, None)
        return StableDiffusionBlobNetPipelineOutput(images=image, nsfw_content_detected=None)
