"""PyTorch custom-op registrations of the hot path (`torch.ops.blobctrl.*`, `torch.library.custom_op`).

BASELINE.json's north star words the boundary as "driven from Python through PyTorch-ROCm custom ops that keep the
StableDiffusionBlobCtrlPipeline.__call__ / BlobNet / UNet-LoRA API surface".  The compute entry points of this package are the C ABI
of libblobctrl_hip.so (include/blobctrl_hip.h) reached through ctypes; this module registers the four calls the reference makes into
its hot path, FreeU, and the five steps of its blob visualisation / feature grid, as dispatcher-visible ops OVER that same C ABI, so that
`torch.profiler`, dispatch modes and fake-tensor tracing see them:

    blobctrl::splat_scores     blobctrl/utils/utils.py:145-194             (splat_features, tuple score_size branch)
    blobctrl::blobnet_forward  blobctrl/models/blobnet.py:720-945          (BlobNetModel.forward -> down / mid / up residuals)
    blobctrl::unet_forward     D/models/unets/unet_2d_condition.py:1039-1353 (patched forward with the three residual lists)
    blobctrl::denoise          blobctrl/pipelines/pipeline_blobnet.py:1025-1123 (the whole loop: one hipGraph launch per edit)
    blobctrl::denoise_requests the same loop for a request batch with per-request step counts, guidance scales and control windows
    blobctrl::freeu            D/utils/torch_utils.py:93-148                (apply_freeu on (hidden, skip) in front of an up-block concat)
    blobctrl::splat_maps       blobctrl/utils/utils.py:120-135, 145-181    (raw and composed scores, channels-last)
    blobctrl::alpha_composite  blobctrl/utils/utils.py:179-181, 205-209    (compositing of raw scores a viz_score_fn changed)
    blobctrl::splat_from_scores blobctrl/utils/utils.py:57-77, pipeline_blobnet.py:706-721 (scores x features, resize folded in)
    blobctrl::resize_bilinear  blobctrl/utils/utils.py:280-294             (one level of pyramid_resize)
    blobctrl::pack_rgb8        scripts/blobctrl_app.py:647-648             (fp64 [1][3][H][W] -> uint8 [H][W][3])

The nn.Module shells (modules.py), `splat.splat_features` and `BlobCtrlEngine.__call__` call THROUGH these ops.  A module / engine is
passed as an integer handle (ops take tensors and scalars, not Python objects): `register(obj)` keeps a weak reference.  Every op has
a fake (meta) kernel that states its output shapes, dtypes and devices without touching the GPU; the real kernels raise
BlobCtrlHipError when the HIP library is missing - there is no CPU fallback.  No autograd: the path is inference only.
"""
import weakref
from typing import List, Optional

import torch

_objects = weakref.WeakValueDictionary()
_next_handle = [1]


def register(obj) -> int:
    """Handle of a module / engine for the ops below (kept weakly: the handle dies with the object)."""
    h = getattr(obj, "_bc_handle", None)
    if h is None or _objects.get(h) is not obj:
        h = _next_handle[0]
        _next_handle[0] += 1
        _objects[h] = obj
        try:
            object.__setattr__(obj, "_bc_handle", h)
        except Exception:          # noqa: BLE001  (objects without a __dict__)
            pass
    return h


def _get(handle: int):
    obj = _objects.get(int(handle))
    if obj is None:
        raise RuntimeError(f"blobctrl op: handle {handle} does not name a live module / engine (ops.register)")
    return obj


def _dev(index: int) -> torch.device:
    return torch.device("cuda", index)


# ------------------------------------------------------------------------------------------------------------------ splat_scores
@torch.library.custom_op("blobctrl::splat_scores", mutates_args=())
def splat_scores(params: torch.Tensor, h: int, w: int, device_index: int) -> torch.Tensor:
    """params [n][8] float64 on the host (xs, ys, cov00, cov01, cov10, cov11, size, unused) -> scores [n][2][h][w] float64 on the GPU."""
    from . import splat
    return splat._splat_scores_impl(params, h, w, _dev(device_index))


@splat_scores.register_fake
def _(params, h, w, device_index):
    return torch.empty((params.shape[0], 2, h, w), dtype=torch.float64, device=_dev(device_index))


# ------------------------------------------------------------------------------------------------------------------ blob visualisation
@torch.library.custom_op("blobctrl::splat_maps", mutates_args=())
def splat_maps(params: torch.Tensor, h: int, w: int, device_index: int) -> List[torch.Tensor]:
    """params as for splat_scores -> [raw, composed], each [n][h][w][2] float64 on the GPU: raw = (1, s), composed = ((1 - s), s)."""
    from . import splat
    return splat._splat_maps_impl(params, h, w, _dev(device_index))


@splat_maps.register_fake
def _(params, h, w, device_index):
    return [torch.empty((params.shape[0], h, w, 2), dtype=torch.float64, device=_dev(device_index)) for _ in range(2)]


@torch.library.custom_op("blobctrl::alpha_composite", mutates_args=())
def alpha_composite(raw: torch.Tensor) -> torch.Tensor:
    """raw [..., K] float64 on the GPU -> composed scores of the same shape: d_i = s_i * prod_{j>i}(1 - s_j), d_{K-1} = s_{K-1}."""
    from . import splat
    return splat._alpha_composite_impl(raw)


@alpha_composite.register_fake
def _(raw):
    return torch.empty(tuple(raw.shape), dtype=raw.dtype, device=raw.device)


@torch.library.custom_op("blobctrl::splat_from_scores", mutates_args=())
def splat_from_scores(scores: torch.Tensor, features: torch.Tensor, out_h: int, out_w: int, channels_last: bool) -> torch.Tensor:
    """scores [N][H][W][M] (channels_last) or [N][M][H][W], any strides, x features [N][M][C] -> [N][C][out_h][out_w] in the scores' dtype
    (float64 / float32); a grid other than H x W is sampled bilinearly (align_corners=False) inside the read."""
    from . import splat
    return splat._splat_from_scores_impl(scores, features, out_h, out_w, channels_last)


@splat_from_scores.register_fake
def _(scores, features, out_h, out_w, channels_last):
    return torch.empty((scores.shape[0], features.shape[2], out_h, out_w), dtype=scores.dtype, device=scores.device)


@torch.library.custom_op("blobctrl::resize_bilinear", mutates_args=())
def resize_bilinear(img: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """img [N][K][H][W] float64 / float32 on the GPU -> [N][K][out_h][out_w], F.interpolate(mode="bilinear", align_corners=False)."""
    from . import splat
    return splat._resize_bilinear_impl(img, out_h, out_w)


@resize_bilinear.register_fake
def _(img, out_h, out_w):
    return torch.empty((img.shape[0], img.shape[1], out_h, out_w), dtype=img.dtype, device=img.device)


@torch.library.custom_op("blobctrl::pack_rgb8", mutates_args=())
def pack_rgb8(img: torch.Tensor) -> torch.Tensor:
    """img [1][3][H][W] float64 in [0, 1] on the GPU -> [H][W][3] uint8 = truncation of img * 255."""
    from . import splat
    return splat._pack_rgb8_impl(img)


@pack_rgb8.register_fake
def _(img):
    return torch.empty((img.shape[2], img.shape[3], 3), dtype=torch.uint8, device=img.device)


# ------------------------------------------------------------------------------------------------------------------ blobnet_forward
def blobnet_output_shapes(cfg, B: int, H: int, W: int):
    """(channels, h, w) of BlobNet's 12 down + 1 mid + 12 up residuals on an H x W canvas (bn:860-864, 881, 921-924)."""
    boc = cfg.block_out_channels
    nb = len(boc)
    down, sizes = [(boc[0], H, W)], []
    h, w = H, W
    for i in range(nb):
        sizes.append((h, w))
        down += [(boc[i], h, w)] * cfg.layers_per_block
        if i < nb - 1:
            h, w = (h + 1) // 2, (w + 1) // 2
            down.append((boc[i], h, w))
    mid = (boc[-1], h, w)
    rev = list(reversed(boc))
    up = []
    for i in range(nb):
        hh, ww = sizes[nb - 1 - i]
        up += [(rev[i], hh, ww)] * (cfg.layers_per_block + 1)
        if i < nb - 1:
            up.append((rev[i],) + sizes[nb - 2 - i])
    return down, mid, up


@torch.library.custom_op("blobctrl::blobnet_forward", mutates_args=())
def blobnet_forward(sample: torch.Tensor, timestep: float, conditioning_scale: float, handle: int) -> List[torch.Tensor]:
    """BlobNetModel.forward: the down residuals, the mid residual, the up residuals, in that order (NCHW, sample's dtype)."""
    down, mid, up = _get(handle)._forward_impl(sample, timestep, conditioning_scale)
    return list(down) + [mid] + list(up)


@blobnet_forward.register_fake
def _(sample, timestep, conditioning_scale, handle):
    m = _get(handle)
    B, _, H, W = sample.shape
    down, mid, up = blobnet_output_shapes(m.trunk_config, B, H, W)
    dt = sample.dtype if sample.dtype in (torch.float16, torch.float32) else torch.float32
    return [torch.empty((B,) + s, dtype=dt, device=m.device) for s in down + [mid] + up]


# ------------------------------------------------------------------------------------------------------------------ unet_forward
@torch.library.custom_op("blobctrl::unet_forward", mutates_args=())
def unet_forward(sample: torch.Tensor, timestep: float, encoder_hidden_states: torch.Tensor, down_add: List[torch.Tensor],
                 mid_add: Optional[torch.Tensor], up_add: List[torch.Tensor], handle: int,
                 timestep_cond: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The patched UNet2DConditionModel.forward; empty lists / None = no BlobNet residuals.  Returns eps [B][4][H][W] fp32.
    `timestep_cond` [B][time_cond_proj_dim] (a UNet with time_embedding.cond_proj): the guidance-scale embedding."""
    with_res = mid_add is not None
    extra = {} if timestep_cond is None else dict(timestep_cond=timestep_cond)
    return _get(handle)._forward_impl(sample, timestep, encoder_hidden_states, list(down_add) if with_res else None, mid_add,
                                      list(up_add) if with_res else None, **extra)


@unet_forward.register_fake
def _(sample, timestep, encoder_hidden_states, down_add, mid_add, up_add, handle, timestep_cond=None):
    m = _get(handle)
    B, _, H, W = sample.shape
    return torch.empty((B, m.trunk_config.out_channels, H, W), dtype=torch.float32, device=m.device)


# ------------------------------------------------------------------------------------------------------------------ denoise
@torch.library.custom_op("blobctrl::denoise", mutates_args=())
def denoise(prompt_embeds: torch.Tensor, fg_image_latents: torch.Tensor, bg_image_latents: torch.Tensor, gs_score: torch.Tensor,
            dino_feats: torch.Tensor, latents: torch.Tensor, num_inference_steps: int, guidance_scale: float,
            conditioning_scales: List[float], guidance_start: float, guidance_end: float, handle: int,
            scales_are_per_request: bool = False, eta: float = 0.0, variance_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The denoise loop of one edit (or one request batch) at tensor level: final latents [B][4][h][w] fp32 on the engine's device.
    `scales_are_per_request`: the caller passed a LIST of conditioning scales (one per request; `denoise` validates its length exactly
    as for a direct call) rather than one float (a one-element list used to be collapsed to a scalar and broadcast).
    `eta` > 0: stochastic DDIM, with `variance_noise` [num_inference_steps][B][4][h][w] or, when None, noise from the global RNG of the
    engine's device (a torch.Generator cannot cross the dispatcher: call the engine's `denoise(..., generator=)` for seeded noise)."""
    eng = _get(handle)
    sc = list(conditioning_scales) if scales_are_per_request else conditioning_scales[0]
    return eng.denoise(prompt_embeds, fg_image_latents, bg_image_latents, gs_score, dino_feats, num_inference_steps=num_inference_steps,
                       guidance_scale=guidance_scale, latents=latents, blobnet_conditioning_scale=sc,
                       blobnet_control_guidance_start=guidance_start, blobnet_control_guidance_end=guidance_end, eta=eta,
                       variance_noise=variance_noise)


@denoise.register_fake
def _(prompt_embeds, fg_image_latents, bg_image_latents, gs_score, dino_feats, latents, num_inference_steps, guidance_scale,
      conditioning_scales, guidance_start, guidance_end, handle, scales_are_per_request=False, eta=0.0, variance_noise=None):
    eng = _get(handle)
    return torch.empty(tuple(latents.shape), dtype=torch.float32, device=eng.device)


@torch.library.custom_op("blobctrl::denoise_requests", mutates_args=())
def denoise_requests(prompt_embeds: torch.Tensor, fg_image_latents: torch.Tensor, bg_image_latents: torch.Tensor, gs_score: torch.Tensor,
                     dino_feats: torch.Tensor, latents: torch.Tensor, num_inference_steps: List[int], guidance_scale: List[float],
                     conditioning_scales: List[float], guidance_start: List[float], guidance_end: List[float], handle: int) -> torch.Tensor:
    """The denoise loop of a request batch whose requests run their own schedules: one entry per request in every list (step count,
    guidance scale, conditioning scale, control window).  Final latents [B][4][h][w] fp32 on the engine's device; a request that ends
    before the longest one keeps the latents of its own last step."""
    eng = _get(handle)
    return eng.denoise(prompt_embeds, fg_image_latents, bg_image_latents, gs_score, dino_feats,
                       num_inference_steps=[int(v) for v in num_inference_steps], guidance_scale=[float(v) for v in guidance_scale],
                       latents=latents, blobnet_conditioning_scale=[float(v) for v in conditioning_scales],
                       blobnet_control_guidance_start=[float(v) for v in guidance_start],
                       blobnet_control_guidance_end=[float(v) for v in guidance_end])


@denoise_requests.register_fake
def _(prompt_embeds, fg_image_latents, bg_image_latents, gs_score, dino_feats, latents, num_inference_steps, guidance_scale,
      conditioning_scales, guidance_start, guidance_end, handle):
    eng = _get(handle)
    return torch.empty(tuple(latents.shape), dtype=torch.float32, device=eng.device)


# ------------------------------------------------------------------------------------------------------------------ freeu
def freeu_launch(hidden: torch.Tensor, skip: torch.Tensor, params: torch.Tensor, stage: int):
    """One bc_freeu launch on the current stream: (hidden_out, skip_out, tot_h, tot_s) - the two outputs and their GroupNorm statistics
    totals [B][C][GN_TOT_WORDS] (int64, per channel).  hidden [B][H][W][C_h], skip [B][H][W][C_s] fp16 channels-last on the GPU, params
    fp32 (s1, s2, b1, b2) on the GPU."""
    from . import _lib
    from .engine import freeu_basis
    lib = _lib.load()
    if hidden.dim() != 4 or skip.dim() != 4 or hidden.shape[:3] != skip.shape[:3]:
        raise ValueError("freeu: hidden [B][H][W][C_h] and skip [B][H][W][C_s] must share batch, height and width")
    if hidden.dtype != torch.float16 or skip.dtype != torch.float16 or params.dtype != torch.float32 or params.numel() != 4:
        raise ValueError("freeu: hidden and skip are fp16, params is fp32 (s1, s2, b1, b2)")
    if hidden.device.type != "cuda" or skip.device != hidden.device or params.device != hidden.device:
        raise _lib.BlobCtrlHipError("freeu runs on MI355X only (all tensors on one cuda device); there is no CPU fallback")
    B, H, W, C_h = hidden.shape
    C_s = skip.shape[3]
    hidden, skip, params = hidden.contiguous(), skip.contiguous(), params.contiguous()
    basis = freeu_basis(H, W).to(torch.float32).to(hidden.device)
    h_out, s_out = torch.empty_like(hidden), torch.empty_like(skip)
    tot_h = torch.zeros(B, C_h, _lib.GN_TOT_WORDS, dtype=torch.int64, device=hidden.device)
    tot_s = torch.zeros(B, C_s, _lib.GN_TOT_WORDS, dtype=torch.int64, device=hidden.device)
    _lib.check(lib.bc_freeu(hidden.data_ptr(), C_h, skip.data_ptr(), C_s, B, H * W, params.data_ptr(), int(stage), basis.data_ptr(),
                            h_out.data_ptr(), s_out.data_ptr(), tot_h.data_ptr(), tot_s.data_ptr(),
                            torch.cuda.current_stream(hidden.device).cuda_stream), "bc_freeu")
    return h_out, s_out, tot_h, tot_s


@torch.library.custom_op("blobctrl::freeu", mutates_args=())
def freeu(hidden: torch.Tensor, skip: torch.Tensor, params: torch.Tensor, stage: int) -> tuple[torch.Tensor, torch.Tensor]:
    """apply_freeu(stage, hidden, skip, s1=, s2=, b1=, b2=) on channels-last fp16 tensors [B][H][W][C]; `params` = fp32 (s1, s2, b1, b2)
    on the GPU, `stage` 0 | 1 = the up block's resolution_idx.  Returns new (hidden, skip); the inputs are not modified."""
    return freeu_launch(hidden, skip, params, stage)[:2]


@freeu.register_fake
def _(hidden, skip, params, stage):
    return (torch.empty(tuple(hidden.shape), dtype=hidden.dtype, device=hidden.device),
            torch.empty(tuple(skip.shape), dtype=skip.dtype, device=skip.device))
