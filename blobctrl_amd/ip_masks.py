"""IP-Adapter masks (`cross_attention_kwargs={"ip_adapter_masks": ...}`): the checks of IPAdapterAttnProcessor2_0
(D/models/attention_processor.py:3776-3803), the grid of IPAdapterMaskProcessor.downsample (D/image_processor.py:969-1029) and the launch
that fills a plan's per-level mask buffers, bc_ip_mask_downsample (include/blobctrl_ip_mask.h).

A mask list holds one tensor [1][images][H][W] per loaded adapter, float or uint8, on the device or the host.  The plan never sees the
contents: it owns fp16 [images][rows] buffers per adapter and attention level, and `fill_plan_masks` refills them for every edit."""
import math
import warnings

import numpy as np
import torch

from . import _lib

KEY = "ip_adapter_masks"
ASPECT_WARNING = ("The aspect ratio of the mask does not match the aspect ratio of the output image. "
                  "Please update your masks or adjust the output size for optimal performance.")


def split_kwargs(cross_attention_kwargs):
    """`cross_attention_kwargs` -> (the same without "ip_adapter_masks" (None when nothing is left), the masks or None).  What is left
    goes to weights.lora_scale_of, which refuses every key but "scale" as before."""
    if not cross_attention_kwargs or KEY not in cross_attention_kwargs:
        return cross_attention_kwargs, None
    rest = {k: v for k, v in cross_attention_kwargs.items() if k != KEY}
    return (rest or None), cross_attention_kwargs[KEY]


def check_masks(masks, images_per_adapter):
    """The processor's checks, with its wording: a tensor [adapters][1][H][W] is the legacy form; the list has one entry per adapter; each
    is a 4D tensor with leading dimension 1 whose shape[1] is the adapter's image count.  Returns the list."""
    n = len(images_per_adapter)
    if not isinstance(masks, (list, tuple)):
        if not torch.is_tensor(masks):
            raise ValueError("Each element of the ip_adapter_masks array should be a tensor with shape [1, num_images_for_ip_adapter, height, width]."
                             " Please use `IPAdapterMaskProcessor` to preprocess your mask")
        masks = list(masks.unsqueeze(1))       # for backward compatibility: a tensor of shape [num_ip_adapter, 1, height, width]
    masks = list(masks)
    if len(masks) != n:
        raise ValueError(f"Length of ip_adapter_masks array ({len(masks)}) must match length of self.scale array ({n}) and number of "
                         f"ip_hidden_states ({n})")
    for index, (mask, images) in enumerate(zip(masks, images_per_adapter)):
        if not torch.is_tensor(mask) or mask.ndim != 4 or mask.shape[0] != 1:
            raise ValueError("Each element of the ip_adapter_masks array should be a tensor with shape [1, num_images_for_ip_adapter, height, width]."
                             " Please use `IPAdapterMaskProcessor` to preprocess your mask")
        if mask.shape[1] != images:
            raise ValueError(f"Number of masks ({mask.shape[1]}) does not match number of ip images ({images}) at index {index}")
    return masks


def canvas_masks(frame_masks):
    """Masks over the edited frame [1][images][H][W] -> masks over the canvas the UNet of this pipeline runs on, [1][images][H][2 W]: the
    canvas holds the background frame on the left and the edited frame on the right (bc_assemble_input), so the left half is zero.  A mask
    with the canvas' aspect ratio downsamples onto every attention level without padding; a frame-shaped mask handed to the call as it
    is goes through the reference's grid formula with the frame's ratio, warnings and padding included, as it does in the reference."""
    if not torch.is_tensor(frame_masks) or frame_masks.ndim != 4:
        raise ValueError("canvas_masks takes a tensor [1][images][H][W]")
    return torch.cat([torch.zeros_like(frame_masks), frame_masks], dim=-1)


def mask_grid(rows, H, W, warn=True):
    """(mask_h, mask_w) of the reference's downsample for `rows` query rows under an H x W mask: int(sqrt(rows / (W / H))), plus 1 if it
    does not divide rows; rows // mask_h.  mask_w = rows // mask_h, so the grid never exceeds rows (the reference's truncation branch cannot
    be reached); a smaller grid is padded with zeros and warned about in the reference's words.  Where the reference divides by zero - the
    square root truncates to 0, one query row under a wide mask for example - this raises a ValueError."""
    ratio = W / H
    mask_h = int(math.sqrt(rows / ratio))
    if mask_h == 0:
        raise ValueError(f"ip_adapter_masks: {rows} query rows under a {H} x {W} mask give a mask height of 0 rows (int(sqrt(rows / (W / H)))); "
                         "the reference divides by zero here.  Use a mask with the aspect ratio of the output image")
    mask_h = mask_h + int(rows % mask_h != 0)
    mask_w = rows // mask_h
    if mask_w == 0:
        raise ValueError(f"ip_adapter_masks: {rows} query rows under a {H} x {W} mask give a mask width of 0 columns")
    if warn and mask_h * mask_w < rows:
        warnings.warn(ASPECT_WARNING, UserWarning)
    return mask_h, mask_w


def cubic_weights(t):
    """The four weights of the cubic convolution with A = -0.75 at fraction t (float64; taps floor - 1 .. floor + 2)."""
    A = -0.75
    c1 = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    c2 = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return np.stack([c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)], -1)


def downsample_reference(mask, rows, warn=False):
    """Float64 restatement of the launch, on the host: mask [images][H][W] (any real dtype) -> float64 [images][rows].  The tests'
    yardstick, no route of the product."""
    m = np.asarray(mask, dtype=np.float64)
    n, H, W = m.shape
    mh, mw = mask_grid(rows, H, W, warn=warn)

    def axis(size, out):
        src = size / out * (np.arange(out) + 0.5) - 0.5
        f = np.floor(src)
        idx = np.clip(f[:, None].astype(np.int64) + np.arange(-1, 3)[None], 0, size - 1)
        return idx, cubic_weights(src - f)
    iy, wy = axis(H, mh)
    ix, wx = axis(W, mw)
    rowsum = (m[:, :, ix] * wx[None, None]).sum(-1)                    # [n][H][mw]
    out = (rowsum[:, iy, :] * wy[None, :, :, None]).sum(2)             # [n][mh][mw]
    full = np.zeros((n, rows))
    full[:, : mh * mw] = out.reshape(n, -1)
    return full


def _device_mask(mask, device):
    """A mask [1][images][H][W] -> contiguous device tensor [images][H][W], uint8 as it is, everything else as fp32."""
    m = mask[0].to(device)
    m = m if m.dtype == torch.uint8 else m.to(torch.float32)
    return m.contiguous()


@torch.no_grad()
def downsample(mask, rows, out=None):
    """bc_ip_mask_downsample on the current stream: device mask [images][H][W], fp32 or uint8 -> fp16 [images][rows] (`out`, or a new
    tensor), the grid by `mask_grid`."""
    if not torch.is_tensor(mask) or mask.device.type != "cuda":
        raise _lib.BlobCtrlHipError("blobctrl_amd.ip_masks.downsample runs on MI355X only; there is no CPU fallback")
    if mask.ndim != 3 or mask.dtype not in (torch.uint8, torch.float32) or not mask.is_contiguous():
        raise ValueError(f"downsample takes a contiguous fp32 or uint8 mask [images][H][W], not {mask.dtype} {tuple(mask.shape)}")
    n, H, W = mask.shape
    mh, mw = mask_grid(rows, H, W)
    if out is None:
        out = torch.empty(n, rows, dtype=torch.float16, device=mask.device)
    elif not (out.dtype == torch.float16 and out.device == mask.device and out.ndim == 2 and out.shape[0] == n and out.shape[1] >= rows and
              out.stride(1) == 1):
        raise ValueError(f"downsample: out must be fp16 [{n}][>= {rows}] on {mask.device}")
    with torch.cuda.device(mask.device):
        _lib.check(_lib.load().bc_ip_mask_downsample(mask.data_ptr(), int(mask.dtype == torch.uint8), n, H, W, mh, mw, rows, out.data_ptr(),
                                                     out.stride(0), torch.cuda.current_stream(mask.device).cuda_stream),
                   "bc_ip_mask_downsample")
    return out


def fill_plan_masks(adapters, masks, device):
    """Refill the mask buffers of a plan made for masks: `adapters` = its engine.IpAdapter objects (mask_bufs: rows -> fp16 [images][rows]),
    `masks` = the checked list of the call.  One launch per adapter and level, on the current stream."""
    for ad, mask in zip(adapters, masks):
        m = _device_mask(mask, device)
        for rows, buf in ad.mask_bufs.items():
            downsample(m, rows, out=buf)
