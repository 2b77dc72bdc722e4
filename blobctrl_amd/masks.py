"""Connected components of binary masks on the GPU, and `segment_anything.utils.amg.remove_small_regions` on top of them
(include/blobctrl_masks.h, csrc/mask_regions.hip): what stands between a raw SAM mask and the ellipse fitted to its convex hull.  One
detached speck is a hull vertex and a pinhole changes the area, so `blob_edit` and `SamAutomaticMaskGenerator.generate` clean masks here,
on the device, before any of them crosses to the host.

Everything is integer and exact: a label is the smallest raster index y * W + x of the pixel's 8-connected component (-1 for pixels of the
other colour), and the result does not depend on how a launch splits the image.  Both colours use 8-connectivity, as
`cv2.connectedComponentsWithStats(working_mask, 8)` does in both of the package's modes.  No CPU fallback: a CPU tensor raises
`BlobCtrlHipError`.  This module raises it itself, before the library is called: the entry points take raw addresses, and a host pointer
handed to a kernel would fault on the device instead of being refused.
"""
import numpy as np
import torch

from . import _lib

MODES = {"holes": _lib.MASK_HOLES, "islands": _lib.MASK_ISLANDS}
# `clean_masks` / `remove_small_regions` need two int32 words of scratch per pixel (labels, areas).  They process the masks in groups whose
# scratch stays under this many bytes (at least one mask per group): 64 masks of 1024 x 1024 would need 512 MiB at once, and run as two
# groups of 32.
SCRATCH_BUDGET_BYTES = 256 << 20


def _device_masks(masks, what):
    """bool / uint8 device tensor [n][H][W] or [H][W] -> (uint8 view or copy [n][H][W] contiguous, whether a batch axis was added)."""
    if not torch.is_tensor(masks):
        raise TypeError(f"{what} takes a torch tensor")
    if masks.device.type != "cuda":
        raise _lib.BlobCtrlHipError(f"blobctrl_amd.masks.{what} runs on MI355X only; there is no CPU fallback")
    if masks.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{what} takes bool or uint8 masks, not {masks.dtype}")
    if masks.ndim not in (2, 3) or 0 in masks.shape:
        raise ValueError(f"{what} takes masks [n][H][W] or [H][W] with n, H, W >= 1")
    m = masks[None] if masks.ndim == 2 else masks
    m = m.contiguous()
    return (m.view(torch.uint8) if m.dtype == torch.bool else m), masks.ndim == 2


def _group(n, H, W):
    return max(1, SCRATCH_BUDGET_BYTES // (8 * H * W)) if n else 1


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


@torch.no_grad()
def label_components(masks, foreground=True):
    """bc_mask_label: int32 labels of the shape of `masks` - the smallest raster index of the pixel's 8-connected component among the set
    pixels (`foreground`) or the zero pixels (not `foreground`), -1 for the pixels of the other colour."""
    m, squeeze = _device_masks(masks, "label_components")
    n, H, W = m.shape
    lib = _lib.load()
    labels = torch.empty(n, H, W, dtype=torch.int32, device=m.device)
    with torch.cuda.device(m.device):
        _lib.check(lib.bc_mask_label(m.data_ptr(), n, H, W, 1 if foreground else 0, labels.data_ptr(), _stream(m.device)), "bc_mask_label")
    return labels[0] if squeeze else labels


def _remove_small(work, modes, area_thresh):
    """bc_mask_remove_small for each mode of `modes` in turn, in place on `work` uint8 [n][H][W] -> out int32 [len(modes)][n][6]."""
    lib = _lib.load()
    n, H, W = work.shape
    out = torch.empty(len(modes), n, 6, dtype=torch.int32, device=work.device)
    step = _group(n, H, W)
    scratch = torch.empty(2, min(step, n), H, W, dtype=torch.int32, device=work.device)
    with torch.cuda.device(work.device):
        stream = _stream(work.device)
        for lo in range(0, n, step):
            k = min(step, n - lo)
            for j, mode in enumerate(modes):
                _lib.check(lib.bc_mask_remove_small(work[lo].data_ptr(), k, H, W, int(area_thresh), mode, scratch[0].data_ptr(),
                                                    scratch[1].data_ptr(), out[j, lo].data_ptr(), stream), "bc_mask_remove_small")
    return out


@torch.no_grad()
def remove_small_regions(mask, area_thresh, mode):
    """`segment_anything.utils.amg.remove_small_regions`.  A 2-D numpy array gives (numpy bool array, bool): it is uploaded, run and
    downloaded.  A device tensor [n][H][W] (or [H][W]) gives (bool tensor of that shape, bool tensor [n] (or a 0-d one)); the input is not
    modified.  `changed` is the package's flag: a region below the threshold exists (in "islands" that includes a lone speck, which then
    stays as the largest).  `area_thresh` <= 0 changes nothing: the numpy array itself comes back, a bool tensor itself, and a uint8 tensor
    as `mask != 0` (the result is bool in every case)."""
    if mode not in MODES:
        raise ValueError(f"remove_small_regions: mode must be 'holes' or 'islands', not {mode!r}")
    if isinstance(mask, np.ndarray):
        if mask.ndim != 2:
            raise ValueError("remove_small_regions takes a 2-D numpy mask (or a device tensor [n][H][W])")
        if area_thresh <= 0:
            return mask, False
        if not torch.cuda.is_available():
            raise _lib.BlobCtrlHipError("blobctrl_amd.masks.remove_small_regions runs on MI355X only; there is no CPU fallback")
        out, changed = remove_small_regions(torch.from_numpy(np.ascontiguousarray(mask != 0)).cuda(), area_thresh, mode)
        return out.cpu().numpy(), bool(changed.item())
    m, squeeze = _device_masks(mask, "remove_small_regions")
    if area_thresh <= 0:
        return (mask if mask.dtype == torch.bool else mask != 0), torch.zeros(() if squeeze else m.shape[:1], dtype=torch.bool, device=m.device)
    work = (m != 0).view(torch.uint8)                  # a copy with bytes 0 / 1: the input stays as it is
    out = _remove_small(work, [MODES[mode]], area_thresh)[0]
    res, changed = work.view(torch.bool), out[:, 0] != 0
    return (res[0], changed[0]) if squeeze else (res, changed)


@torch.no_grad()
def clean_masks(masks, min_area):
    """What `SamAutomaticMaskGenerator.postprocess_small_regions` does to each mask: fill the holes below `min_area`, then remove the islands
    below it FROM THE HOLE-FILLED MASK (filling a hole can join two islands, so the order is part of the result).  masks: device tensor bool /
    uint8 [n][H][W] -> (bool masks [n][H][W], changed bool [n], stats int32 [n][5] = area, x0, y0, x1, y1 of the cleaned mask; the box is
    inclusive and 0 0 0 0 for an empty mask).  The input is not modified.  Scratch: see SCRATCH_BUDGET_BYTES."""
    m, squeeze = _device_masks(masks, "clean_masks")
    if squeeze:
        raise ValueError("clean_masks takes masks [n][H][W]")
    if min_area < 0:
        raise ValueError("clean_masks: min_area must be >= 0")
    work = (m != 0).view(torch.uint8)
    out = _remove_small(work, [_lib.MASK_HOLES, _lib.MASK_ISLANDS], min_area)
    return work.view(torch.bool), (out[0, :, 0] != 0) | (out[1, :, 0] != 0), out[1, :, 1:].contiguous()
