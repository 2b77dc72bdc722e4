"""The front half of an edit on the GPU (include/blobctrl_edit.h, csrc/edit_inputs.hip): from the clean device mask that `SamPredictor` and
`masks.clean_masks` leave, to the three things the pipeline takes - without the mask or the image crossing to the host.  Device tensors in,
device tensors out.

Every function here gives THE SAME BYTES as the host function of `blob_edit` / `image_processor` it stands for, and those stay what they
were: they are the checkers (tests/test_edit_inputs_gpu.py).  The ellipse predicate is `blob_edit.ellipse_mask`'s arithmetic in fp64, one
correctly rounded operation at a time on both sides; everything else is integer.  One small copy does cross: `ellipses_from_masks` fetches
the first / last set column of every mask row (n * H * 8 bytes) and fits the ellipses on the host, as `blob_edit.ellipses_from_image` does
from the same points.  The foreground canvas no longer does: the pipeline builds DINOv2's input from it on the device
(`resample.dinov2_pixel_values`, Pillow's bicubic resize bit for bit), unless it was given a processor object that is not this package's.

No CPU fallback: a CPU tensor raises `BlobCtrlHipError`.  This module raises it itself, before the library is called: the entry points take
raw addresses, and a host pointer handed to a kernel would fault on the device instead of being refused.
"""
import math

import numpy as np
import torch

from . import _lib
from .blob_edit import convex_hull, fit_ellipse
from .splat import blob_dict_from_ellipse, splat_features

EDIT_OPS = ("move", "resize", "rotate", "add", "replace")
WHITE, BLACK = (255, 255, 255), (0, 0, 0)


def _no_cpu(what):
    return _lib.BlobCtrlHipError(f"blobctrl_amd.edit_inputs.{what} runs on MI355X only; there is no CPU fallback")


def _cuda_device(device, what):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _no_cpu(what)
    return dev


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _frame(H, W, what):
    H, W = int(H), int(W)
    if not (1 <= H <= _lib.EDIT_MAX_DIM and 1 <= W <= _lib.EDIT_MAX_DIM):
        raise ValueError(f"{what}: a frame of {H} x {W} is outside 1 .. {_lib.EDIT_MAX_DIM} a side")
    return H, W


def _device_masks(masks, what):
    """bool / uint8 device tensor [n][H][W] or [H][W] -> (uint8 view or copy [n][H][W] contiguous, whether a batch axis was added)."""
    if not torch.is_tensor(masks):
        raise TypeError(f"{what} takes a torch tensor")
    if masks.device.type != "cuda":
        raise _no_cpu(what)
    if masks.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{what} takes bool or uint8 masks, not {masks.dtype}")
    if masks.ndim not in (2, 3) or 0 in masks.shape:
        raise ValueError(f"{what} takes masks [n][H][W] or [H][W] with n, H, W >= 1")
    m = masks[None] if masks.ndim == 2 else masks
    m = m.contiguous()
    return (m.view(torch.uint8) if m.dtype == torch.bool else m), masks.ndim == 2


def _device_images(images, what):
    """uint8 device tensor [n][H][W][3] or [H][W][3] -> (contiguous [n][H][W][3], whether a batch axis was added)."""
    if not torch.is_tensor(images):
        raise TypeError(f"{what} takes a torch tensor")
    if images.device.type != "cuda":
        raise _no_cpu(what)
    if images.dtype != torch.uint8 or images.ndim not in (3, 4) or images.shape[-1] != 3 or 0 in images.shape:
        raise ValueError(f"{what} takes uint8 images [n][H][W][3] or [H][W][3], not {images.dtype} {tuple(images.shape)}")
    x = images[None] if images.ndim == 3 else images
    return x.contiguous(), images.ndim == 3


def _out(out, shape, dtype, device, what):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not (torch.is_tensor(out) and out.device == device and out.dtype == dtype and tuple(out.shape) == tuple(shape) and out.is_contiguous()):
        raise ValueError(f"{what}: out must be a contiguous {dtype} tensor {tuple(shape)} on {device}")
    return out


def ellipse_params(ellipse):
    """((xc, yc), (d1, d2), angle_deg) -> [xc, yc, a, b, cos t, sin t], prepared exactly as `blob_edit.ellipse_mask` prepares them: the
    device evaluates no trigonometric function and floors no axis."""
    (xc, yc), (d1, d2), angle = ellipse
    t = math.radians(angle)
    row = [float(xc), float(yc), max(d1 / 2.0, 1e-9), max(d2 / 2.0, 1e-9), math.cos(t), math.sin(t)]
    if not all(math.isfinite(v) for v in row):
        raise ValueError(f"ellipse {ellipse!r} is not finite")
    return row


def _params(ellipses, device):
    return torch.tensor([ellipse_params(e) for e in ellipses], dtype=torch.float64).reshape(-1, 6).to(device)


@torch.no_grad()
def ellipse_masks(ellipses, H, W, device="cuda:0", out=None):
    """bc_ellipse_cover: `blob_edit.ellipse_mask(e, H, W)` for every ellipse of the list -> uint8 [n][H][W], 255 / 0."""
    dev = _cuda_device(device, "ellipse_masks")
    H, W = _frame(H, W, "ellipse_masks")
    ellipses = list(ellipses)
    if not ellipses:
        raise ValueError("ellipse_masks takes at least one ellipse")
    prm = _params(ellipses, dev)
    mask = _out(out, (len(ellipses), H, W), torch.uint8, prm.device, "ellipse_masks")
    with torch.cuda.device(prm.device):
        _lib.check(_lib.load().bc_ellipse_cover(prm.data_ptr(), len(ellipses), H, W, mask.data_ptr(), _stream(prm.device)), "bc_ellipse_cover")
    return mask


@torch.no_grad()
def edit_region_masks(ops, start_ellipses, target_ellipses, H, W, device="cuda:0"):
    """The region an edit may repaint, for `pipeline(..., mask_image=)`: per request the union of its start and its target ellipse cover
    (`ellipse_masks`) -> uint8 [n][H][W], 255 / 0.  A move changes both places; a "remove" (or a request without a target) has only its
    start."""
    ops, starts = list(ops), list(start_ellipses)
    targets = list(target_ellipses) if target_ellipses is not None else [None] * len(ops)
    if not ops or not (len(starts) == len(targets) == len(ops)):
        raise ValueError("edit_region_masks: ops, start_ellipses and target_ellipses must have one entry per request, at least one")
    for op, target in zip(ops, targets):
        if op != "remove" and op not in EDIT_OPS:
            raise ValueError(f"unknown edit operation {op!r}")
        if op != "remove" and target is None:
            raise ValueError(f"{op} needs a target ellipse")
    seconds = [s if (op == "remove" or t is None) else t for op, s, t in zip(ops, starts, targets)]
    cover = ellipse_masks(starts + seconds, H, W, device)
    return cover[: len(ops)] | cover[len(ops):]


@torch.no_grad()
def paint_ellipses(images, ellipses, colors):
    """bc_ellipse_paint, IN PLACE on `images` uint8 [n][H][W][3] (contiguous): image i takes `ellipses[i][j]` in `colors[i][j]` (r, g, b) for
    j = 0 .. k - 1 in that order - `composite_mask_and_image(ellipse_mask(e), image, color)` k times over - in one launch."""
    x, squeeze = _device_images(images, "paint_ellipses")
    if squeeze or x.data_ptr() != images.data_ptr():
        raise ValueError("paint_ellipses works in place: images must be contiguous [n][H][W][3]")
    n, H, W, _ = x.shape
    _frame(H, W, "paint_ellipses")
    k = len(ellipses[0]) if len(ellipses) else 0
    if len(ellipses) != n or len(colors) != n or k < 1 or any(len(e) != k for e in ellipses) or any(len(c) != k for c in colors):
        raise ValueError("paint_ellipses takes k >= 1 ellipses and k colours for each of the n images")
    prm = _params([e for per in ellipses for e in per], x.device)
    rgb = torch.tensor(np.asarray(colors, dtype=np.int64).reshape(n, k, 3).clip(0, 255), dtype=torch.uint8).to(x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().bc_ellipse_paint(x.data_ptr(), n, H, W, prm.data_ptr(), rgb.data_ptr(), k, _stream(x.device)), "bc_ellipse_paint")
    return images


@torch.no_grad()
def row_extents(masks, out=None):
    """bc_mask_row_extents: the first and the last set column of every row, (-1, -1) for an empty row.  masks bool / uint8 [n][H][W] or
    [H][W] (non-zero = set) -> int32 [n][H][2] or [H][2]."""
    m, squeeze = _device_masks(masks, "row_extents")
    n, H, W = m.shape
    _frame(H, W, "row_extents")
    ext = _out(out, (n, H, 2), torch.int32, m.device, "row_extents")
    with torch.cuda.device(m.device):
        _lib.check(_lib.load().bc_mask_row_extents(m.data_ptr(), n, H, W, ext.data_ptr(), _stream(m.device)), "bc_mask_row_extents")
    return ext[0] if squeeze else ext


def extent_points(ext):
    """One mask's extents [H][2] (numpy) -> (points [2 R][2] = (first, y) then (last, y) of the R non-empty rows, box (x, y, w, h) or None)."""
    ys = np.nonzero(ext[:, 0] >= 0)[0]
    if len(ys) == 0:
        return np.zeros((0, 2), dtype=np.int64), None
    first, last = ext[ys, 0].astype(np.int64), ext[ys, 1].astype(np.int64)
    x, y = int(first.min()), int(ys[0])
    return np.concatenate([np.stack([first, ys], 1), np.stack([last, ys], 1)]), (x, y, int(last.max()) - x + 1, int(ys[-1]) - y + 1)


@torch.no_grad()
def ellipses_from_masks(masks):
    """`blob_edit.ellipse_from_mask` for every mask of a device batch -> (ellipses, boxes), two lists of n.  One copy of n * H * 8 bytes comes
    to the host; per mask the ellipse is `fit_ellipse(convex_hull(...))` of the first / last set pixel of every row - every vertex of the hull
    of the set pixels is one of them, so hull and ellipse are those of the whole mask (the route of `blob_edit.ellipses_from_image`).
    ellipses[i] is None for an empty mask and for one `fit_ellipse` refuses; boxes[i] = (x, y, w, h), what `object_region_from_mask` cuts
    out, is None for an empty mask only."""
    ext = row_extents(masks)
    ext = (ext[None] if ext.ndim == 2 else ext).cpu().numpy()
    ellipses, boxes = [], []
    for e in ext:
        pts, box = extent_points(e)
        boxes.append(box)
        try:
            ellipses.append(fit_ellipse(convex_hull(pts)) if box is not None else None)
        except ValueError:
            ellipses.append(None)
    return ellipses, boxes


@torch.no_grad()
def object_regions(image, masks, boxes, out=None):
    """bc_mask_cutout: `blob_edit.object_region_from_mask(masks[i], image)` for every mask -> uint8 [n][H][W][3], the pipeline's fg images.
    image uint8 device [H][W][3]; masks bool / uint8 [n][H][W] or [H][W]; boxes: n (x, y, w, h) as `ellipses_from_masks` returns them (None,
    an empty mask, raises ValueError as the host function does)."""
    img, squeeze = _device_images(image, "object_regions")
    if not squeeze:
        raise ValueError("object_regions takes one image [H][W][3]")
    m, _ = _device_masks(masks, "object_regions")
    n, H, W = m.shape
    _frame(H, W, "object_regions")
    if m.device != img.device or tuple(img.shape[1:3]) != (H, W):
        raise ValueError(f"object_regions: image {tuple(img.shape[1:])} and masks {tuple(m.shape)} differ in size or device")
    boxes = list(boxes)
    if len(boxes) != n or any(b is None for b in boxes):
        raise ValueError("empty mask" if any(b is None for b in boxes) else f"object_regions: {len(boxes)} boxes for {n} masks")
    b = np.asarray(boxes, dtype=np.int64).reshape(n, 4)
    if ((b[:, 0] < 0) | (b[:, 1] < 0) | (b[:, 2] < 1) | (b[:, 3] < 1) | (b[:, 0] + b[:, 2] > W) | (b[:, 1] + b[:, 3] > H)).any():
        raise ValueError(f"object_regions: a box leaves the {H} x {W} frame")
    bt = torch.tensor(b, dtype=torch.int32).to(m.device)
    res = _out(out, (n, H, W, 3), torch.uint8, m.device, "object_regions")
    with torch.cuda.device(m.device):
        _lib.check(_lib.load().bc_mask_cutout(img.data_ptr(), m.data_ptr(), bt.data_ptr(), n, H, W, res.data_ptr(), _stream(m.device)),
                   "bc_mask_cutout")
    return res


@torch.no_grad()
def build_edit_inputs_batch(ops, images, start_ellipses, target_ellipses=None, strengths=None, device="cuda:0"):
    """`blob_edit.build_edit_inputs(ops[i], images[i], start_ellipses[i], target_ellipses[i], strengths[i])` for a whole request batch ->
    (bg uint8 [n][H][W][3], gs_score [n][2][H // 8][W // 8], strengths list of n).  images: uint8 device tensor [n][H][W][3], or one
    [H][W][3] every request edits; it is not modified.  One paint launch covers the batch: start ellipse white, then target ellipse black
    (a "remove" paints its start ellipse white twice, has its score overwritten to bg = 1, fg = 0 and strength 0.0).  The scores are the
    existing splat's, one call per request."""
    dev = _cuda_device(device, "build_edit_inputs_batch")
    ops = list(ops)
    n = len(ops)
    if n == 0:
        raise ValueError("build_edit_inputs_batch takes at least one request")
    targets = list(target_ellipses) if target_ellipses is not None else [None] * n
    strengths = [1.0] * n if strengths is None else list(strengths)
    starts = list(start_ellipses)
    if not (len(starts) == len(targets) == len(strengths) == n):
        raise ValueError("build_edit_inputs_batch: ops, start_ellipses, target_ellipses and strengths must have one entry per request")
    for op, target in zip(ops, targets):
        if op != "remove" and op not in EDIT_OPS:
            raise ValueError(f"unknown edit operation {op!r}")
        if op != "remove" and target is None:
            raise ValueError(f"{op} needs a target ellipse")
    x, squeeze = _device_images(images, "build_edit_inputs_batch")
    if dev.index is not None and x.device != dev:
        raise ValueError(f"build_edit_inputs_batch: images are on {x.device}, not on {dev}")
    if squeeze:
        x = x.expand(n, -1, -1, -1)
    if x.shape[0] != n:
        raise ValueError(f"build_edit_inputs_batch: {x.shape[0]} images for {n} requests")
    H, W = x.shape[1:3]
    bg = x.clone(memory_format=torch.contiguous_format)
    removes = [op == "remove" for op in ops]
    paint_ellipses(bg, [(s, s if rm else t) for s, t, rm in zip(starts, targets, removes)],
                   [(WHITE, WHITE if rm else BLACK) for rm in removes])
    scores = []
    for s, t, rm in zip(starts, targets, removes):
        e = s if rm else t
        blob = blob_dict_from_ellipse([list(e[0]), list(e[1]), e[2]], W, H)
        score = splat_features(**blob, score_size=(H // 8, W // 8), return_d_score=True, device=x.device)
        if rm:
            score[:, 0] = 1.0
            score[:, 1] = 0.0
        scores.append(score)
    return bg, torch.cat(scores, 0), [0.0 if rm else float(s) for s, rm in zip(strengths, removes)]


@torch.no_grad()
def vae_input(images_u8):
    """`VaeImageProcessor.preprocess` of the same pixels at their own size, bit for bit: uint8 device [n][H][W][3] or [H][W][3] -> fp32
    [n][3][H][W] in [-1, 1].  Plain torch: the bytes as fp32, DIVIDED by 255 (by a device tensor: dividing by a Python number multiplies by
    its rounded reciprocal on the device, which is a different fp32 for 126 of the 256 byte values), then 2 x - 1."""
    x, _ = _device_images(images_u8, "vae_input")
    x = x.permute(0, 3, 1, 2).to(torch.float32) / torch.tensor(255.0, dtype=torch.float32, device=x.device)
    return (2.0 * x - 1.0).contiguous()
