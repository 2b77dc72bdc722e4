"""Zoomed ("only masked") edits on the GPU (include/blobctrl_overlay.h, csrc/overlay.hip): the box around the edited region, that box blown
up to the model's resolution, and the result pasted back through a blurred mask - `VaeImageProcessor.get_crop_region`, `blur`,
`resize(..., "fill" | "crop")` and `apply_overlay` of D/image_processor.py, without the pixels crossing to the host.

The yardstick is Pillow, and every one of those is an integer algorithm there.  The host half of this module restates them in numpy and
runs without a GPU; tests/test_overlay_cpu.py holds it to Pillow byte for byte:

  * `crop_region_reference`     get_crop_region line by line, truncations and the order of its corrections included
  * `gaussian_blur_reference`   `ImageFilter.GaussianBlur` on an "L" image: three box blurs along the rows, then three along the columns
                                (BoxBlur.c), a uint8 image between passes.  The box radius and the two weights are computed in FLOAT32, as C
                                does: `ww = (UINT32)((float)(1 << 24) / (rf * 2 + 1))` is a float32 quotient (rounded to nearest, which for
                                a radius below 0.5 is a whole number above 2^23) truncated to an integer - not a double quotient truncated
  * `apply_overlay_reference`   the RGBa paste, the un-premultiply and `alpha_composite` of apply_overlay
  * `resize_and_fill_reference`, `resize_and_crop_reference`    on top of `resample.resize_reference`

The device half runs the same integer arithmetic, so its bytes are Pillow's, with no tolerance.  No CPU fallback: a CPU tensor raises
`BlobCtrlHipError`, here, before the library is called (the entry points take raw addresses).
"""
import functools
import math

import numpy as np
import torch

from . import _lib, resample

BLUR_PASSES = 3
MAX_BLUR_RADIUS = _lib.BLUR_MAX_R     # largest integer box radius the kernels take (BC_BLUR_MAX_R): 63, that of blur_factor 64


# ---- get_crop_region ------------------------------------------------------------------------------------------------------------------

def bounds_reference(mask_u8):
    """(first column, last column, first row, last row) with a non-zero pixel, four -1 for an empty mask: what bc_mask_bounds writes."""
    m = np.asarray(mask_u8) != 0
    if m.ndim != 2 or 0 in m.shape:
        raise ValueError("a mask is [H][W] with H, W >= 1")
    cols, rows = np.nonzero(m.any(0))[0], np.nonzero(m.any(1))[0]
    if len(cols) == 0:
        return (-1, -1, -1, -1)
    return (int(cols[0]), int(cols[-1]), int(rows[0]), int(rows[-1]))


def crop_region_from_bounds(bounds, w, h, width, height, pad=0):
    """Steps 2 and 3 of D/image_processor.py:get_crop_region from the mask's bounds (step 1) and its frame (w, h)."""
    xf, xl, yf, yl = (int(v) for v in bounds)
    if xf < 0:
        raise ValueError("get_crop_region: the mask is empty (the reference divides by zero)")
    crop_left, crop_right, crop_top, crop_bottom = xf, w - 1 - xl, yf, h - 1 - yl
    x1, y1, x2, y2 = (int(max(crop_left - pad, 0)), int(max(crop_top - pad, 0)), int(min(w - crop_right + pad, w)),
                      int(min(h - crop_bottom + pad, h)))
    ratio_crop_region = (x2 - x1) / (y2 - y1)
    ratio_processing = width / height
    if ratio_crop_region > ratio_processing:
        desired_height = (x2 - x1) / ratio_processing
        desired_height_diff = int(desired_height - (y2 - y1))
        y1 -= desired_height_diff // 2
        y2 += desired_height_diff - desired_height_diff // 2
        if y2 >= h:
            diff = y2 - h
            y2 -= diff
            y1 -= diff
        if y1 < 0:
            y2 -= y1
            y1 -= y1
        if y2 >= h:
            y2 = h
    else:
        desired_width = (y2 - y1) * ratio_processing
        desired_width_diff = int(desired_width - (x2 - x1))
        x1 -= desired_width_diff // 2
        x2 += desired_width_diff - desired_width_diff // 2
        if x2 >= w:
            diff = x2 - w
            x2 -= diff
            x1 -= diff
        if x1 < 0:
            x2 -= x1
            x1 -= x1
        if x2 >= w:
            x2 = w
    return x1, y1, x2, y2


def crop_region_reference(mask_u8, width, height, pad=0):
    """`VaeImageProcessor.get_crop_region(Image.fromarray(mask_u8), width, height, pad)` -> (x1, y1, x2, y2).  An all-zero mask is a
    ValueError (the reference divides by zero)."""
    m = np.asarray(mask_u8)
    return crop_region_from_bounds(bounds_reference(m), m.shape[1], m.shape[0], width, height, pad)


# ---- ImageFilter.GaussianBlur ---------------------------------------------------------------------------------------------------------

def box_radius(blur_factor, passes=BLUR_PASSES):
    """BoxBlur.c:_gaussian_blur_radius: the fractional box radius whose `passes` box blurs have the Gaussian's variance.  C floats where C
    has floats, doubles where its literals make the expression double."""
    f = np.float32
    radius = f(blur_factor)
    sigma2 = f(f(radius * radius) / f(passes))
    L = f(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f(math.floor((float(L) - 1.0) / 2.0))
    a = f(f(f(2) * l + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * sigma2)))
    a = f(a / f(f(6) * f(sigma2 - f(f(l + f(1)) * f(l + f(1))))))
    return f(l + a)


def box_weights(rf):
    """BoxBlur.c:ImagingHorizontalBoxBlur's constants for the float32 radius rf -> (R, ww, fw): the integer radius, the weight of the 2 R + 1
    inner pixels and that of the two far pixels, in units of 2^-24.  The quotient is a float32 one, truncated."""
    rf = np.float32(rf)
    R = int(rf)
    ww = int(np.float32(1 << 24) / np.float32(rf * np.float32(2) + np.float32(1)))
    fw = ((1 << 24) - (R * 2 + 1) * ww) // 2
    return R, ww, fw


def blur_params(blur_factor):
    """(R, ww, fw) of `ImageFilter.GaussianBlur(blur_factor)`, None for a blur factor of 0 (Pillow returns a copy).  Refuses, by name, what
    the kernels do not take: a negative or non-finite factor, and an integer radius above MAX_BLUR_RADIUS."""
    bf = float(blur_factor)
    if not (math.isfinite(bf) and bf >= 0.0):
        raise ValueError(f"blur_factor {blur_factor!r} is not supported (it must be finite and >= 0)")
    if bf == 0.0:
        return None
    R, ww, fw = box_weights(box_radius(bf))
    if R > MAX_BLUR_RADIUS:
        raise ValueError(f"blur_factor {blur_factor!r} is not supported: its box radius {R} exceeds {MAX_BLUR_RADIUS} (blur_factor 64)")
    assert 0 <= fw and (2 * R + 1) * ww + 2 * fw <= 1 << 24
    return R, ww, fw


def box_blur_lines(a, R, ww, fw):
    """One BoxBlur.c line pass along the LAST axis of `a` uint8 [...][n], edge pixels repeated:
    out[x] = (sum(a[x - R .. x + R]) * ww + (a[x - R - 1] + a[x + R + 1]) * fw + 2^23) >> 24."""
    n = a.shape[-1]
    idx = np.clip(np.arange(-R - 1, n + R + 1), 0, n - 1)
    e = a[..., idx].astype(np.int64)                                      # e[j] = a[clamp(j - R - 1)]
    c = np.concatenate([np.zeros(e.shape[:-1] + (1,), np.int64), np.cumsum(e, -1)], -1)
    inner = c[..., 2 * R + 2:2 * R + 2 + n] - c[..., 1:1 + n]             # sum of e[x + 1 .. x + 2 R + 1] = a[x - R .. x + R]
    far = e[..., 0:n] + e[..., 2 * R + 2:2 * R + 2 + n]
    return ((inner * ww + far * fw + (1 << 23)) >> 24).astype(np.uint8)


def gaussian_blur_reference(mask_u8, blur_factor):
    """`np.array(Image.fromarray(mask_u8).filter(ImageFilter.GaussianBlur(blur_factor)))` for mask_u8 uint8 [H][W] (or a batch [n][H][W])."""
    a = np.asarray(mask_u8)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or 0 in a.shape:
        raise ValueError("gaussian_blur_reference takes a uint8 array [H][W] or [n][H][W]")
    prm = blur_params(blur_factor)
    if prm is None:
        return a.copy()
    for _ in range(BLUR_PASSES):
        a = box_blur_lines(a, *prm)
    a = np.swapaxes(a, -1, -2)
    for _ in range(BLUR_PASSES):
        a = box_blur_lines(a, *prm)
    return np.ascontiguousarray(np.swapaxes(a, -1, -2))


# ---- apply_overlay --------------------------------------------------------------------------------------------------------------------

def _div255(v):
    return (((v + 128) >> 8) + v + 128) >> 8


def overlay_pixels(c, m, d):
    """The pixel arithmetic of apply_overlay for int arrays of init bytes c, mask bytes m and destination bytes d (broadcast together):
    init pasted through the inverted mask onto a transparent RGBa image, back to RGBA, then `alpha_composite` onto the opaque d."""
    c, m, d = (np.asarray(v).astype(np.int64) for v in (c, m, d))
    mi = 255 - m
    p, a = _div255(mi * c), _div255(mi * 255)
    u = np.where(a > 0, np.minimum(255, 255 * p // np.maximum(a, 1)), 0)
    outa255 = a * 255 + 255 * (255 - a)
    coef1 = a * 255 * 255 * 128 // outa255
    coef2 = 255 * 128 - coef1
    t = u * coef1 + d * coef2 + (0x80 << 7)
    out = (((t >> 8) + t) >> 8) >> 7
    return np.where(a == 0, d, out).astype(np.uint8)


def _fit_sizes(iw, ih, width, height, crop):
    """(src_w, src_h) of `_resize_and_crop` (crop) / `_resize_and_fill` for an iw x ih image in a width x height frame."""
    ratio, src_ratio = width / height, iw / ih
    if crop:
        return (width if ratio > src_ratio else iw * height // ih), (height if ratio <= src_ratio else ih * width // iw)
    return (width if ratio < src_ratio else iw * height // ih), (height if ratio >= src_ratio else ih * width // iw)


def _paste_geometry(src_w, src_h, width, height):
    """`res.paste(resized, box=(width // 2 - src_w // 2, height // 2 - src_h // 2))` into a width x height frame -> (x0, y0 in the frame,
    sx, sy in resized, w, h): Pillow clips a paste that leaves the frame."""
    px, py = width // 2 - src_w // 2, height // 2 - src_h // 2
    x0, y0 = max(px, 0), max(py, 0)
    x1, y1 = min(px + src_w, width), min(py + src_h, height)
    return x0, y0, x0 - px, y0 - py, x1 - x0, y1 - y0


def resize_and_crop_reference(image_u8, width, height):
    """`np.array(VaeImageProcessor()._resize_and_crop(Image.fromarray(image_u8), width, height))` for uint8 [H][W][3]."""
    a = np.asarray(image_u8)
    src_w, src_h = _fit_sizes(a.shape[1], a.shape[0], width, height, True)
    resized = resample.resize_reference(a, (src_h, src_w), "lanczos")
    res = np.zeros((height, width, 3), np.uint8)
    x0, y0, sx, sy, w, h = _paste_geometry(src_w, src_h, width, height)
    res[y0:y0 + h, x0:x0 + w] = resized[sy:sy + h, sx:sx + w]
    return res


def band_tables(in_size, at_end, out_size):
    """The tables of `Image.resize` (its default filter, bicubic) with a box of zero extent at the start (at_end False) or the end of an
    axis of in_size pixels, `_resize_and_fill`'s bands: the scale is 0, so every output index has the same centre - the box's edge - and
    the same taps, Pillow's `precompute_coeffs` with in0 = in1.  -> (bounds [out][2], coeffs [out][ksize], ksize) as `resample_tables`."""
    support, center = 2.0, float(in_size if at_end else 0)
    ksize = int(math.ceil(support)) * 2 + 1
    xmin = max(int(center - support + 0.5), 0)
    xmax = min(int(center + support + 0.5), in_size) - xmin
    w = [resample._bicubic((x + xmin - center + 0.5) * 1.0) for x in range(xmax)]
    ww = 0.0
    for v in w:
        ww += v
    if ww != 0.0:
        w = [v / ww for v in w]
    one = float(1 << resample.PRECISION_BITS)
    k = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
    bounds = np.tile(np.array([[xmin, xmax]], np.int32), (out_size, 1))
    coeffs = np.zeros((out_size, ksize), np.int32)
    coeffs[:, :xmax] = k
    return bounds, coeffs, ksize


def fill_geometry(iw, ih, width, height):
    """`_resize_and_fill`'s numbers -> (src_w, src_h, ox, oy, band): the resized size, where it lands in the frame and which bands are
    drawn: "rows" (above and below, oy of them each side at the top), "cols" or None."""
    ratio, src_ratio = width / height, iw / ih
    src_w, src_h = _fit_sizes(iw, ih, width, height, False)
    ox, oy = width // 2 - src_w // 2, height // 2 - src_h // 2
    band = "rows" if ratio < src_ratio and oy > 0 else "cols" if ratio > src_ratio and ox > 0 else None
    return src_w, src_h, ox, oy, band


def resize_and_fill_reference(image_u8, width, height):
    """`np.array(VaeImageProcessor()._resize_and_fill(Image.fromarray(image_u8), width, height))` for uint8 [H][W][3]."""
    a = np.asarray(image_u8)
    src_w, src_h, ox, oy, band = fill_geometry(a.shape[1], a.shape[0], width, height)
    if min(src_w, src_h) < 1:
        raise ValueError(f"resize fill: a {a.shape[1]} x {a.shape[0]} image leaves nothing in a {width} x {height} frame")
    resized = resample.resize_reference(a, (src_h, src_w), "lanczos")
    res = np.zeros((height, width, 3), np.uint8)
    x0, y0, sx, sy, w, h = _paste_geometry(src_w, src_h, width, height)
    res[y0:y0 + h, x0:x0 + w] = resized[sy:sy + h, sx:sx + w]
    if band == "rows":
        for at_end, y in ((False, 0), (True, oy + src_h)):
            b, c, _ = band_tables(src_h, at_end, oy)
            strip = resample.apply_tables(resized, b, c)
            hh = min(oy, height - y)
            res[y:y + hh] = strip[:hh]
    elif band == "cols":
        for at_end, x in ((False, 0), (True, ox + src_w)):
            b, c, _ = band_tables(src_w, at_end, ox)
            strip = resample.apply_tables(resized.transpose(1, 0, 2), b, c).transpose(1, 0, 2)
            ww = min(ox, width - x)
            res[:, x:x + ww] = strip[:, :ww]
    return res


def apply_overlay_reference(mask_u8, init_u8, image_u8, crop_coords=None):
    """`np.array(VaeImageProcessor().apply_overlay(mask, init_image, image, crop_coords))` for mask uint8 [H][W], init and image uint8
    [..][..][3].  init and mask are resized to the image's frame with lanczos when they differ, as the reference does."""
    mask, init, image = np.asarray(mask_u8), np.asarray(init_u8), np.asarray(image_u8)
    H, W = image.shape[:2]
    if init.shape[:2] != (H, W):
        init = resample.resize_reference(init, (H, W), "lanczos")
    if mask.shape[:2] != (H, W):
        mask = resample.resize_reference(mask[:, :, None], (H, W), "lanczos")[:, :, 0]
    if crop_coords is not None:
        x, y, x2, y2 = (int(v) for v in crop_coords)
        patch = resize_and_crop_reference(image, x2 - x, y2 - y)
        image = np.zeros((H, W, 3), np.uint8)
        cx0, cy0, cx1, cy1 = max(x, 0), max(y, 0), min(x2, W), min(y2, H)
        if cx1 > cx0 and cy1 > cy0:
            image[cy0:cy1, cx0:cx1] = patch[cy0 - y:cy1 - y, cx0 - x:cx1 - x]
    return overlay_pixels(init, mask[:, :, None], image)


# ---- the device side ------------------------------------------------------------------------------------------------------------------

def _no_cpu(what):
    return _lib.BlobCtrlHipError(f"blobctrl_amd.overlay.{what} runs on MI355X only; there is no CPU fallback")


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _device_masks(masks, what):
    """uint8 (or bool) device tensor [n][H][W] or [H][W] -> (contiguous uint8 [n][H][W], whether a batch axis was added)."""
    if not torch.is_tensor(masks):
        raise TypeError(f"{what} takes a torch tensor")
    if masks.device.type != "cuda":
        raise _no_cpu(what)
    if masks.dtype not in (torch.bool, torch.uint8) or masks.ndim not in (2, 3) or 0 in masks.shape:
        raise ValueError(f"{what} takes uint8 masks [n][H][W] or [H][W], not {masks.dtype} {tuple(masks.shape)}")
    m = (masks[None] if masks.ndim == 2 else masks).contiguous()
    if max(m.shape[1:]) > _lib.EDIT_MAX_DIM:
        raise ValueError(f"{what}: a frame of {m.shape[1]} x {m.shape[2]} is outside 1 .. {_lib.EDIT_MAX_DIM} a side")
    return (m.view(torch.uint8) if m.dtype == torch.bool else m), masks.ndim == 2


def _device_images(images, what):
    if torch.is_tensor(images) and images.device.type != "cuda":
        raise _no_cpu(what)
    return resample._device_images(images, what)


@torch.no_grad()
def mask_bounds(masks):
    """bc_mask_bounds: (first column, last column, first row, last row) with a non-zero pixel, four -1 for an empty mask.  masks uint8 device
    [n][H][W] or [H][W] -> int32 device [n][4] or [4]."""
    m, squeeze = _device_masks(masks, "mask_bounds")
    n, H, W = m.shape
    ext = torch.empty((n, H, 2), dtype=torch.int32, device=m.device)
    out = torch.empty((n, 4), dtype=torch.int32, device=m.device)
    with torch.cuda.device(m.device):
        _lib.check(_lib.load().bc_mask_bounds(m.data_ptr(), n, H, W, ext.data_ptr(), out.data_ptr(), _stream(m.device)), "bc_mask_bounds")
    return out[0] if squeeze else out


@torch.no_grad()
def crop_region(masks, width, height, pad=0):
    """`VaeImageProcessor.get_crop_region(mask, width, height, pad)` for a device mask [H][W] -> (x1, y1, x2, y2), or for a batch [n][H][W]
    -> a list of n.  Sixteen bytes a mask come to the host; the box arithmetic is the reference's, on them.  An empty mask is a ValueError."""
    m, squeeze = _device_masks(masks, "crop_region")
    boxes = [crop_region_from_bounds(b, m.shape[2], m.shape[1], width, height, pad) for b in mask_bounds(m).cpu().tolist()]
    return boxes[0] if squeeze else boxes


@torch.no_grad()
def blur(masks, blur_factor=4):
    """`VaeImageProcessor.blur`: `ImageFilter.GaussianBlur(blur_factor)` of every mask, uint8 device [n][H][W] or [H][W] -> the same shape,
    Pillow's bytes: bc_box_blur3_rows, then bc_box_blur3_cols.  A blur factor the kernels do not take raises ValueError, by name."""
    prm = blur_params(blur_factor)
    m, squeeze = _device_masks(masks, "blur")
    if prm is None:
        out = m.clone()
    else:
        n, H, W = m.shape
        tmp, out = torch.empty_like(m), torch.empty_like(m)
        with torch.cuda.device(m.device):
            lib = _lib.load()
            _lib.check(lib.bc_box_blur3_rows(m.data_ptr(), n, H, W, *prm, tmp.data_ptr(), _stream(m.device)), "bc_box_blur3_rows")
            _lib.check(lib.bc_box_blur3_cols(tmp.data_ptr(), n, H, W, *prm, out.data_ptr(), _stream(m.device)), "bc_box_blur3_cols")
    return out[0] if squeeze else out


@functools.lru_cache(maxsize=32)
def _device_band_tables(in_size, at_end, count, device):
    """`band_tables` in device memory, kept per device like `resample._device_tables`: an upload is a synchronising copy."""
    b, c, ksize = band_tables(in_size, at_end, count)
    return torch.from_numpy(b).to(device), torch.from_numpy(c).to(device), ksize


def _band(resized, axis, at_end, count, keep):
    """`keep` lines of `_resize_and_fill`'s band of `count` lines at one end of `axis` (1 rows, 2 columns) of resized [n][h][w][3]: the
    existing resample launch of that axis with `band_tables`."""
    tabs = _device_band_tables(resized.shape[axis], at_end, count, str(resized.device))
    return resample.apply_axis_tables(resized, axis, tabs, keep, "resize_fill")


@torch.no_grad()
def resize_fill(images, width, height):
    """`VaeImageProcessor.resize(image, height, width, resize_mode="fill")` (`_resize_and_fill`) for uint8 device images [n][H][W][3] or
    [H][W][3]: lanczos to the largest size of the image's ratio that fits, centred, the bands beside it filled as Pillow fills them."""
    x, squeeze = _device_images(images, "resize_fill")
    n, H, W, _ = x.shape
    src_w, src_h, ox, oy, band = fill_geometry(W, H, int(width), int(height))
    if min(src_w, src_h) < 1:
        raise ValueError(f"resize fill: a {W} x {H} image leaves nothing in a {width} x {height} frame")
    resized = resample.resize_images(x, (src_h, src_w), "lanczos")
    if (src_w, src_h) == (width, height):
        res = resized
    else:
        res = torch.zeros((n, height, width, 3), dtype=torch.uint8, device=x.device)
        x0, y0, sx, sy, w, h = _paste_geometry(src_w, src_h, width, height)
        res[:, y0:y0 + h, x0:x0 + w] = resized[:, sy:sy + h, sx:sx + w]
        with torch.cuda.device(x.device):
            if band == "rows":
                for at_end, y in ((False, 0), (True, oy + src_h)):
                    keep = min(oy, height - y)
                    if keep > 0:
                        res[:, y:y + keep] = _band(resized, 1, at_end, oy, keep)
            elif band == "cols":
                for at_end, xx in ((False, 0), (True, ox + src_w)):
                    keep = min(ox, width - xx)
                    if keep > 0:
                        res[:, :, xx:xx + keep] = _band(resized, 2, at_end, ox, keep)
    return res[0] if squeeze else res


@torch.no_grad()
def resize_fit(images, width, height):
    """`VaeImageProcessor.resize(image, height, width, resize_mode="crop")` (`_resize_and_crop`) for uint8 device images: lanczos to the
    smallest size of the image's ratio that covers the frame, centred, the excess cut.  Only the window that lands in the frame is resampled."""
    x, squeeze = _device_images(images, "resize_fit")
    n, H, W, _ = x.shape
    width, height = int(width), int(height)
    src_w, src_h = _fit_sizes(W, H, width, height, True)
    x0, y0, sx, sy, w, h = _paste_geometry(src_w, src_h, width, height)
    part = resample.resize_images(x, (src_h, src_w), "lanczos", window=(sy, sx, h, w))
    if (w, h) == (width, height):
        res = part
    else:
        res = torch.zeros((n, height, width, 3), dtype=torch.uint8, device=x.device)
        res[:, y0:y0 + h, x0:x0 + w] = part
    return res[0] if squeeze else res


def _crop_box(crop, H, W, what):
    x1, y1, x2, y2 = (int(v) for v in crop)
    if not (0 <= x1 < x2 <= W and 0 <= y1 < y2 <= H):
        raise ValueError(f"{what}: the box {(x1, y1, x2, y2)} is empty or leaves the {H} x {W} frame")
    return x1, y1, x2, y2


@torch.no_grad()
def crop_and_resize(image, crop, size):
    """`image.crop(crop)` then `resize(..., resize_mode="fill")` to size = (height, width): the zoomed frame the model edits.  image uint8
    device [H][W][3] (or a batch), crop = (x1, y1, x2, y2) inside it."""
    x, squeeze = _device_images(image, "crop_and_resize")
    x1, y1, x2, y2 = _crop_box(crop, x.shape[1], x.shape[2], "crop_and_resize")
    res = resize_fill(x[:, y1:y2, x1:x2].contiguous(), int(size[1]), int(size[0]))
    return res[0] if squeeze else res


@torch.no_grad()
def apply_overlay(mask, init_image, image, crop_coords=None):
    """`VaeImageProcessor.apply_overlay(mask, init_image, image, crop_coords)` on the device: the original shows through where the mask is
    0, the result where it is 255, Pillow's blend between.  mask uint8 [h][w], init_image uint8 [h'][w'][3], image uint8 [H][W][3] or
    [n][H][W][3] (num_images_per_prompt results against one original) -> the shape of image.  The frame is the image's: init and mask are
    resized to it with lanczos when they differ, as the reference does.  With crop_coords = (x1, y1, x2, y2) the image is resized into that
    box (`_resize_and_crop`) and pasted there; outside the box the destination is black, as the reference's transparent base is."""
    what = "apply_overlay"
    img, squeeze = _device_images(image, what)
    init, one = _device_images(init_image, what)
    m, one_m = _device_masks(mask, what)
    if not (one and one_m):
        raise ValueError("apply_overlay takes one init image [H][W][3] and one mask [H][W]")
    if init.device != img.device or m.device != img.device:
        raise ValueError(f"{what}: mask, init_image and image are on different devices")
    n, H, W, _ = img.shape
    if max(H, W) > _lib.EDIT_MAX_DIM:
        raise ValueError(f"{what}: a frame of {H} x {W} is outside 1 .. {_lib.EDIT_MAX_DIM} a side")
    if tuple(init.shape[1:3]) != (H, W):
        init = resample.resize_images(init, (H, W), "lanczos")
    if tuple(m.shape[1:]) != (H, W):
        # a rare path (the caller's mask is normally the frame's): the resize launches take interleaved RGB, so the mask goes through as
        # three equal channels - three times the work and two copies, for not having a one-channel variant of two kernels
        m = resample.resize_images(m[..., None].expand(-1, -1, -1, 3).contiguous(), (H, W), "lanczos")[..., 0].contiguous()
    x, y = 0, 0
    if crop_coords is not None:
        x, y, x2, y2 = (int(v) for v in crop_coords)
        if x2 <= x or y2 <= y:
            raise ValueError(f"{what}: crop_coords {tuple(crop_coords)} is empty")
        img = resize_fit(img, x2 - x, y2 - y)
        cx0, cy0, cx1, cy1 = max(x, 0), max(y, 0), min(x2, W), min(y2, H)
        if cx1 <= cx0 or cy1 <= cy0:
            raise ValueError(f"{what}: crop_coords {tuple(crop_coords)} lies outside the {H} x {W} frame")
        if (cx0, cy0, cx1, cy1) != (x, y, x2, y2):                          # Pillow clips a paste that leaves the frame
            img = img[:, cy0 - y:cy1 - y, cx0 - x:cx1 - x].contiguous()
            x, y = cx0, cy0
    h, w = img.shape[1:3]
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=img.device)
    with torch.cuda.device(img.device):
        _lib.check(_lib.load().bc_overlay_composite(init.data_ptr(), m.data_ptr(), img.data_ptr(), n, H, W, h, w, x, y, out.data_ptr(),
                                                    _stream(img.device)), "bc_overlay_composite")
    return out[0] if squeeze else out


@torch.no_grad()
def to_uint8(images_f, do_denormalize=True):
    """The bytes of `VaeImageProcessor.postprocess(images, "pil")` without leaving the device: fp [n][3][h][w] in [-1, 1] -> uint8
    [n][h][w][3]: / 2 + 0.5, clamp, * 255, round half to even (numpy's `round`, and torch's).  do_denormalize=False is postprocess's: the
    images are in [0, 1] already (what the engine returns for output_type="pt")."""
    if not torch.is_tensor(images_f):
        raise TypeError("to_uint8 takes a torch tensor")
    if images_f.device.type != "cuda":
        raise _no_cpu("to_uint8")
    if images_f.ndim != 4 or images_f.shape[1] != 3 or not images_f.is_floating_point():
        raise ValueError(f"to_uint8 takes floating-point images [n][3][h][w], not {images_f.dtype} {tuple(images_f.shape)}")
    x = ((images_f / 2 + 0.5).clamp(0, 1) if do_denormalize else images_f).permute(0, 2, 3, 1).float()
    return (x * 255).round().to(torch.uint8).contiguous()


def map_ellipse(ellipse, origin, scale, ox, oy):
    """((xc, yc), (d1, d2), angle) of the whole frame -> the same ellipse in the zoomed frame: the crop's origin removed, the uniform scale
    of the fill resize about pixel centres, the fill offsets added; the angle is unchanged."""
    (xc, yc), (d1, d2), angle = ellipse
    return (((xc - origin[0] + 0.5) * scale - 0.5 + ox, (yc - origin[1] + 0.5) * scale - 0.5 + oy), (d1 * scale, d2 * scale), angle)


@torch.no_grad()
def zoom_edit(image, start_ellipse, target_ellipse, height=512, width=512, pad=32):
    """The front of a zoomed edit: image uint8 device [H][W][3] and the edit's two ellipses in its frame -> (crop (x1, y1, x2, y2), the
    cropped frame blown up to height x width uint8 [height][width][3], the union mask of both ellipses uint8 [H][W], start and target
    ellipses mapped into the zoomed frame).  A caller runs `build_edit_inputs_batch` and the pipeline in that frame, then
    `apply_overlay(blur(mask, f), image, to_uint8(result), crop)`."""
    from .edit_inputs import ellipse_masks
    x, squeeze = _device_images(image, "zoom_edit")
    if not squeeze:
        raise ValueError("zoom_edit takes one image [H][W][3]")
    H, W = x.shape[1:3]
    mask = ellipse_masks([start_ellipse, target_ellipse], H, W, device=x.device).amax(0)
    crop = crop_region(mask, width, height, pad)
    x1, y1, x2, y2 = crop
    src_w, _, ox, oy, _ = fill_geometry(x2 - x1, y2 - y1, int(width), int(height))
    s = src_w / (x2 - x1)
    zoomed = crop_and_resize(x[0], crop, (height, width))
    return crop, zoomed, mask, map_ellipse(start_ellipse, (x1, y1), s, ox, oy), map_ellipse(target_ellipse, (x1, y1), s, ox, oy)
