"""Pillow's 8-bit resize on the GPU (include/blobctrl_resample.h, csrc/image_resample.hip): the resampling in front of DINOv2, SAM and the
VAE, without the pixels crossing to the host.  Device tensors in, device tensors out, on the current stream.

Every resize on the edit path is `PIL.Image.resize` of an RGB image, and that is ONE algorithm (Pillow's `ImagingResample`, 8 bits per
channel): a separable convolution whose coefficients are computed in doubles, rounded to fixed point with 22 fraction bits, and applied in
int32 - the horizontal pass first, into a uint8 intermediate, the vertical pass second, a pass whose side does not change skipped.  The host
half of this module restates it: `resample_tables` builds the tables exactly as Pillow's `precompute_coeffs` and `normalize_coeffs_8bpc` do
(Python floats are C doubles, one operation at a time in Pillow's order), `resize_reference` applies them in numpy.  Both run without a
GPU; tests/test_image_resample_cpu.py holds them to `Image.resize` on every pixel.  The device applies the same tables with the same
integer arithmetic, so its bytes are Pillow's, with no tolerance.

What follows a resize on the host - /255, mean and std for DINOv2 and for SAM - is a function of one byte and its channel.  The device does
not redo that arithmetic: the Python layer evaluates the host processor's own expression for the 256 byte values of each channel and the
vertical pass looks the result up (`float[3][256]`), so no rounding can differ.

No CPU fallback: a CPU tensor raises `BlobCtrlHipError`, here, before the library is called (the entry points take raw addresses).
"""
import functools
import math

import numpy as np
import torch

from . import _lib

PRECISION_BITS = 22                                   # Pillow: 32 - 8 - 2
FILTERS = ("bilinear", "bicubic", "lanczos")
FILTER_SUPPORT = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}


def _bilinear(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_FILTER = {"bilinear": _bilinear, "bicubic": _bicubic, "lanczos": _lanczos}


def _filter_name(resample):
    if resample not in FILTERS:
        raise ValueError(f"resample must be one of {FILTERS}, got {resample!r}")
    return resample


def _sizes(in_size, out_size, what):
    in_size, out_size = int(in_size), int(out_size)
    if not (1 <= in_size <= _lib.EDIT_MAX_DIM and 1 <= out_size <= _lib.EDIT_MAX_DIM):
        raise ValueError(f"{what}: a side of {in_size} -> {out_size} is outside 1 .. {_lib.EDIT_MAX_DIM}")
    return in_size, out_size


@functools.lru_cache(maxsize=64)
def _tables(in_size, out_size, resample):
    fn, scale = _FILTER[resample], in_size / out_size
    filterscale = max(scale, 1.0)
    support = FILTER_SUPPORT[resample] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, ksize), dtype=np.int32)
    ss, one = 1.0 / filterscale, float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        coeffs[xx, :xmax] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs, ksize


def resample_tables(in_size, out_size, resample):
    """Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc` for one axis -> (bounds int32 [out][2] = (first source index, taps), coeffs
    int32 [out][ksize] in units of 2^-22, zero past a row's taps, ksize).  The arrays are shared and read-only."""
    in_size, out_size = _sizes(in_size, out_size, "resample_tables")
    return _tables(in_size, out_size, _filter_name(resample))


def identity_tables(size):
    """The tables of a pass that changes nothing: one tap of weight 1.0 on the same index ((2^21 + 2^22 p) >> 22 == p)."""
    bounds = np.stack([np.arange(size, dtype=np.int32), np.ones(size, dtype=np.int32)], 1)
    return bounds, np.full((size, 1), 1 << PRECISION_BITS, dtype=np.int32), 1


def accumulator_bound(coeffs):
    """The largest |2^21 + sum pixel * k| a table can reach over uint8 pixels; the passes accumulate in int32, so it must stay below 2^31."""
    return 255 * int(np.abs(coeffs.astype(np.int64)).sum(1).max()) + (1 << (PRECISION_BITS - 1))


def apply_tables(a, bounds, coeffs):
    """One pass along axis 0 of `a` uint8 [in][...] -> uint8 [out][...]: out[i] = clamp((2^21 + sum_k coeffs[i][k] * a[bounds[i][0] + k])
    >> 22, 0, 255) over k < bounds[i][1], in int32.  A tap whose source index is outside [0, in) contributes nothing - `resample_tables`
    produces none, and the kernels guard the same way because they cannot inspect a table in device memory."""
    in_size = a.shape[0]
    out = np.empty((len(bounds),) + a.shape[1:], dtype=np.uint8)
    for i, ((lo, cnt), k) in enumerate(zip(bounds.tolist(), coeffs)):
        acc = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int32)
        for j in range(min(cnt, coeffs.shape[1])):
            if 0 <= lo + j < in_size:
                acc += a[lo + j].astype(np.int32) * k[j]
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_reference(array_u8, size, resample):
    """`np.array(Image.fromarray(array_u8).resize((out_w, out_h), resample))` in numpy, for array_u8 uint8 [H][W][C] and size = (out_h,
    out_w): the horizontal pass into a uint8 intermediate unless the width stays, then the vertical pass unless the height stays."""
    a = np.asarray(array_u8)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError("resize_reference takes a uint8 array [H][W][C]")
    (H, W), (oh, ow) = a.shape[:2], size
    if ow != W:
        bx, cx, _ = resample_tables(W, ow, resample)
        a = apply_tables(a.transpose(1, 0, 2), bx, cx).transpose(1, 0, 2)
    if oh != H:
        by, cy, _ = resample_tables(H, oh, resample)
        a = apply_tables(a, by, cy)
    return np.array(a, order="C")                                          # (a copy when both passes are skipped, as Pillow's is)


# ---- the device side ----------------------------------------------------------------------------------------------------------------

def _no_cpu(what):
    return _lib.BlobCtrlHipError(f"blobctrl_amd.resample.{what} runs on MI355X only; there is no CPU fallback")


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


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


@functools.lru_cache(maxsize=64)
def _device_tables(in_size, out_size, resample, device):
    """(bounds, coeffs, ksize) of one axis in device memory; resample None is the identity pass.  Kept per device: an app resizes to the same
    few sizes over and over, and a table is a few KiB."""
    b, c, ksize = identity_tables(in_size) if resample is None else _tables(in_size, out_size, resample)
    assert accumulator_bound(c) < 2 ** 31
    return torch.from_numpy(b.copy()).to(device), torch.from_numpy(c.copy()).to(device), ksize


def _window(window, oh, ow, what):
    y0, x0, ch, cw = (0, 0, oh, ow) if window is None else (int(v) for v in window)
    if not (0 <= y0 and 0 <= x0 and ch >= 1 and cw >= 1 and y0 + ch <= oh and x0 + cw <= ow):
        raise ValueError(f"{what}: window {(y0, x0, ch, cw)} (y0, x0, h, w) leaves the resized frame of {oh} x {ow}")
    return y0, x0, ch, cw


def source_rows(H, oh, resample, y0, ch):
    """The source rows [r0, r0 + rows) the vertical pass reads for output rows [y0, y0 + ch): all the horizontal pass has to produce."""
    if oh == H:
        return y0, ch
    b = resample_tables(H, oh, resample)[0][y0:y0 + ch].astype(np.int64)
    r0 = int(b[:, 0].min())
    return r0, int((b[:, 0] + b[:, 1]).max()) - r0


def temp_shape(H, W, size, resample, window=None):
    """(rows, w, 3) of the uint8 intermediate `resize_images` needs per image for this resize, None when it needs none (at most one pass
    runs).  A caller who passes `tmp=` sizes it n times this."""
    (H, oh), (W, ow) = _sizes(H, size[0], "temp_shape"), _sizes(W, size[1], "temp_shape")
    y0, _, ch, cw = _window(window, oh, ow, "temp_shape")
    if ow == W or oh == H:
        return None
    return (source_rows(H, oh, _filter_name(resample), y0, ch)[1], cw, 3)


def _horizontal(lib, x, r0, rows, tx, ow, x0, cw, tmp, what):
    n, H, W, _ = x.shape
    _lib.check(lib.bc_resample_horizontal(x.data_ptr(), n, H, W, r0, rows, tx[0].data_ptr(), tx[1].data_ptr(), tx[2], ow, x0, cw,
                                          tmp.data_ptr(), _stream(x.device)), f"{what}: bc_resample_horizontal")


def _vertical(lib, src, n, IH, IW, r0, xin0, ty, oh, y0, ch, cw, out_u8, out_f32, lut, PH, PW, what):
    _lib.check(lib.bc_resample_vertical(src.data_ptr(), n, IH, IW, r0, xin0, ty[0].data_ptr(), ty[1].data_ptr(), ty[2], oh, y0, ch, cw,
                                        out_u8.data_ptr() if out_u8 is not None else None, out_f32.data_ptr() if out_f32 is not None else None,
                                        lut.data_ptr() if lut is not None else None, PH, PW, _stream(src.device)),
               f"{what}: bc_resample_vertical")


def _temp(tmp, shape, device, what):
    if tmp is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    need = math.prod(shape)
    if not (torch.is_tensor(tmp) and tmp.device == device and tmp.dtype == torch.uint8 and tmp.is_contiguous() and tmp.numel() >= need):
        raise ValueError(f"{what}: tmp must be a contiguous uint8 tensor of at least {need} bytes on {device} (temp_shape per image)")
    return tmp.view(-1)[:need].view(shape)


@torch.no_grad()
def resize_images(images, size, resample="lanczos", window=None, out=None, tmp=None):
    """`Image.resize((out_w, out_h), resample)` of every image: uint8 device [n][H][W][3] or [H][W][3], size = (out_h, out_w), resample
    "bilinear" | "bicubic" | "lanczos" -> uint8 [n][oh][ow][3] (or [oh][ow][3]), the same bytes as Pillow.  `window` = (y0, x0, h, w) returns
    that part of the resized frame only and resamples nothing outside it.  `out` (contiguous, of the result's shape) and `tmp` (contiguous
    uint8, at least n x `temp_shape` bytes) let a caller provide the memory.  This is what a caller runs before handing `encode_latents` a
    device image of another size (the VAE's host preprocessing resizes with lanczos)."""
    what = "resize_images"
    x, squeeze = _device_images(images, what)
    resample = _filter_name(resample)
    n, H, W, _ = x.shape
    (H, oh), (W, ow) = _sizes(H, size[0], what), _sizes(W, size[1], what)
    y0, x0, ch, cw = _window(window, oh, ow, what)
    shape = (ch, cw, 3) if squeeze else (n, ch, cw, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    elif not (torch.is_tensor(out) and out.device == x.device and out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()):
        raise ValueError(f"{what}: out must be a contiguous uint8 tensor {shape} on {x.device}")
    dev = str(x.device)
    with torch.cuda.device(x.device):
        lib = _lib.load()
        if ow == W and oh == H:
            out.view(n, ch, cw, 3).copy_(x[:, y0:y0 + ch, x0:x0 + cw])
        elif oh == H:
            _horizontal(lib, x, y0, ch, _device_tables(W, ow, resample, dev), ow, x0, cw, out, what)
        elif ow == W:
            _vertical(lib, x, n, H, W, 0, x0, _device_tables(H, oh, resample, dev), oh, y0, ch, cw, out, None, None, 0, 0, what)
        else:
            r0, rows = source_rows(H, oh, resample, y0, ch)
            t = _temp(tmp, (n, rows, cw, 3), x.device, what)
            _horizontal(lib, x, r0, rows, _device_tables(W, ow, resample, dev), ow, x0, cw, t, what)
            _vertical(lib, t, n, rows, cw, r0, 0, _device_tables(H, oh, resample, dev), oh, y0, ch, cw, out, None, None, 0, 0, what)
    return out


@torch.no_grad()
def apply_axis_tables(images, axis, tables, lines, what="apply_axis_tables"):
    """One pass with the caller's own tables, for a resampling `resample_tables` does not describe (a box other than the whole axis):
    images uint8 device [n][H][W][3], axis 1 (rows) or 2 (columns), tables = (bounds int32 [out][2], coeffs int32 [out][ksize], ksize) as
    DEVICE tensors, `lines` <= out the number of leading output lines wanted -> uint8 [n][lines][W][3] or [n][H][lines][3]: the device's
    `apply_tables` along that axis."""
    x, _ = _device_images(images, what)
    if images.ndim != 4 or axis not in (1, 2):
        raise ValueError(f"{what} takes a batch [n][H][W][3] and axis 1 or 2")
    n, H, W, _ = x.shape
    bounds, coeffs, ksize = tables
    out_size = bounds.shape[0]
    if not (1 <= lines <= out_size and tuple(coeffs.shape) == (out_size, ksize) and bounds.device == coeffs.device == x.device and
            bounds.dtype == coeffs.dtype == torch.int32 and bounds.is_contiguous() and coeffs.is_contiguous()):
        raise ValueError(f"{what}: tables must be contiguous int32 [out][2] and [out][{ksize}] on {x.device}, and lines within 1 .. out")
    with torch.cuda.device(x.device):
        lib = _lib.load()
        if axis == 1:
            out = torch.empty((n, lines, W, 3), dtype=torch.uint8, device=x.device)
            _vertical(lib, x, n, H, W, 0, 0, tables, out_size, 0, lines, W, out, None, None, 0, 0, what)
        else:
            out = torch.empty((n, H, lines, 3), dtype=torch.uint8, device=x.device)
            _horizontal(lib, x, 0, H, tables, out_size, 0, lines, out, what)
    return out


def _resize_to_planar(x, size, resample, window, lut, frame, what):
    """Resize + lookup: uint8 [n][H][W][3] -> fp32 [n][3][PH][PW] with lut[c][byte] in the window's rows and columns and 0.0 elsewhere.  The
    vertical launch carries the epilogue, so a pass whose side stays runs with the identity table."""
    n, H, W, _ = x.shape
    (H, oh), (W, ow) = _sizes(H, size[0], what), _sizes(W, size[1], what)
    y0, x0, ch, cw = _window(window, oh, ow, what)
    PH, PW = frame
    if PH < ch or PW < cw:
        raise ValueError(f"{what}: a frame of {PH} x {PW} does not hold {ch} x {cw}")
    dev = str(x.device)
    out = torch.empty((n, 3, PH, PW), dtype=torch.float32, device=x.device)
    ty = _device_tables(H, oh, None if oh == H else resample, dev)
    with torch.cuda.device(x.device):
        lib = _lib.load()
        if ow == W:
            _vertical(lib, x, n, H, W, 0, x0, ty, oh, y0, ch, cw, None, out, lut, PH, PW, what)
        else:
            r0, rows = source_rows(H, oh, resample, y0, ch)
            t = torch.empty((n, rows, cw, 3), dtype=torch.uint8, device=x.device)
            _horizontal(lib, x, r0, rows, _device_tables(W, ow, resample, dev), ow, x0, cw, t, what)
            _vertical(lib, t, n, rows, cw, r0, 0, ty, oh, y0, ch, cw, None, out, lut, PH, PW, what)
    return out


def dinov2_lut(processor):
    """`Dinov2ImageProcessor._one`'s expression after the crop, for every byte value of every channel -> float32 [3][256]."""
    arr = np.repeat(np.arange(256, dtype=np.uint8).reshape(256, 1, 1), 3, axis=2)
    arr = arr.astype(np.float32) * np.float32(processor.rescale_factor)
    arr = (arr - np.array(processor.image_mean, np.float32)) / np.array(processor.image_std, np.float32)
    return np.ascontiguousarray(arr.transpose(2, 0, 1).reshape(3, 256))


_LUTS = {}


def _device_lut(key, build, device):
    """A lookup table in device memory, uploaded once per normalisation (`key`) and device: an upload is a synchronising copy."""
    key = key + (str(device),)
    if key not in _LUTS:
        _LUTS[key] = build().to(device)
    return _LUTS[key]


def dinov2_geometry(H, W, shortest_edge, crop_size):
    """((resized h, w), crop window (top, left, crop, crop)) of `Dinov2ImageProcessor._one` for an H x W image."""
    short, long = (W, H) if W <= H else (H, W)
    new_short, new_long = int(shortest_edge), int(shortest_edge * long / short)
    nw, nh = (new_short, new_long) if W <= H else (new_long, new_short)
    crop = int(crop_size)
    if crop > nh or crop > nw:
        raise ValueError(f"dinov2_pixel_values: a crop of {crop} does not fit the resized frame of {nh} x {nw}")
    return (nh, nw), ((nh - crop) // 2, (nw - crop) // 2, crop, crop)


@torch.no_grad()
def dinov2_pixel_values(images, processor):
    """`Dinov2ImageProcessor.preprocess(images)["pixel_values"]` for uint8 device RGB images [n][H][W][3] or [H][W][3] -> fp32
    [n][3][crop][crop] on the device, bit for bit: the bicubic resize of the shortest edge, of the centre crop's rows and columns only, and
    the processor's own normalisation looked up per byte."""
    what = "dinov2_pixel_values"
    x, _ = _device_images(images, what)
    size, window = dinov2_geometry(x.shape[1], x.shape[2], processor.shortest_edge, processor.crop_size)
    lut = _device_lut(("dinov2", float(processor.rescale_factor), tuple(processor.image_mean), tuple(processor.image_std)),
                      lambda: torch.from_numpy(dinov2_lut(processor)), x.device)
    return _resize_to_planar(x, size, "bicubic", window, lut, window[2:], what)


def clip_lut(processor):
    """`CLIPImageProcessor.normalise` - the processor's own expression after the crop - for every byte value of every channel -> float32
    [3][256]."""
    arr = np.repeat(np.arange(256, dtype=np.uint8).reshape(256, 1, 1), 3, axis=2)
    return np.ascontiguousarray(processor.normalise(arr).transpose(2, 0, 1).reshape(3, 256))


@torch.no_grad()
def clip_pixel_values(images, processor):
    """`CLIPImageProcessor.preprocess(images)["pixel_values"]` (blobctrl_amd.image_processor) for uint8 device RGB images [n][H][W][3] or
    [H][W][3] -> fp32 [n][3][crop][crop] on the device, bit for bit: the sibling of dinov2_pixel_values - the same resize kernels on the
    centre crop's window, the processor's own normalisation looked up per byte."""
    what = "clip_pixel_values"
    x, _ = _device_images(images, what)
    size, window = dinov2_geometry(x.shape[1], x.shape[2], processor.shortest_edge, processor.crop_size)
    lut = _device_lut(("clip", float(processor.rescale_factor), tuple(processor.image_mean), tuple(processor.image_std)),
                      lambda: torch.from_numpy(clip_lut(processor)), x.device)
    return _resize_to_planar(x, size, "bicubic", window, lut, window[2:], what)


def sam_lut():
    """`sam.preprocess_image`'s normalisation for every byte value of every channel -> float32 tensor [3][256] (host)."""
    from .sam import PIXEL_MEAN, PIXEL_STD
    x = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(3, 256, 1).float()
    x = (x - torch.tensor(PIXEL_MEAN).view(3, 1, 1)) / torch.tensor(PIXEL_STD).view(3, 1, 1)
    return x.reshape(3, 256).contiguous()


def _sam_rgb(image, image_format, what):
    x, squeeze = _device_images(image, what)
    if not squeeze:
        raise ValueError("set_image takes a uint8 image [H][W][3]")
    if image_format not in ("RGB", "BGR"):
        raise ValueError(f"image_format must be 'RGB' or 'BGR', got {image_format!r}")
    return x.flip(-1).contiguous() if image_format == "BGR" else x


@torch.no_grad()
def sam_pixel_values(image, long_side, image_format="RGB"):
    """The second value of `sam_input` alone (what `SamPredictor.set_image` needs) -> ((h, w) of the resized frame, fp32 [1][3][S][S])."""
    from .sam import preprocess_shape
    x = _sam_rgb(image, image_format, "sam_input")
    S = int(long_side)
    nh, nw = preprocess_shape(x.shape[1], x.shape[2], S)
    return (nh, nw), _resize_to_planar(x, (nh, nw), "bilinear", None, _device_lut(("sam",), sam_lut, x.device), (S, S), "sam_input")


@torch.no_grad()
def sam_input(image, long_side, image_format="RGB"):
    """`sam.preprocess_image` for a uint8 device image [H][W][3] -> (resized uint8 [h][w][3], padded normalised fp32 [1][3][S][S]), both on
    the device and both the host function's bytes.  BGR is a channel flip on the device before the resize."""
    from .sam import preprocess_shape
    x = _sam_rgb(image, image_format, "sam_input")
    nh, nw = preprocess_shape(x.shape[1], x.shape[2], int(long_side))
    resized = resize_images(x[0], (nh, nw), "bilinear")
    S = int(long_side)
    # the frame is the resized image behind an identity pass: one read of h x w x 3 bytes instead of a second resize
    return resized, _resize_to_planar(resized[None], (nh, nw), "bilinear", None, _device_lut(("sam",), sam_lut, x.device), (S, S), "sam_input")
