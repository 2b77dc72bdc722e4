"""Zoomed edits without a GPU: the host restatement of blobctrl_amd/overlay.py against Pillow byte for byte and against the vendored
VaeImageProcessor's recorded outputs (tests/golden/overlay.npz), the binding table of include/blobctrl_overlay.h, and what the entry points
and the Python layer refuse before anything reaches the device."""
import os

import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter, ImageOps

from blobctrl_amd import _lib, image_processor, overlay
from tests import overlay_common as oc

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("bc_box_blur3_rows", "bc_box_blur3_cols", "bc_mask_bounds", "bc_overlay_composite")


def pillow_pixels(c, m, d):
    """apply_overlay's own Pillow calls on 1-pixel-high grey images: init c, mask m, destination d (uint8 [N]) -> uint8 [N]."""
    n = len(c)
    rgb = lambda v: Image.fromarray(np.repeat(v.reshape(1, n, 1), 3, axis=2))
    masked = Image.new("RGBa", (n, 1))
    masked.paste(rgb(c).convert("RGBA").convert("RGBa"), mask=ImageOps.invert(Image.fromarray(m.reshape(1, n)).convert("L")))
    masked = masked.convert("RGBA")
    out = rgb(d).convert("RGBA")
    out.alpha_composite(masked)
    return np.array(out.convert("RGB"))[0, :, 0]


def test_the_pixel_arithmetic_is_pillows_on_all_2_to_the_24_triples():
    c, m = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    c, m = c.reshape(-1), m.reshape(-1)
    for d0 in range(0, 256, 16):                                          # 16 destination values a chunk: 2^20 pixels
        d = np.arange(d0, d0 + 16, dtype=np.uint8)
        cc, mm, dd = np.tile(c, 16), np.tile(m, 16), np.repeat(d, 65536)
        want, got = pillow_pixels(cc, mm, dd), overlay.overlay_pixels(cc, mm, dd)
        assert np.array_equal(want, got), (d0, np.flatnonzero(want != got)[:4])


def pillow_blur(a, factor):
    return np.array(Image.fromarray(a).filter(ImageFilter.GaussianBlur(factor)))


def supported(factor):
    try:
        return overlay.blur_params(factor)
    except ValueError as e:
        assert repr(factor) in str(e) and "not supported" in str(e), e
        return None


def test_the_blur_sweep_is_byte_exact_or_refused_by_name():
    ok = []
    for factor in oc.BLUR_FACTORS:
        prm = supported(factor)
        if prm is None:
            with pytest.raises(ValueError, match="not supported"):
                overlay.gaussian_blur_reference(np.zeros((3, 3), np.uint8), factor)
            continue
        ok.append(factor)
        for i, (H, W) in enumerate(oc.BLUR_FRAMES):
            for hard in (False, True):
                a = oc.blob_mask(H, W, 1000 + i, hard)
                assert np.array_equal(pillow_blur(a, factor), overlay.gaussian_blur_reference(a, factor)), (factor, H, W, hard, prm)
    assert set(oc.REQUIRED_FACTORS) <= set(ok), ok
    assert any(overlay.blur_params(f)[0] > 3 for f in ok)                  # ... the 64 x 3 frame has R wider than its 3 rows
    a = oc.blob_mask(5, 6, 7)
    assert np.array_equal(overlay.gaussian_blur_reference(a, 0), a) and np.array_equal(pillow_blur(a, 0), a)
    for bad in (-1, float("nan"), float("inf"), 200):
        with pytest.raises(ValueError, match="not supported"):
            overlay.blur_params(bad)
    assert overlay.blur_params(64)[0] == overlay.MAX_BLUR_RADIUS == _lib.BLUR_MAX_R


def test_one_line_pass_is_pillows_box_blur():
    a = oc.blob_mask(9, 41, 3)
    for r in (0.25, 0.4, 0.9, 1.0, 2.5, 7.3, 30.0):
        R, ww, fw = overlay.box_weights(np.float32(r))
        assert np.array_equal(np.array(Image.fromarray(a).filter(ImageFilter.BoxBlur((r, 0)))), overlay.box_blur_lines(a, R, ww, fw)), r
        assert np.array_equal(np.array(Image.fromarray(a).filter(ImageFilter.BoxBlur((0, r)))),
                              overlay.box_blur_lines(a.T, R, ww, fw).T), r


def test_the_blur_against_the_reference_processor():
    g = oc.golden()
    for name, ((H, W), factor, seed) in oc.BLUR_GOLDEN.items():
        a = oc.blob_mask(H, W, seed, hard="hard" in name)
        assert np.array_equal(overlay.gaussian_blur_reference(a, factor), g[f"blur_{name}"]), name
        got = image_processor.VaeImageProcessor.blur(Image.fromarray(a), factor)
        assert np.array_equal(np.array(got), g[f"blur_{name}"]), name


def test_crop_regions_are_the_reference_processors():
    g = oc.golden()
    seen = set()
    for name, ((H, W), box, (width, height), pad) in oc.CROP_CASES.items():
        mask = oc.box_mask(H, W, *box)
        want = tuple(int(v) for v in g[f"crop_{name}"])
        assert overlay.crop_region_reference(mask, width, height, pad) == want, name
        assert image_processor.VaeImageProcessor.get_crop_region(Image.fromarray(mask), width, height, pad=pad) == want, name
        x0, y0, x1, y1 = box
        assert overlay.bounds_reference(mask) == (x0, x1 - 1, y0, y1 - 1)
        px0, py0, px1, py1 = max(x0 - pad, 0), max(y0 - pad, 0), min(x1 + pad, W), min(y1 + pad, H)
        seen.add("wider" if (px1 - px0) / (py1 - py0) > width / height else "taller_or_equal")
        seen.add("needs_shift" if want[0] == 0 or want[1] == 0 or want[2] == W or want[3] == H else "free")
    assert seen == {"wider", "taller_or_equal", "needs_shift", "free"}
    assert overlay.bounds_reference(np.zeros((3, 4), np.uint8)) == (-1, -1, -1, -1)
    with pytest.raises(ValueError, match="empty"):
        overlay.crop_region_reference(np.zeros((3, 4), np.uint8), 512, 512)
    with pytest.raises(ValueError, match="empty"):
        image_processor.VaeImageProcessor.get_crop_region(Image.new("L", (4, 3)), 512, 512)


def test_the_resize_helpers_are_pillows_with_bands_and_without():
    g = oc.golden()
    bands = set()
    proc = image_processor.VaeImageProcessor()
    for name, ((H, W), (width, height), seed) in oc.RESIZE_CASES.items():
        img = oc.rgb_image(H, W, seed)
        assert np.array_equal(overlay.resize_and_fill_reference(img, width, height), g[f"fill_{name}"]), name
        assert np.array_equal(overlay.resize_and_crop_reference(img, width, height), g[f"fit_{name}"]), name
        assert np.array_equal(np.array(proc.resize(Image.fromarray(img), height, width, resize_mode="fill")), g[f"fill_{name}"]), name
        assert np.array_equal(np.array(proc.resize(Image.fromarray(img), height, width, resize_mode="crop")), g[f"fit_{name}"]), name
        bands.add(overlay.fill_geometry(W, H, width, height)[4])
    assert bands == {"rows", "cols", None}
    # what Pillow returns for a box of zero extent, directly: every line of the band is the same two-tap bicubic extrapolation of the edge
    img = oc.rgb_image(9, 11, 5)
    for at_end in (False, True):
        e = 9 if at_end else 0
        want = np.array(Image.fromarray(img).resize((11, 3), box=(0, e, 11, e)))
        b, c, _ = overlay.band_tables(9, at_end, 3)
        from blobctrl_amd import resample
        assert np.array_equal(resample.apply_tables(img, b, c), want)


def test_apply_overlay_is_the_reference_processors():
    g = oc.golden()
    proc = image_processor.VaeImageProcessor()
    for name in oc.OVERLAY_CASES:
        mask, init, image, crop = oc.overlay_inputs(name)
        assert len(np.unique(mask)) == 256
        assert np.array_equal(overlay.apply_overlay_reference(mask, init, image, crop), g[f"overlay_{name}"]), name
        got = proc.apply_overlay(Image.fromarray(mask), Image.fromarray(init), Image.fromarray(image), crop)
        assert np.array_equal(np.array(got), g[f"overlay_{name}"]), name
    mask, init, image = oc.overlay_resized_inputs()
    assert np.array_equal(overlay.apply_overlay_reference(mask, init, image), g["overlay_resized"])


def test_binding_table_of_the_overlay_entry_points():
    lib = _lib.load()
    header = open(os.path.join(HERE, "..", "include", "blobctrl_overlay.h")).read()
    assert set(_lib.OVERLAY_SIGNATURES) == set(NAMES)
    entry = open(os.path.join(HERE, "..", "__graft_entry__.py")).read()
    assert '"blobctrl_overlay.h"' in entry and '"overlay.hip"' in entry
    for name in NAMES:
        assert getattr(lib, name) is not None and f"int {name}(" in header
        assert getattr(lib, name).argtypes == _lib.OVERLAY_SIGNATURES[name][1]
        for table in _lib._OP_TABLES + (_lib.EXPORTED_SYMBOLS, _lib.VAE_SIGNATURES, _lib.REQUEST_SIGNATURES, _lib.SAM_SIGNATURES,
                                        _lib.SAM_BATCH_SIGNATURES, _lib.SAM_HOST_SIGNATURES, _lib.MASK_SIGNATURES, _lib.EDIT_SIGNATURES,
                                        _lib.RESAMPLE_SIGNATURES, _lib.IP_SIGNATURES, _lib.IP_PATH_SIGNATURES):
            assert name not in table
        with pytest.raises(KeyError):
            _lib.op_code(name)
    assert len(_lib.EXPORTED_SYMBOLS) == 92 and _lib.IP_OPS == {"bc_attention_ip": 53}
    assert f"#define BC_BLUR_MAX_R {_lib.BLUR_MAX_R}" in header


def refused(fn, args, word):
    lib = _lib.load()
    assert fn(*args, None) == 1, args
    msg = lib.bc_last_error()
    assert word in msg, (args, msg)
    return msg


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Dummy addresses, far enough apart not to overlap: every call below must return before a kernel could touch them."""
    lib = _lib.load()
    p, q, r, s, big = 1 << 30, 2 << 30, 3 << 30, 4 << 30, _lib.EDIT_MAX_DIM + 1

    def vary(fn, good, nulls, dims, word):
        assert fn is not None
        for at in nulls:
            refused(fn, good[:at] + [None] + good[at + 1:], word)
        for at in dims:
            for bad in (0, -1):
                refused(fn, good[:at] + [bad] + good[at + 1:], word)
        for at in dims[1:]:                                                # H and W: oversize frames
            assert b"limit" in refused(fn, good[:at] + [big] + good[at + 1:], word)

    R, ww, fw = overlay.blur_params(4)
    for name in ("bc_box_blur3_rows", "bc_box_blur3_cols"):
        fn, word = getattr(lib, name), name.encode()
        good = [p, 1, 8, 8, R, ww, fw, q]
        vary(fn, good, (0, 7), (1, 2, 3), word)
        for bad in (-1, _lib.BLUR_MAX_R + 1):
            assert b"radius" in refused(fn, [p, 1, 8, 8, bad, ww, fw, q], word)
        assert b"weights" in refused(fn, [p, 1, 8, 8, R, ww + 1, fw, q], word)         # (2 R + 1) ww + 2 fw would pass 2^24
        assert b"weights" in refused(fn, [p, 1, 8, 8, R, -1, fw, q], word)
        assert b"overlaps" in refused(fn, [p, 1, 8, 8, R, ww, fw, p + 63], word)
        assert b"grid" in refused(fn, [p, 1 << 20, 16384, 16384, R, ww, fw, 1 << 62], word)
    vary(lib.bc_mask_bounds, [p, 1, 8, 8, q, r], (0, 4, 5), (1, 2, 3), b"bc_mask_bounds")
    assert b"aligned" in refused(lib.bc_mask_bounds, [p, 1, 8, 8, q + 2, r], b"bc_mask_bounds")
    assert b"aligned" in refused(lib.bc_mask_bounds, [p, 1, 8, 8, q, r + 1], b"bc_mask_bounds")
    good = [p, q, r, 1, 8, 9, 4, 5, 2, 3, s]
    vary(lib.bc_overlay_composite, good, (0, 1, 2, 10), (3, 4, 5), b"bc_overlay_composite")
    for at, bad in ((6, 0), (7, 0), (8, -1), (9, -1), (8, 5), (9, 5), (6, 9), (7, 10)):       # a patch that leaves the 8 x 9 frame
        assert b"leaves the frame" in refused(lib.bc_overlay_composite, good[:at] + [bad] + good[at + 1:], b"bc_overlay_composite")
    assert b"overlaps" in refused(lib.bc_overlay_composite, good[:10] + [p + 8], b"bc_overlay_composite")


def test_the_python_surface_refuses_without_a_gpu():
    m = torch.zeros(6, 7, dtype=torch.uint8)
    img = torch.zeros(6, 7, 3, dtype=torch.uint8)
    e = ((3.0, 3.0), (2.0, 3.0), 10.0)
    proc = image_processor.VaeImageProcessor()
    for call in (lambda: overlay.crop_region(m, 512, 512, 0),
                 lambda: overlay.mask_bounds(m),
                 lambda: overlay.blur(m, 4),
                 lambda: overlay.crop_and_resize(img, (0, 0, 4, 4), (8, 8)),
                 lambda: overlay.resize_fit(img, 8, 8),
                 lambda: overlay.apply_overlay(m, img, img),
                 lambda: overlay.to_uint8(torch.zeros(1, 3, 4, 4)),
                 lambda: overlay.zoom_edit(img, e, e, 8, 8, 1),
                 lambda: proc.blur(m, 4),
                 lambda: proc.get_crop_region(m, 8, 8),
                 lambda: proc.resize(img, 8, 8, resize_mode="fill"),
                 lambda: proc.apply_overlay(m, img, img)):
        with pytest.raises(_lib.BlobCtrlHipError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="not supported"):
        overlay.blur(m, 500)
    with pytest.raises(ValueError, match="resize_mode"):
        proc.resize(Image.new("RGB", (4, 4)), 8, 8, resize_mode="stretch")


def test_the_mapped_ellipse_closed_form_on_the_host():
    """`map_ellipse` is the uniform scale of the fill resize about pixel centres, offsets added; angle unchanged."""
    e = ((40.25, 31.5), (20.0, 10.0), 33.0)
    (cx, cy), (d1, d2), ang = overlay.map_ellipse(e, (10, 20), 4.0, 3, 0)
    assert (cx, cy) == ((40.25 - 10 + 0.5) * 4.0 - 0.5 + 3, (31.5 - 20 + 0.5) * 4.0 - 0.5 + 0) and (d1, d2, ang) == (80.0, 40.0, 33.0)
