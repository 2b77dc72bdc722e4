"""Cases shared by tools/make_golden.py:golden_overlay (which runs the vendored VaeImageProcessor on them and writes
tests/golden/overlay.npz), tests/test_overlay_cpu.py and tests/test_overlay_gpu.py.  Inputs are regenerated from seeds on both sides;
the fixture holds the reference's outputs only."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlay.npz")

BLUR_FACTORS = (0.5, 1, 1.5, 2, 3, 4, 8, 16, 32)             # the CPU sweep; at least 2, 4, 8, 16 and 32 must be supported
REQUIRED_FACTORS = (2, 4, 8, 16, 32)
BLUR_FRAMES = ((1, 1), (1, 9), (5, 7), (17, 23), (40, 37), (3, 64))      # (H, W); 64 x 3 (W x H) has R wider than the frame at factor 4 up


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def blob_mask(H, W, seed, hard=False):
    """A uint8 mask [H][W] with flat 0 and 255 regions and noise between: what a blur has to get right at edges and in ramps."""
    r = rng(seed)
    m = r.integers(0, 256, (H, W), dtype=np.uint8)
    y0, y1 = sorted(r.integers(0, H + 1, 2).tolist())
    x0, x1 = sorted(r.integers(0, W + 1, 2).tolist())
    m[y0:y1, x0:x1] = 255
    m[: H // 3, : W // 4] = 0
    return ((m > 127) * 255).astype(np.uint8) if hard else m


def rgb_image(H, W, seed):
    return rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def box_mask(H, W, x0, y0, x1, y1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 255
    return m


# name -> (mask frame (H, W), set box (x0, y0, x1, y1) half-open, processing (width, height), pad)
CROP_CASES = {
    "touch_left": ((48, 64), (0, 10, 9, 30), (512, 512), 4),
    "touch_right": ((48, 64), (50, 10, 64, 30), (512, 512), 4),
    "touch_top": ((48, 64), (20, 0, 40, 7), (512, 512), 4),
    "touch_bottom": ((48, 64), (20, 40, 40, 48), (512, 512), 4),
    "same_ratio": ((96, 128), (30, 20, 62, 52), (512, 512), 0),
    "same_ratio_43": ((96, 128), (20, 20, 60, 50), (640, 480), 0),
    "wider": ((96, 128), (10, 40, 90, 50), (512, 512), 8),
    "taller": ((96, 128), (60, 5, 70, 85), (512, 512), 8),
    "wider_at_bottom": ((96, 128), (10, 88, 90, 96), (512, 512), 2),
    "taller_at_right": ((96, 128), (120, 5, 128, 85), (512, 384), 2),
    "wider_than_frame_is_tall": ((40, 128), (4, 10, 120, 20), (512, 512), 0),
    "pad_larger_than_frame": ((40, 56), (20, 15, 30, 25), (512, 512), 100),
    "single_pixel": ((33, 47), (21, 13, 22, 14), (512, 512), 0),
    "single_pixel_corner": ((33, 47), (46, 32, 47, 33), (512, 384), 3),
    "odd_ratio": ((81, 97), (13, 29, 57, 44), (448, 320), 5),
}

# name -> (frame (H, W), crop box (x1, y1, x2, y2) or None, seed).  init, mask and image all live in the frame; with a crop the image (of
# the frame's size, as the reference requires) is resized into the box with `_resize_and_crop`.  Small frames: the fixture holds an output
# of each (the 37 x 53 frame of the composite launch's own test is checked against the host restatement instead).
OVERLAY_CASES = {
    "no_crop": ((19, 27), None, 11),
    "crop_inner": ((19, 27), (3, 2, 19, 18), 12),
    "crop_origin": ((19, 27), (0, 0, 10, 7), 13),
    "crop_far_corner": ((19, 27), (17, 10, 27, 19), 14),
    "crop_one_pixel": ((19, 27), (9, 5, 10, 6), 15),
}


def overlay_frame_inputs(H, W, seed):
    """(mask uint8 [H][W] with all 256 values present and flat 0 / 255 regions, init uint8 [H][W][3], image uint8 [H][W][3]); H * W >= 256."""
    r = rng(seed)
    mask = r.integers(0, 256, (H, W), dtype=np.uint8)
    mask[H // 2:, : W // 3] = 0
    mask[H // 2:, 2 * W // 3:] = 255
    mask.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    return mask, rgb_image(H, W, seed + 100), rgb_image(H, W, seed + 200)


def overlay_inputs(name):
    """(mask, init, image, crop) of a case of OVERLAY_CASES."""
    (H, W), crop, seed = OVERLAY_CASES[name]
    return overlay_frame_inputs(H, W, seed) + (crop,)


# init and mask of another size than the image: the reference resizes both with lanczos first
OVERLAY_RESIZED = {"frame": (18, 26), "init": (25, 36), "mask": (13, 19), "seed": 31}


def overlay_resized_inputs():
    c = OVERLAY_RESIZED
    return (blob_mask(*c["mask"], c["seed"]), rgb_image(*c["init"], c["seed"] + 1), rgb_image(*c["frame"], c["seed"] + 2))


# name -> (image (H, W), (width, height) to fit into, seed): fill with row bands, with column bands, without bands; crop both ways
RESIZE_CASES = {
    "rows_band": ((15, 32), (24, 20), 41),
    "cols_band": ((25, 15), (28, 24), 42),
    "exact": ((10, 15), (30, 20), 43),
    "down_rows": ((45, 80), (32, 24), 44),
    "down_cols": ((49, 26), (20, 32), 45),
    "one_px_band": ((31, 32), (32, 32), 46),
}

BLUR_GOLDEN = {"b4": ((30, 27), 4, 51), "b2_hard": ((17, 23), 2, 52), "b8": ((21, 40), 8, 53), "b1": ((17, 23), 1, 54)}


def golden():
    return np.load(GOLDEN)
