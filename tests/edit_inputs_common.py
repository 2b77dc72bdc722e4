"""What tests/test_edit_inputs_cpu.py and tests/test_edit_inputs_gpu.py share: the test ellipses and frames, the numpy reference of the row
extents, the synthetic masks, and the host recomputation of the ellipse predicate's decision values.  The reference of every comparison is
the host code of blobctrl_amd/blob_edit.py - never blobctrl_amd/edit_inputs.py."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAMES = [(37, 45), (1, 1), (1, 130), (64, 64), (24, 257)]
MOVE_HAT_512 = ((361.1067, 367.8526), (85.4812, 103.6543), 87.3739)        # the README's move_hat target blob, in a 512 x 512 frame
EXTENT_WIDTHS = (1, 3, 63, 64, 65, 130, 1030)
EXTENT_HEIGHTS = (1, 7)
# start / target ellipses of the paint and batch tests, in a 64 x 96 frame (they overlap each other)
BATCH_ELLIPSES = [((30.3, 25.7), (22.1, 31.3), 33.3), ((42.9, 33.1), (26.7, 18.3), 101.9), ((70.2, 20.4), (15.3, 40.9), 5.7),
                  ((44.4, 41.3), (30.2, 12.6), 77.1)]


def generic_ellipses(H, W):
    """name -> ellipse, for a frame: none of them decides any pixel on a tie (test_edit_inputs_cpu.py asserts it)."""
    rotated = ((20.3, 17.9), (9.7, 23.1), 33.3) if (H, W) == (37, 45) else \
        ((W * 0.4513 + 0.3, H * 0.4838 + 0.0113), (max(W, 3) * 0.2156 + 0.0371, max(H, 3) * 0.5133 + 0.0177), 33.3)
    return {
        "rotated": rotated,
        "centre_outside": ((-3.217, H + 2.641), (W * 0.9 + 7.313, H * 0.7 + 5.177), 61.7),
        "covers_frame": ((W / 2.0 + 0.123, H / 2.0 - 0.217), (3.1 * (W + H) + 1.37, 2.7 * (W + H) + 0.41), 17.3),
        "misses_frame": ((W + 40.37, -35.21), (9.7, 23.1), 112.9),
    }


def app_dot(H, W):
    """the ellipse the app draws for "no blob": ((W / 2, H / 2), (1e-5, 1e-5), 0)"""
    return ((W / 2, H / 2), (1e-5, 1e-5), 0)


def tie_ellipses(H, W):
    """Ellipses whose arithmetic is exact and that put pixel corners or edges ON the boundary: an integer-centred circle and an axis-aligned
    ellipse, both at angle 0 (cos = 1, sin = 0; half-integer offsets, power-of-two or small-integer axes)."""
    cx, cy = W // 2, H // 2
    return {"circle": ((cx, cy), (9.0, 9.0), 0), "axis_aligned": ((cx, cy), (8.0, 5.0), 0), "circle_r2": ((cx, cy), (4.0, 4.0), 0)}


def decision_margin(ellipse, height, width):
    """min over the frame's pixels of |cu^2 + cv^2 - 1|, |best - 1|, ||X| - 0.5|, ||Y| - 0.5| in `blob_edit.ellipse_mask`'s own arithmetic:
    how far the nearest pixel is from deciding the other way."""
    (xc, yc), (d1, d2), angle = ellipse
    t = math.radians(angle)
    a, b = max(d1 / 2.0, 1e-9), max(d2 / 2.0, 1e-9)
    ct, st = math.cos(t), math.sin(t)
    X, Y = np.meshgrid(np.arange(width, dtype=np.float64) - xc, np.arange(height, dtype=np.float64) - yc)

    def to_disc(x, y):
        return (x * ct + y * st) / a, (-x * st + y * ct) / b
    corners = [to_disc(X + dx, Y + dy) for dx, dy in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5))]
    cu, cv = to_disc(X, Y)
    best = np.full(X.shape, np.inf)
    for k in range(4):
        (pu, pv), (qu, qv) = corners[k], corners[(k + 1) % 4]
        eu, ev = qu - pu, qv - pv
        tt = np.clip(-(pu * eu + pv * ev) / np.maximum(eu * eu + ev * ev, 1e-300), 0.0, 1.0)
        du, dv = pu + tt * eu, pv + tt * ev
        best = np.minimum(best, du * du + dv * dv)
    return float(min(np.abs(cu * cu + cv * cv - 1.0).min(), np.abs(best - 1.0).min(), np.abs(np.abs(X) - 0.5).min(),
                     np.abs(np.abs(Y) - 0.5).min()))


def row_extents_reference(masks):
    """masks [n][H][W] (non-zero = set) -> int32 [n][H][2]: first and last set column of every row, (-1, -1) for an empty row."""
    ind = np.asarray(masks) != 0
    n, H, W = ind.shape
    out = np.full((n, H, 2), -1, dtype=np.int32)
    for i in range(n):
        for y in range(H):
            xs = np.flatnonzero(ind[i, y])
            if len(xs):
                out[i, y] = xs[0], xs[-1]
    return out


def points_and_box(ext):
    """one mask's extents [H][2] -> (points [(first, y) ..., (last, y) ...] of the non-empty rows, box (x, y, w, h) or None)"""
    rows = [(int(f), int(l), y) for y, (f, l) in enumerate(ext) if f >= 0]
    if not rows:
        return np.zeros((0, 2)), None
    pts = np.array([(f, y) for f, _, y in rows] + [(l, y) for _, l, y in rows])
    x0, x1 = min(f for f, _, _ in rows), max(l for _, l, _ in rows)
    return pts, (x0, rows[0][2], x1 - x0 + 1, rows[-1][2] - rows[0][2] + 1)


def host_box(mask):
    """(x, y, w, h) exactly as `blob_edit.object_region_from_mask` takes it from the set pixels"""
    ys, xs = np.nonzero(np.asarray(mask) > 0)
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def extent_masks(H, W, seed=0):
    """name -> uint8 mask [H][W] for the extents tests (non-zero bytes of several values: any of them means set)"""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * H + W))
    out = {"empty": np.zeros((H, W), np.uint8), "full": np.full((H, W), 255, np.uint8)}
    for name, (y, x) in {"corner_tl": (0, 0), "corner_tr": (0, W - 1), "corner_bl": (H - 1, 0), "corner_br": (H - 1, W - 1)}.items():
        out[name] = np.zeros((H, W), np.uint8)
        out[name][y, x] = 1
    out["first_column"] = np.zeros((H, W), np.uint8)
    out["first_column"][:, 0] = 7
    out["last_column"] = np.zeros((H, W), np.uint8)
    out["last_column"][:, W - 1] = 128
    out["sparse"] = (rng.random((H, W)) < 0.001).astype(np.uint8)
    out["dense"] = (rng.random((H, W)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8)
    return out


def synthetic_object_masks():
    """name -> bool mask: shapes an ellipse can be fitted to, for the extents route against `ellipse_from_mask`"""
    yy, xx = np.mgrid[:60, :83]
    disc = ((xx - 40.3) / 21.0) ** 2 + ((yy - 29.1) / 12.5) ** 2 <= 1
    rot = (((xx - 44) * 0.8 + (yy - 30) * 0.6) / 25.0) ** 2 + ((-(xx - 44) * 0.6 + (yy - 30) * 0.8) / 9.0) ** 2 <= 1
    holes = disc.copy()
    holes[25:33, 30:50] = False                         # a hole and ...
    holes[::3] = False                                  # ... empty rows: both routes see the same hull
    two = disc.copy()
    two[2:6, 70:80] = True                              # a detached island is a hull vertex
    return {"disc": disc, "rotated": rot, "holes_and_empty_rows": holes, "with_island": two}


def demo_masks():
    """name -> bool mask of the demo states in tests/golden/blob_edit_cv.npz"""
    z = np.load(os.path.join(GOLDEN, "blob_edit_cv.npz"))
    out = {}
    for name in [str(n) for n in z["names"]]:
        H, W = [int(v) for v in z[f"{name}_shape"]]
        out[name] = np.unpackbits(z[f"{name}_mask"])[: H * W].reshape(H, W).astype(bool)
    return out


def random_image(H, W, seed=5):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (H, W, 3)).astype(np.uint8)
