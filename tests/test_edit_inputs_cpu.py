"""An edit's inputs on the device, without a GPU: the binding table of include/blobctrl_edit.h, what the entry points and the Python layer
refuse before anything reaches the device, the extents route to the ellipse against `blob_edit.ellipse_from_mask`, and the condition the
GPU cover test puts on its own inputs (no generic test ellipse decides a pixel on a tie)."""
import os

import numpy as np
import pytest
import torch

from blobctrl_amd import _lib, blob_edit, edit_inputs
from tests import edit_inputs_common as ec

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("bc_ellipse_cover", "bc_ellipse_paint", "bc_mask_row_extents", "bc_mask_cutout")


def test_binding_table_of_the_edit_entry_points():
    lib = _lib.load()
    header = open(os.path.join(HERE, "..", "include", "blobctrl_edit.h")).read()
    assert set(_lib.EDIT_SIGNATURES) == set(NAMES)
    entry = open(os.path.join(HERE, "..", "__graft_entry__.py")).read()                 # built from its own source, with its header a dependency
    assert '"blobctrl_edit.h"' in entry and '"edit_inputs.hip"' in entry
    for name in NAMES:
        assert getattr(lib, name) is not None and f"int {name}(" in header
        assert getattr(lib, name).argtypes == _lib.EDIT_SIGNATURES[name][1]
        for table in (_lib.OPS, _lib.REQUEST_OPS, _lib.SAM_OPS, _lib.SAM_BATCH_OPS, _lib.EXPORTED_SYMBOLS, _lib.VAE_SIGNATURES,
                      _lib.REQUEST_SIGNATURES, _lib.SAM_SIGNATURES, _lib.SAM_BATCH_SIGNATURES, _lib.SAM_HOST_SIGNATURES, _lib.MASK_SIGNATURES):
            assert name not in table
        with pytest.raises(KeyError):
            _lib.op_code(name)
    assert len(_lib.EXPORTED_SYMBOLS) == 92
    assert f"#define BC_EDIT_MAX_DIM {_lib.EDIT_MAX_DIM}" in header
    assert "BC_OP_COUNT = 53" in open(os.path.join(HERE, "..", "include", "blobctrl_hip.h")).read()


def refused(fn, args, word):
    lib = _lib.load()
    assert fn(*args, None) == 1, args
    msg = lib.bc_last_error()
    assert word in msg, (args, msg)
    return msg


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Dummy addresses: every call below must return before a kernel could touch them."""
    lib = _lib.load()
    p, big = 4096, _lib.EDIT_MAX_DIM + 1

    def vary(fn, good, nulls, dims, word):
        for at in nulls:
            refused(fn, good[:at] + [None] + good[at + 1:], word)
        for at in dims:
            for bad in (0, -1):
                refused(fn, good[:at] + [bad] + good[at + 1:], word)
        for at in dims[1:]:                                                # H and W: oversize frames
            assert b"limit" in refused(fn, good[:at] + [big] + good[at + 1:], word)

    vary(lib.bc_ellipse_cover, [p, 1, 8, 8, p], (0, 4), (1, 2, 3), b"bc_ellipse_cover")
    vary(lib.bc_ellipse_paint, [p, 1, 8, 8, p, p, 2], (0, 4, 5), (1, 2, 3), b"bc_ellipse_paint")
    vary(lib.bc_mask_row_extents, [p, 1, 8, 8, p], (0, 4), (1, 2, 3), b"bc_mask_row_extents")
    vary(lib.bc_mask_cutout, [p, p, p, 1, 8, 8, p], (0, 1, 2, 6), (3, 4, 5), b"bc_mask_cutout")
    for k in (0, -3):
        assert b"k = " in refused(lib.bc_ellipse_paint, [p, 1, 8, 8, p, p, k], b"bc_ellipse_paint")
    # alignment the kernels rely on (fp64 ellipses, int32 extents and boxes), and counts that would not fit the grid
    assert b"aligned" in refused(lib.bc_ellipse_cover, [p + 4, 1, 8, 8, p], b"bc_ellipse_cover")
    assert b"aligned" in refused(lib.bc_ellipse_paint, [p, 1, 8, 8, p + 4, p, 2], b"bc_ellipse_paint")
    assert b"aligned" in refused(lib.bc_mask_row_extents, [p, 1, 8, 8, p + 2], b"bc_mask_row_extents")
    assert b"aligned" in refused(lib.bc_mask_cutout, [p, p, p + 1, 1, 8, 8, p], b"bc_mask_cutout")
    assert b"grid" in refused(lib.bc_ellipse_paint, [p, 1 << 20, 4096, 4096, p, p, 2], b"bc_ellipse_paint")
    assert b"grid" in refused(lib.bc_mask_cutout, [p, p, p, 1 << 20, 4096, 4096, p], b"bc_mask_cutout")


def test_the_python_surface_refuses_without_a_gpu():
    e = ec.MOVE_HAT_512
    m = torch.zeros(2, 6, 7, dtype=torch.bool)
    img = torch.zeros(6, 7, 3, dtype=torch.uint8)
    for call in (lambda: edit_inputs.ellipse_masks([e], 8, 8, device="cpu"),
                 lambda: edit_inputs.row_extents(m),
                 lambda: edit_inputs.row_extents(m[0].to(torch.uint8)),
                 lambda: edit_inputs.ellipses_from_masks(m),
                 lambda: edit_inputs.object_regions(img, m, [(0, 0, 1, 1)] * 2),
                 lambda: edit_inputs.paint_ellipses(img[None], [[e]], [[(0, 0, 0)]]),
                 lambda: edit_inputs.build_edit_inputs_batch(["move"], img, [e], [e], [1.0], device="cpu"),
                 lambda: edit_inputs.build_edit_inputs_batch(["move"], img, [e], [e], [1.0], device="cuda:0"),
                 lambda: edit_inputs.vae_input(img)):
        with pytest.raises(_lib.BlobCtrlHipError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        edit_inputs.row_extents(np.zeros((2, 3, 4), bool))
    with pytest.raises(ValueError, match="not finite"):
        edit_inputs.ellipse_params(((float("nan"), 1.0), (2.0, 3.0), 0.0))
    with pytest.raises(ValueError, match="unknown edit operation"):
        edit_inputs.build_edit_inputs_batch(["shear"], img, [e], [e], [1.0])
    with pytest.raises(ValueError, match="needs a target ellipse"):
        edit_inputs.build_edit_inputs_batch(["remove", "move"], img, [e, e], [None, None], [1.0, 1.0])
    with pytest.raises(ValueError, match="outside 1"):
        edit_inputs.ellipse_masks([e], _lib.EDIT_MAX_DIM + 1, 8)


def test_ellipse_params_are_the_host_functions():
    import math
    row = edit_inputs.ellipse_params(((3, 4.5), (1e-12, 7.0), 33.3))
    t = math.radians(33.3)
    assert row == [3.0, 4.5, 1e-9, 3.5, math.cos(t), math.sin(t)] and all(type(v) is float for v in row)


def test_the_reference_of_the_extents_on_a_hand_made_mask():
    m = np.zeros((1, 4, 6), np.uint8)
    m[0, 1, 2] = m[0, 1, 4] = 9
    m[0, 3, 0] = 1
    assert ec.row_extents_reference(m).tolist() == [[[-1, -1], [2, 4], [-1, -1], [0, 0]]]
    pts, box = ec.points_and_box(ec.row_extents_reference(m)[0])
    assert sorted(map(tuple, pts.tolist())) == [(0, 3), (0, 3), (2, 1), (4, 1)] and box == (0, 1, 5, 3) == ec.host_box(m[0])
    assert ec.points_and_box(ec.row_extents_reference(np.zeros((1, 3, 3)))[0])[1] is None


def check_route(name, mask):
    want = blob_edit.ellipse_from_mask(mask)
    ext = ec.row_extents_reference(mask[None])[0]
    pts, box = ec.points_and_box(ext)
    assert blob_edit.fit_ellipse(blob_edit.convex_hull(pts)) == want, name
    assert box == ec.host_box(mask), name
    mine_pts, mine_box = edit_inputs.extent_points(ext)                  # the module's own host half, on the reference's extents
    assert blob_edit.fit_ellipse(blob_edit.convex_hull(mine_pts)) == want and mine_box == box, name
    x, y, w, h = box
    image = ec.random_image(*mask.shape)
    region = blob_edit.object_region_from_mask(mask, image)            # the box IS what the host function cuts out and centres
    H, W = mask.shape
    sy, sx = (H - h) // 2, (W - w) // 2
    assert np.array_equal(region[sy:sy + h, sx:sx + w], np.where(mask[y:y + h, x:x + w, None], image[y:y + h, x:x + w], 255)), name


def test_the_extents_route_gives_ellipse_from_mask_on_synthetic_masks():
    for name, mask in ec.synthetic_object_masks().items():
        check_route(name, mask)
    assert edit_inputs.extent_points(np.full((5, 2), -1, np.int32))[1] is None


def test_the_extents_route_gives_ellipse_from_mask_on_the_demo_masks():
    masks = ec.demo_masks()
    assert len(masks) >= 8
    for name, mask in masks.items():
        check_route(name, mask)


def test_no_generic_test_ellipse_decides_a_pixel_on_a_tie():
    """The cover test's INPUT condition: fp64 arithmetic that is the host's, operation for operation, gives the host's mask whatever the
    margins are - but a test whose pixels all sit far from a tie says so without leaning on it.  The tie cases are exempt: they are there
    to sit ON the boundary, in arithmetic that is exact."""
    assert ec.decision_margin(ec.MOVE_HAT_512, 512, 512) > 1e-9
    assert ec.generic_ellipses(37, 45)["rotated"] == ((20.3, 17.9), (9.7, 23.1), 33.3)
    for H, W in ec.FRAMES:
        for name, e in ec.generic_ellipses(H, W).items():
            assert ec.decision_margin(e, H, W) > 1e-9, (H, W, name, ec.decision_margin(e, H, W))
    for H, W in [(64, 96)]:                                               # the batch test's frame and ellipses
        for e in ec.BATCH_ELLIPSES:
            assert ec.decision_margin(e, H, W) > 1e-9
    # what the cases are for
    H, W = 37, 45
    g = {k: blob_edit.ellipse_mask(e, H, W) for k, e in ec.generic_ellipses(H, W).items()}
    assert g["covers_frame"].all() and not g["misses_frame"].any() and 0 < (g["rotated"] > 0).sum() < H * W
    assert 0 < (g["centre_outside"] > 0).sum() < H * W
    assert (blob_edit.ellipse_mask(ec.app_dot(H, W), H, W) > 0).sum() in (1, 2, 4)
    t = ec.tie_ellipses(64, 64)
    assert ec.decision_margin(t["circle_r2"], 64, 64) == 0.0 and ec.decision_margin(t["axis_aligned"], 64, 64) == 0.0

