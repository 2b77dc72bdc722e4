"""Connected components and small-region removal without a GPU: the numpy checker of tests/mask_regions_common.py against scipy, the binding
table of include/blobctrl_masks.h, and what the new arguments refuse before anything reaches the device."""
import os

import numpy as np
import pytest
import torch

from blobctrl_amd import _lib, blob_edit, masks, sam
from tests import mask_regions_common as mc
from tests import sam_common as sc

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("bc_mask_label", "bc_mask_remove_small", "bc_mask_remove_small_phase")


def canonical_from_scipy(m):
    ndi = pytest.importorskip("scipy.ndimage")
    lab, n = ndi.label(m, structure=np.ones((3, 3)))
    out = np.full(m.shape, -1, dtype=np.int32)
    idx = np.arange(m.size).reshape(m.shape)
    for k in range(1, n + 1):
        out[lab == k] = idx[lab == k].min()
    return out, n


@pytest.mark.parametrize("size", [(37, 53), (150, 200), (3, 1030), (1, 1), (64, 1)])
def test_the_checker_equals_scipy(size):
    H, W = size
    counts = {}
    for name, make in mc.PATTERNS.items():
        m = make(H, W)
        for fg in (True, False):
            want, n = canonical_from_scipy(m == fg)
            got = mc.label(m, fg)
            assert got.dtype == np.int32 and np.array_equal(got, want), (name, fg)
            counts[name, fg] = n
    if size == (150, 200):
        # what the patterns are for: many components of both colours in the noise, one long chain, components that meet at corners only
        assert counts["noise35", True] > 500 and counts["noise62", False] > 300 and counts["noise50", True] > 20 and counts["noise50", False] > 20
        assert counts["serpentine", True] == 1 and counts["serpentine", False] == 75
        assert counts["checkerboard", True] == counts["checkerboard", False] == 1
        assert counts["diagonal", True] == 1 and counts["comb", True] == 1 and counts["comb", False] == 100
        assert counts["empty", True] == 0 and counts["full", False] == 0 and counts["last_pixel", True] == 1


def test_the_checkers_removal_on_hand_made_masks():
    m = np.zeros((12, 16), dtype=bool)
    m[1:5, 1:5] = True                                   # 16 pixels ...
    m[2, 2] = False                                      # ... with a pinhole
    m[8, 10] = m[9, 11] = True                           # a diagonal 2-pixel speck
    out, changed = mc.remove_small_regions(m, 2, "holes")
    assert changed and out[2, 2] and out.sum() == m.sum() + 1
    out, changed = mc.remove_small_regions(m, 1, "holes")
    assert not changed and np.array_equal(out, m)
    out, changed = mc.remove_small_regions(m, 3, "islands")
    assert changed and not out[8, 10] and not out[9, 11] and out.sum() == 15
    out, changed = mc.remove_small_regions(m, 2, "islands")                              # strict comparison: a speck of exactly 2 stays
    assert not changed and np.array_equal(out, m)
    out, changed = mc.remove_small_regions(m, 100, "islands")                            # all small: the largest stays
    assert changed and out.sum() == 15 and out[1, 1]
    two = np.zeros((5, 9), dtype=bool)
    two[1, 1] = two[1, 2] = two[3, 6] = two[3, 7] = True                                 # two equal largest: the first in raster order
    out, changed = mc.remove_small_regions(two, 100, "islands")
    assert changed and out.sum() == 2 and out[1, 1] and out[1, 2]
    assert mc.stats_of(out) == [2, 1, 1, 2, 1] and mc.stats_of(np.zeros((3, 3), bool)) == [0, 0, 0, 0, 0]


def test_binding_table_of_the_mask_entry_points():
    lib = _lib.load()
    header = open(os.path.join(HERE, "..", "include", "blobctrl_masks.h")).read()
    assert set(_lib.MASK_SIGNATURES) == set(NAMES)
    entry = open(os.path.join(HERE, "..", "__graft_entry__.py")).read()                 # built from its own source, with its header a dependency
    assert '"blobctrl_masks.h"' in entry and '"mask_regions.hip"' in entry
    for name in NAMES:
        assert getattr(lib, name) is not None and f"int {name}(" in header
        for table in (_lib.OPS, _lib.REQUEST_OPS, _lib.SAM_OPS, _lib.SAM_BATCH_OPS, _lib.EXPORTED_SYMBOLS, _lib.SAM_SIGNATURES,
                      _lib.SAM_BATCH_SIGNATURES):
            assert name not in table
        with pytest.raises(KeyError):
            _lib.op_code(name)
    assert f"#define BC_MASK_REGION_PHASES {_lib.MASK_REGION_PHASES}" in header and (_lib.MASK_HOLES, _lib.MASK_ISLANDS) == (0, 1)
    assert "BC_OP_COUNT = 53" in open(os.path.join(HERE, "..", "include", "blobctrl_hip.h")).read()


def test_bad_arguments_are_refused_before_anything_is_launched():
    lib = _lib.load()
    p = 4096
    for args in ((None, 1, 8, 8, 1, p), (p, 1, 8, 8, 1, None), (p, 0, 8, 8, 1, p), (p, 1, 0, 8, 1, p), (p, 1, 8, -1, 1, p)):
        assert lib.bc_mask_label(*args, None) == 1 and b"bc_mask_label" in lib.bc_last_error(), args
    assert lib.bc_mask_label(p, 1, 65536, 32768, 1, p, None) == 1 and b"2^31" in lib.bc_last_error()
    good = [p, 1, 8, 8, 4, 1, p, p, p]
    for at, bad in ((0, None), (6, None), (7, None), (8, None), (1, 0), (2, 0), (3, 0), (4, -1), (5, 2), (5, -1)):
        args = list(good)
        args[at] = bad
        assert lib.bc_mask_remove_small(*args, None) == 1 and b"bc_mask_remove_small" in lib.bc_last_error(), (at, bad)
        assert lib.bc_mask_remove_small_phase(*args, 0, None) == 1
    assert lib.bc_mask_remove_small(p, 1, 32768, 65536, 4, 1, p, p, p, None) == 1 and b"2^31" in lib.bc_last_error()
    assert lib.bc_mask_remove_small_phase(*good, _lib.MASK_REGION_PHASES, None) == 1 and b"phase" in lib.bc_last_error()
    assert lib.bc_mask_remove_small_phase(*good, -1, None) == 1


def test_the_python_surface_refuses_without_a_gpu():
    m = np.zeros((6, 7), dtype=bool)
    with pytest.raises(ValueError, match="mode"):
        masks.remove_small_regions(m, 3, "specks")
    with pytest.raises(ValueError, match="mode"):
        masks.remove_small_regions(torch.zeros(1, 6, 7, dtype=torch.bool), 3, "both")
    out, changed = masks.remove_small_regions(m, 0, "islands")             # area_thresh <= 0: the input, unchanged
    assert out is m and changed is False
    for call in (lambda: masks.label_components(torch.zeros(2, 6, 7, dtype=torch.bool)),
                 lambda: masks.remove_small_regions(torch.zeros(2, 6, 7, dtype=torch.uint8), 3, "holes"),
                 lambda: masks.clean_masks(torch.zeros(2, 6, 7, dtype=torch.bool), 3)):
        with pytest.raises(_lib.BlobCtrlHipError, match="no CPU fallback"):
            call()
    assert masks.SCRATCH_BUDGET_BYTES == 256 << 20                         # two int32 words per pixel: 32 masks of 1024 x 1024 per group
    assert masks._group(64, 1024, 1024) == 32 and masks._group(3, 4096, 4096) == 2 and masks._group(1, 30000, 30000) == 1


def tiny_generator(**kw):
    cfg = sam.SamConfig(num_heads=2, window_size=5, global_attn_indexes=(1,), decoder_heads=2)
    return sam.SamAutomaticMaskGenerator(sam.SamModel(sc.weights_of(sc.TINY_B), cfg, device="cpu"), **kw)


def test_generate_and_the_constructor_refuse():
    with pytest.raises(NotImplementedError, match="min_mask_region_area"):
        tiny_generator(min_mask_region_area=10)
    gen = tiny_generator(points_per_side=2)
    image = np.zeros((20, 30, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="min_mask_region_area"):
        gen.generate(image, min_mask_region_area=-1)
    with pytest.raises(ValueError):
        gen.postprocess_small_regions([], -1, 0.7)
    assert gen.postprocess_small_regions([], 5, 0.7) == []
    ann = {"segmentation": np.ones((4, 4), bool), "area": 16, "bbox": [0, 0, 3, 3]}
    same = gen.postprocess_small_regions([ann], 0, 0.7)                    # min_area 0: copies, nothing to run
    assert same == [ann] and same[0] is not ann
    with pytest.raises(_lib.BlobCtrlHipError):                            # the step itself needs the GPU
        gen.postprocess_small_regions([ann], 3, 0.7)


def test_ellipses_from_image_keeps_the_one_argument_call():
    yy, xx = np.mgrid[:60, :80]
    disc = ((xx - 40) / 20.0) ** 2 + ((yy - 30) / 12.0) ** 2 <= 1
    ann = {"segmentation": disc, "area": int(disc.sum())}

    class Old:                                             # the call surface from before the argument existed
        calls = 0

        def generate(self, image):
            self.calls += 1
            return [ann]

    class New:
        seen = None

        def generate(self, image, min_mask_region_area=0):
            self.seen = min_mask_region_area
            return [ann]

    old, new = Old(), New()
    image = np.zeros((60, 80, 3), dtype=np.uint8)
    got = blob_edit.ellipses_from_image(old, image)
    assert old.calls == 1 and len(got) == 1 and got[0][1] is ann
    assert blob_edit.ellipses_from_image(old, image, min_area=5, min_region_area=0)[0][0] == got[0][0]
    with pytest.raises(TypeError):
        blob_edit.ellipses_from_image(old, image, min_region_area=8)
    assert blob_edit.ellipses_from_image(new, image, min_region_area=8)[0][0] == got[0][0] and new.seen == 8
    with pytest.raises(ValueError):
        blob_edit.ellipses_from_image(new, image, min_region_area=-1)
    with pytest.raises(ValueError):
        blob_edit.ellipse_from_click(None, None, [[1, 2]], min_region_area=-1)
