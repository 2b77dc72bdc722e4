"""Host side of batched SAM prompts and SamAutomaticMaskGenerator (blobctrl_amd/sam.py): the restatement of tests/sam_common.py, run prompt
by prompt, reproduces what transformers' SamModel wrote for ONE batched call of 16 prompts (tests/golden/sam_amg.npz); box NMS on hand-made
boxes; ResizeLongestSide and the point grid; the refusals and the ABI tables of the two new entry points."""
import os

import numpy as np
import pytest
import torch

from blobctrl_amd import _lib, blob_edit, sam
from tests import sam_common as sc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "sam_amg.npz")
TINY = os.path.join(HERE, "golden", "sam_tiny.npz")


@pytest.fixture(scope="module")
def amg():
    return dict(np.load(GOLD))


def test_restatement_prompt_by_prompt_matches_the_batched_reference(amg):
    sd = sc.weights_of(sc.TINY_A)
    emb = torch.from_numpy(np.load(TINY)["a_emb"])[0]
    stored = {int(p): k for k, p in enumerate(amg["stored"])}
    assert sorted(stored) == [0, 5, 10, 15] and amg["iou"].shape == (16, 3) and amg["low"].shape == (4, 3, 64, 64)
    ious = []
    with torch.no_grad():
        for p in range(16):
            low, iou = sc.mask_decoder(sd, emb, [amg["points"][p].tolist()], [1], sc.TINY_A["image"])
            ious.append(iou[1:])
            if p in stored:
                assert sc.rel_err(low[1:], amg["low"][stored[p]]) < 1e-5, p
    assert sc.rel_err(torch.stack(ious), amg["iou"]) < 1e-5


def test_fixture_thresholds_filter_the_reference(amg):
    """The fixture's thresholds sit inside the reference's own values: both filters drop masks and keep masks."""
    iou, stab = amg["iou"].reshape(-1), amg["stability"]
    k1 = iou > amg["pred_iou_thresh"]
    k2 = k1 & (stab >= amg["stability_score_thresh"])
    assert 48 > k1.sum() > k2.sum() >= len(amg["ref_kept"]) >= 2
    assert float(amg["offset"]) == np.float32(0.05) and 0.0 < float(amg["box_nms_thresh"]) <= 1.0
    assert amg["boxes"].shape == (48, 4) and amg["areas"].shape == (48,) and (amg["areas"] > 0).all()
    assert len(amg["ref_kept"]) == k2.sum() - int(amg["nms_dropped"])


def test_box_nms_on_hand_made_boxes():
    # nested: the inner box (IoU 0.64 with the outer) goes at 0.5 and stays at 0.7
    nested = [[0, 0, 10, 10], [1, 1, 9, 9]]
    assert sam.box_nms(nested, [0.9, 0.8], 0.5).tolist() == [0] and sam.box_nms(nested, [0.9, 0.8], 0.7).tolist() == [0, 1]
    assert sam.box_nms(nested, [0.8, 0.9], 0.5).tolist() == [1]                       # the better score wins, whichever box it is
    # disjoint boxes never suppress each other; the result is in descending score
    assert sam.box_nms([[0, 0, 5, 5], [10, 10, 20, 20], [30, 0, 40, 5]], [0.1, 0.3, 0.2], 0.0).tolist() == [1, 2, 0]
    # IoU exactly at the threshold is kept: [0,0,10,10] and [0,0,10,5] have IoU 50 / 100
    half = [[0, 0, 10, 10], [0, 0, 10, 5]]
    assert sam.box_nms(half, [0.9, 0.8], 0.5).tolist() == [0, 1] and sam.box_nms(half, [0.9, 0.8], 0.4999).tolist() == [0]
    # area without + 1: touching boxes have no intersection
    assert sam.box_nms([[0, 0, 5, 5], [5, 0, 10, 5]], [1.0, 0.5], 0.0).tolist() == [0, 1]
    # two zero-area boxes: 0 / 0 is NaN, and NaN never suppresses
    assert sam.box_nms([[5, 5, 5, 5], [5, 5, 5, 5], [0, 0, 10, 10]], [0.9, 0.8, 0.7], 0.0).tolist() == [0, 1, 2]
    # equal scores: the lower index first, and it suppresses the higher one
    same = [[0, 0, 10, 10], [0, 0, 10, 10], [20, 20, 30, 30]]
    assert sam.box_nms(same, [0.5, 0.5, 0.5], 0.5).tolist() == [0, 2]
    # a suppressed box suppresses nothing: 1 goes by 0 (IoU 0.43), so 2 (IoU 0.6 with 1, 0.21 with 0) stays
    chain = [[0, 0, 10, 10], [4, 0, 14, 10], [6.5, 0, 16.5, 10]]
    assert sam.box_nms(chain, [0.9, 0.8, 0.7], 0.4).tolist() == [0, 2]
    assert sam.box_nms(np.zeros((0, 4)), [], 0.5).tolist() == []
    with pytest.raises(ValueError):
        sam.box_nms(nested, [0.5], 0.5)


def test_resize_longest_side_agrees_with_scale_points():
    t = sam.ResizeLongestSide(1024)
    assert t.get_preprocess_shape(200, 150, 1024) == sam.preprocess_shape(200, 150, 1024) == (1024, 768)
    assert t.get_preprocess_shape(1365, 2048, 1024) == (683, 1024)
    rng = np.random.Generator(np.random.PCG64(5))
    for size in ((150, 200), (200, 150), (1365, 2048), (33, 1024)):
        c = rng.uniform(0, 1, (3, 4, 2)) * [size[1], size[0]]
        want = sam.scale_points(c.reshape(-1, 2), size, 1024).reshape(3, 4, 2)
        got = t.apply_coords(c, size)
        assert got.dtype == np.float32 and got.shape == (3, 4, 2) and np.array_equal(got, want)
        got_t = t.apply_coords_torch(torch.from_numpy(c), size)
        assert got_t.dtype == torch.float32 and np.array_equal(got_t.numpy(), want)
    assert np.array_equal(sam.ResizeLongestSide(256).apply_coords(np.array([[100.0, 75.0]]), (150, 200)), np.array([[128.0, 96.0]], np.float32))
    model = sam.SamModel(sc.weights_of(sc.TINY_B), sam.SamConfig(num_heads=2, window_size=5, global_attn_indexes=(1,), decoder_heads=2), device="cpu")
    assert isinstance(sam.SamPredictor(model).transform, sam.ResizeLongestSide) and sam.SamPredictor(model).transform.target_length == 192


def test_point_grid_order(amg):
    g2 = sam.build_point_grid(2)
    assert g2.tolist() == [[0.25, 0.25], [0.75, 0.25], [0.25, 0.75], [0.75, 0.75]]          # x fastest, offset 1 / (2 n)
    H, W = sc.ORIGINAL_SIZE
    grid = sam.build_point_grid(4) * np.array([[W, H]], dtype=np.float64)
    assert np.array_equal(grid, amg["grid"])
    assert np.array_equal(sam.ResizeLongestSide(sc.TINY_A["image"]).apply_coords(grid, sc.ORIGINAL_SIZE), amg["points"])
    model = sam.SamModel(sc.weights_of(sc.TINY_B), sam.SamConfig(num_heads=2, window_size=5, global_attn_indexes=(1,), decoder_heads=2), device="cpu")
    gen = sam.SamAutomaticMaskGenerator(model, points_per_side=4)
    assert np.array_equal(gen.point_grids[0], sam.build_point_grid(4)) and gen.points_per_batch == 64
    assert (gen.pred_iou_thresh, gen.stability_score_thresh, gen.stability_score_offset, gen.box_nms_thresh) == (0.88, 0.95, 1.0, 0.7)
    assert np.array_equal(sam.SamAutomaticMaskGenerator(model).point_grids[0], sam.build_point_grid(32))


def test_refusals():
    cfg = sam.SamConfig(num_heads=2, window_size=5, global_attn_indexes=(1,), decoder_heads=2)
    model = sam.SamModel(sc.weights_of(sc.TINY_B), cfg, device="cpu")
    with pytest.raises(NotImplementedError, match="crop_n_layers"):
        sam.SamAutomaticMaskGenerator(model, crop_n_layers=1)
    with pytest.raises(NotImplementedError, match="min_mask_region_area"):
        sam.SamAutomaticMaskGenerator(model, min_mask_region_area=10)
    for mode in ("uncompressed_rle", "coco_rle"):
        with pytest.raises(NotImplementedError, match="output_mode"):
            sam.SamAutomaticMaskGenerator(model, output_mode=mode)
    with pytest.raises(ValueError):
        sam.SamAutomaticMaskGenerator(model, points_per_side=None)
    pred = sam.SamPredictor(model)
    pts, labs = torch.zeros(2, 1, 2), torch.ones(2, 1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="set_image"):
        pred.predict_torch(pts, labs)
    pred.is_image_set, pred.original_size, pred.input_size = True, (150, 200), (144, 192)
    with pytest.raises(NotImplementedError, match="box"):
        pred.predict_torch(pts, labs, boxes=torch.zeros(2, 4))
    with pytest.raises(NotImplementedError, match="mask_input"):
        pred.predict_torch(pts, labs, mask_input=torch.zeros(2, 1, 48, 48))
    with pytest.raises(ValueError):
        pred.predict_torch(None, None)
    with pytest.raises(RuntimeError, match="another SamPredictor"):
        pred.predict_torch(pts, labs)
    model._emb_owner = id(pred)
    with pytest.raises(_lib.BlobCtrlHipError):                  # running needs the GPU: there is no CPU fallback
        pred.predict_torch(pts, labs)
    with pytest.raises(ValueError):
        model.decode_batch(torch.zeros(2, 2), torch.ones(2, 1))
    with pytest.raises(ValueError):
        model.decode_batch(torch.zeros(2, 1, 2), torch.ones(2, 2))


def test_abi_tables_of_the_new_entry_points(tmp_path):
    lib = _lib.load()
    header = open(os.path.join(HERE, "..", "include", "blobctrl_sam.h")).read()
    assert set(_lib.SAM_BATCH_OPS) == set(_lib.SAM_BATCH_SIGNATURES) == {"bc_sam_tokens_batch", "bc_mask_stats"}
    others = set(_lib.OPS) | set(_lib.REQUEST_OPS) | set(_lib.SAM_OPS)
    codes = set(_lib.OPS.values()) | set(_lib.REQUEST_OPS.values()) | set(_lib.SAM_OPS.values()) | {_lib.OP_SIGNAL, _lib.OP_WAIT}
    assert not set(_lib.SAM_BATCH_OPS) & others and not set(_lib.SAM_BATCH_OPS.values()) & codes
    assert sorted(_lib.SAM_BATCH_OPS.values()) == [51, 52] and "BC_OP_COUNT = 53" in open(os.path.join(HERE, "..", "include", "blobctrl_hip.h")).read()
    assert not set(_lib.SAM_BATCH_SIGNATURES) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.SAM_SIGNATURES))
    for name in list(_lib.SAM_BATCH_OPS) + ["bc_mask_stats_chunks"]:
        assert getattr(lib, name) is not None and f"int {name}(" in header
    for name, code in _lib.SAM_BATCH_OPS.items():
        assert _lib.op_code(name) == code
    assert _lib.op_signature("bc_sam_tokens_batch") == "pippiipippfp" and _lib.op_signature("bc_mask_stats") == "piiiffpp"
    assert _lib.op_code("bc_sam_tokens") == 49 and _lib.op_signature("bc_sam_masks") == "pipiiiiip"         # the older tables still resolve
    with pytest.raises(KeyError):
        _lib.op_code("bc_no_such_entry_point")
    # bad arguments are refused before anything is launched
    p = 4096
    assert lib.bc_sam_tokens_batch(p, 5, p, p, 0, 1, p, 16, p, p, 256.0, p, None) == 1 and b"bc_sam_tokens_batch" in lib.bc_last_error()
    assert lib.bc_sam_tokens_batch(p, 5, p, None, 2, 1, p, 16, p, p, 256.0, p, None) == 1
    assert lib.bc_sam_tokens_batch(p, 5, p, p, 2, 0, p, 16, p, p, 256.0, p, None) == 1
    assert lib.bc_sam_tokens_batch(p, 5, p, p, 2, 1, p, 16, p, p, 0.0, p, None) == 1
    assert lib.bc_mask_stats(p, 0, 8, 8, 0.0, 1.0, p, p, None) == 1 and b"bc_mask_stats" in lib.bc_last_error()
    assert lib.bc_mask_stats(p, 1, 8, 0, 0.0, 1.0, p, p, None) == 1 and lib.bc_mask_stats(p, 1, 8, 8, 0.0, 1.0, None, p, None) == 1
    assert lib.bc_mask_stats(p, 1, 8, 8, 0.0, -1.0, p, p, None) == 1 and b"offset" in lib.bc_last_error()
    assert lib.bc_mask_stats(p, 1, 8, 8, float("nan"), 1.0, p, p, None) == 1
    assert lib.bc_mask_stats(p, 1, 65536, 65536, 0.0, 1.0, p, p, None) == 1 and b"2^31" in lib.bc_last_error()
    assert lib.bc_mask_stats_chunks(1024, 1024) == 64 and lib.bc_mask_stats_chunks(37, 53) == 1 and lib.bc_mask_stats_chunks(129, 128) == 2
    assert lib.bc_mask_stats_chunks(0, 5) == -1 and lib.bc_mask_stats_chunks(65536, 65536) == -1
    # recordable, and in-process only like the other SAM launches
    from blobctrl_amd.launch import Recorder
    for name, args in (("bc_sam_tokens_batch", None), ("bc_mask_stats", None)):
        rec = Recorder(torch.device("cpu"))
        rec.begin("seg")
        buf = torch.zeros(64, dtype=torch.float32)
        if name == "bc_mask_stats":
            rec.call(name, buf, 1, 8, 8, 0.0, 1.0, buf, buf, kind="mask_stats", keep=buf)
        else:
            rec.call(name, buf, 5, buf, buf, 2, 1, buf, 16, buf, buf, 256.0, buf, kind="sam_tokens", keep=buf)
        with pytest.raises(_lib.BlobCtrlHipError, match="in-process only"):
            rec.save(str(tmp_path / (name + ".bcplan")))
        assert not os.path.exists(str(tmp_path / (name + ".bcplan")))
        rec.close()


class _FixtureGenerator:
    def __init__(self, anns):
        self.anns, self.calls = anns, []

    def generate(self, image):
        self.calls.append(image.shape)
        return list(self.anns)


def test_ellipses_from_image_sorts_by_area():
    yy, xx = np.mgrid[0:60, 0:80]
    small = (xx - 20) ** 2 + (yy - 20) ** 2 < 36
    big = ((xx - 50) / 20.0) ** 2 + ((yy - 30) / 12.0) ** 2 < 1
    tiny = (xx == 3) & (yy == 4)
    anns = [{"segmentation": m, "area": int(m.sum())} for m in (small, big, tiny)]
    gen = _FixtureGenerator(anns)
    got = blob_edit.ellipses_from_image(gen, np.zeros((60, 80, 3), np.uint8), min_area=2)
    assert gen.calls == [(60, 80, 3)] and [a is b for (_, a), b in zip(got, (anns[1], anns[0]))] == [True, True] and len(got) == 2
    assert got[0][0] == blob_edit.ellipse_from_mask(big.astype(np.uint8)) and got[1][0] == blob_edit.ellipse_from_mask(small.astype(np.uint8))
    # a single pixel has no ellipse (fit_ellipse needs five hull points): it is left out, not an error
    assert [a for _, a in blob_edit.ellipses_from_image(gen, np.zeros((60, 80, 3), np.uint8))] == [anns[1], anns[0]]


def test_ellipses_from_image_equals_ellipse_from_mask_on_ragged_masks():
    """The blobs come from the row extremes of a mask, not from all its pixels: the same hull, hence the same ellipse, bit for bit."""
    rng = np.random.Generator(np.random.PCG64(17))
    yy, xx = np.mgrid[0:90, 0:120]
    masks = []
    for k in range(6):
        cx, cy, a, b = rng.uniform(30, 90), rng.uniform(25, 65), rng.uniform(8, 40), rng.uniform(6, 25)
        th = rng.uniform(0, np.pi)
        u, v = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th), -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        m = ((u / a) ** 2 + (v / b) ** 2 < 1) & (rng.uniform(0, 1, xx.shape) < 0.7)          # holes and a ragged rim
        m[int(cy) % 90, :5] = k % 2 == 0                                                     # a detached stroke at the frame's edge
        masks.append(m)
    anns = [{"segmentation": m, "area": int(m.sum())} for m in masks]
    got = blob_edit.ellipses_from_image(_FixtureGenerator(anns), np.zeros((90, 120, 3), np.uint8))
    assert len(got) == len(anns)
    for e, a in got:
        assert e == blob_edit.ellipse_from_mask(a["segmentation"].astype(np.uint8))
