"""Connected components and small-region removal on the GPU (include/blobctrl_masks.h, blobctrl_amd/masks.py) and what is wired to them:
`SamAutomaticMaskGenerator.generate(image, min_mask_region_area=)`, `postprocess_small_regions`, and blob_edit's `min_region_area`.
Everything is a decision on integers, so every comparison against the numpy checker (tests/mask_regions_common.py) is `==`."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from blobctrl_amd import _lib, blob_edit, masks, sam  # noqa: E402
from tests import mask_regions_common as mc  # noqa: E402
from tests import sam_common as sc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
LABEL_SIZES = mc.SIZES                                  # (the tile is 32 x 64: every size but the 1 x 1 straddles it, or misses it, some way)
REMOVAL_SIZES = [(37, 53), (150, 200), (3, 1030), (1030, 3)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("name", list(mc.PATTERNS))
@pytest.mark.parametrize("size", LABEL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labels_equal_the_checker(size, name):
    m = mc.PATTERNS[name](*size)
    for fg in (True, False):
        got = masks.label_components(dev(m), foreground=fg)
        assert got.dtype == torch.int32 and tuple(got.shape) == size
        assert np.array_equal(got.cpu().numpy(), mc.label(m, fg)), (name, size, fg)
    as_bytes = masks.label_components(dev(m.astype(np.uint8) * 255)[None])              # uint8 with values other than 1, and a batch axis
    assert np.array_equal(as_bytes[0].cpu().numpy(), mc.label(m, True))


@pytest.mark.parametrize("size", [(37, 53), (150, 200), (3, 1030), (1030, 3), (1, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_batch_labels_every_mask_as_if_alone(size):
    H, W = size
    batch = mc.batch_of_three(H, W)
    assert batch[0, -1, -1] and batch[1, 0, 0]
    for fg in (True, False):
        got = masks.label_components(dev(batch), foreground=fg)
        again = masks.label_components(dev(batch), foreground=fg)
        assert torch.equal(got, again)                                                   # two runs: identical bytes
        for k in range(3):
            alone = masks.label_components(dev(batch[k]), foreground=fg)
            assert torch.equal(got[k], alone) and np.array_equal(alone.cpu().numpy(), mc.label(batch[k], fg)), (k, fg)
        # the same batch behind a base address offset by one byte
        buf = torch.zeros(batch.size + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = dev(batch.astype(np.uint8)).flatten()
        odd = buf[1:].view(3, H, W)
        assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
        assert torch.equal(masks.label_components(odd, foreground=fg), got)


def test_offsets_past_2_to_the_31_bytes_of_labels():
    """513 masks of 1024 x 1024: the last mask's labels start 2^31 bytes into the array.  Only the last mask has set pixels - a diagonal from
    corner to corner, one component - so the expected labels are known without running the checker on half a gigapixel."""
    n, S = 513, 1024
    m = torch.zeros(n, S, S, dtype=torch.bool, device="cuda")
    d = torch.arange(S, device="cuda")
    m[-1, d, d] = True
    m[0, 5, 7] = True
    lab = masks.label_components(m)
    assert int((lab[-1] >= 0).sum()) == S and bool((lab[-1, d, d] == 0).all())
    assert int(lab[0, 5, 7]) == 5 * S + 7 and int((lab[:-1] >= 0).sum()) == 1
    del lab
    bg = masks.label_components(m[-2:], foreground=False)
    assert int(bg[0].max()) == 0 and int(bg[0].min()) == 0                              # an empty mask: one background component, root 0
    assert torch.unique(bg[1]).tolist() == [-1, 1]                                      # 8-connectivity crosses the diagonal: one component


# ------------------------------------------------------------------------------------------------------------------ removal
def run_remove(batch, thresh, mode):
    """bc_mask_remove_small through masks.remove_small_regions AND directly (for `out`): (masks bool [n][H][W], out int32 [n][6])."""
    lib = _lib.load()
    work = dev(batch.astype(np.uint8))
    n, H, W = work.shape
    scratch = torch.full((2, n, H, W), -7, dtype=torch.int32, device="cuda")            # not zeroed: the entry point must not rely on it
    out = torch.full((n, 6), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.bc_mask_remove_small(work.data_ptr(), n, H, W, thresh, masks.MODES[mode],
                                        scratch[0].data_ptr(), scratch[1].data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "bc_mask_remove_small")
    src = dev(batch)
    res, changed = masks.remove_small_regions(src, thresh, mode)
    assert torch.equal(src, dev(batch)), "the input was modified"
    assert res.dtype == torch.bool and changed.dtype == torch.bool and torch.equal(res, work.bool())
    assert torch.equal(changed, out[:, 0] != 0)
    return res.cpu().numpy(), out.cpu().numpy()


def check_remove(batch, thresh, mode):
    got, out = run_remove(batch, thresh, mode)
    flips = 0
    for k, m in enumerate(batch):
        want, changed = mc.remove_small_regions(m, thresh, mode)
        assert np.array_equal(got[k], want), (k, thresh, mode)
        assert out[k].tolist() == [int(changed)] + mc.stats_of(got[k]), (k, thresh, mode)
        flips += int((want != m).sum())
    return got, out, flips


@pytest.mark.parametrize("mode", ["holes", "islands"])
@pytest.mark.parametrize("thresh", [4, 12])
@pytest.mark.parametrize("size", REMOVAL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_removal_on_noise_equals_the_checker(size, thresh, mode):
    batch = np.stack([mc.noise(*size, p) for p in mc.DENSITIES])
    _, out, flips = check_remove(batch, thresh, mode)
    if size == (150, 200):
        assert flips > 100 and out[:, 0].all() and (out[:, 1] > 5000).all()              # both modes do real work, most of every mask survives


def test_removal_edge_cases():
    H, W = 40, 70                                          # four tiles
    # a component of exactly the threshold stays, one pixel fewer goes (both colours; the 16-pixel square straddles a tile corner)
    m = np.zeros((H, W), dtype=bool)
    m[10:15, 20:28] = True                                 # 40
    m[30:34, 62:66] = True                                 # 16
    m[2, 2:17] = True                                      # 15
    got, out, _ = check_remove(m[None], 16, "islands")
    assert got[0].sum() == 56 and got[0, 30:34, 62:66].all() and not got[0, 2].any() and out[0].tolist() == [1, 56, 20, 10, 65, 33]
    got, out, _ = check_remove(m[None], 15, "islands")
    assert np.array_equal(got[0], m) and out[0].tolist() == [0, 71, 2, 2, 65, 33]
    inv = ~m
    got, out, _ = check_remove(inv[None], 16, "holes")
    assert (~got[0]).sum() == 56 and got[0, 2].all() and not got[0, 30:34, 62:66].any() and out[0, :2].tolist() == [1, H * W - 56]
    got, out, _ = check_remove(inv[None], 15, "holes")
    assert np.array_equal(got[0], inv) and out[0, 0] == 0
    # specks only: the largest stays; two equal largest: the first in raster order
    s = np.zeros((H, W), dtype=bool)
    s[3, 60] = s[10, 5] = s[10, 6] = s[10, 7] = s[35, 66] = s[36, 67] = True
    got, out, _ = check_remove(s[None], 50, "islands")
    assert got[0].sum() == 3 and got[0, 10, 5:8].all() and out[0].tolist() == [1, 3, 5, 10, 7, 10]
    t = np.zeros((H, W), dtype=bool)
    t[33, 65] = t[33, 66] = t[5, 1] = t[6, 2] = t[20, 30] = True
    got, out, _ = check_remove(t[None], 50, "islands")
    assert got[0].sum() == 2 and got[0, 5, 1] and got[0, 6, 2]
    one = np.zeros((H, W), dtype=bool)
    one[39, 69] = True                                     # a lone speck stays, and counts as changed (the package's flag)
    got, out, _ = check_remove(one[None], 9, "islands")
    assert got[0].sum() == 1 and out[0].tolist() == [1, 1, 69, 39, 69, 39]
    # an empty mask is unchanged in both modes (a batch, so that rows of `out` do not mix), and a full one
    e = np.zeros((3, H, W), dtype=bool)
    e[1] = True
    for mode in ("holes", "islands"):
        got, out, _ = check_remove(e, 100, mode)          # (below H * W: the whole frame is no "small hole")
        assert got[0].sum() == 0 and out[0].tolist() == [0, 0, 0, 0, 0, 0] and got[1].all() and out[1].tolist() == [0, H * W, 0, 0, W - 1, H - 1]
    # the numpy form of the package, a 2-D tensor, and area_thresh <= 0
    res, changed = masks.remove_small_regions(s, 50, "islands")
    assert isinstance(res, np.ndarray) and res.dtype == np.bool_ and changed is True and res.sum() == 3
    res, changed = masks.remove_small_regions(dev(s), 50, "islands")
    assert res.shape == (H, W) and changed.ndim == 0 and bool(changed) and int(res.sum()) == 3
    src = dev(s[None])
    res, changed = masks.remove_small_regions(src, 0, "holes")
    assert res is src and not bool(changed.any())


def nested_square():
    c = np.zeros((24, 24), dtype=bool)
    c[5:18, 5:18] = True                                   # 13 x 13
    c[7:16, 7:16] = False                                  # a 9 x 9 hole ...
    c[9:14, 9:14] = True                                   # ... with a 5 x 5 core: the ring of background is 56 pixels, the core 25
    return c


def test_holes_are_filled_before_islands_are_removed():
    c = nested_square()
    assert (c[7:16, 7:16] == 0).sum() == 56 and c[9:14, 9:14].sum() == 25
    cleaned, changed, stats = masks.clean_masks(dev(c[None]), 60)
    want = np.zeros_like(c)
    want[5:18, 5:18] = True
    assert np.array_equal(cleaned[0].cpu().numpy(), want) and bool(changed[0]) and stats[0].tolist() == [169, 5, 5, 17, 17]
    assert stats.dtype == torch.int32 and cleaned.dtype == torch.bool
    assert np.array_equal(want, mc.clean(c, 60)[0])
    alone, ch = masks.remove_small_regions(dev(c[None]), 60, "islands")                  # islands alone: the core goes
    assert bool(ch[0]) and not alone[0, 9:14, 9:14].any() and int(alone[0].sum()) == 169 - 81
    assert np.array_equal(alone[0].cpu().numpy(), mc.remove_small_regions(c, 60, "islands")[0])


def test_clean_masks_in_groups_equals_one_group(monkeypatch):
    batch = np.stack([mc.noise(37, 53, p) for p in mc.DENSITIES] + [mc.serpentine(37, 53), mc.checkerboard(37, 53)])
    whole = masks.clean_masks(dev(batch), 6)
    monkeypatch.setattr(masks, "SCRATCH_BUDGET_BYTES", 2 * 8 * 37 * 53)                  # two masks per group: 2 + 2 + 1
    assert masks._group(5, 37, 53) == 2
    parts = masks.clean_masks(dev(batch), 6)
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)
    for k, m in enumerate(batch):
        want, changed = mc.clean(m, 6)
        assert np.array_equal(whole[0][k].cpu().numpy(), want) and bool(whole[1][k]) == changed
        assert whole[2][k].tolist() == mc.stats_of(want)


# ------------------------------------------------------------------------------------------------------------------ the generator's step
@functools.lru_cache(maxsize=None)
def tiny():
    return dict(np.load(os.path.join(HERE, "golden", "sam_tiny.npz")))


@functools.lru_cache(maxsize=None)
def amg():
    return dict(np.load(os.path.join(HERE, "golden", "sam_amg.npz")))


@functools.lru_cache(maxsize=None)
def model_a():
    cfg = sc.TINY_A
    return sam.SamModel(sc.weights_of(cfg), sam.SamConfig(num_heads=cfg["heads"], window_size=cfg["window"],
                                                          global_attn_indexes=cfg["global_attn_indexes"], decoder_heads=sc.DECODER_HEADS))


@functools.lru_cache(maxsize=None)
def fixture_generator():
    """tests/test_sam_amg_gpu.py::fixture_generator restated: fixture (a)'s frame is a stored tensor, so set_image runs the encoder on it."""
    z, model = amg(), model_a()
    gen = sam.SamAutomaticMaskGenerator(model, points_per_side=4, points_per_batch=5, pred_iou_thresh=float(z["pred_iou_thresh"]),
                                        stability_score_thresh=float(z["stability_score_thresh"]), stability_score_offset=float(z["offset"]),
                                        box_nms_thresh=float(z["box_nms_thresh"]))
    pred = gen.predictor

    def set_image(image, image_format="RGB"):
        assert tuple(np.asarray(image).shape) == sc.ORIGINAL_SIZE + (3,)
        pred.reset_image()
        pred.features = model.encode(torch.from_numpy(tiny()["a_pixels_q8"]).float() / 32)
        model._emb_owner = id(pred)
        pred.original_size, pred.input_size, pred.is_image_set = sc.ORIGINAL_SIZE, sc.INPUT_SIZE, True

    pred.set_image = set_image
    return gen


KEYS = {"segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box"}


def same_annotations(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y)
        assert x["segmentation"].dtype == np.bool_ and np.array_equal(x["segmentation"], y["segmentation"])
        for key in set(x) - {"segmentation"}:
            assert x[key] == y[key], key


def disc(H, W, cx, cy, r):
    yy, xx = np.mgrid[:H, :W]
    return (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r


def annotation(m, score):
    area, x0, y0, x1, y1 = mc.stats_of(m)
    return {"segmentation": m, "area": area, "bbox": [x0, y0, x1 - x0, y1 - y0], "predicted_iou": score, "point_coords": [[1.0, 2.0]],
            "stability_score": 0.5 + score / 4, "crop_box": [0, 0, m.shape[1], m.shape[0]]}


def test_postprocess_small_regions_on_painted_annotations():
    H, W = 96, 128
    clean_disc = disc(H, W, 40, 40, 18)
    specked = clean_disc.copy()
    specked[90, 120] = specked[91, 121] = True             # (ii): the disc plus a 2-pixel speck far away
    holed = disc(H, W, 95, 60, 15)
    holed[60, 95] = False                                  # (iii): another disc with a 1-pixel hole
    specks = np.zeros((H, W), dtype=bool)                  # (iv): five specks of 1 .. 5 pixels
    for k in range(5):
        specks[5 + 12 * k, 100:101 + k] = True
    anns = [annotation(clean_disc, 0.99), annotation(specked, 0.98), annotation(holed, 0.97), annotation(specks, 0.96)]
    gen = fixture_generator()
    got = gen.postprocess_small_regions(anns, 8, 0.7)
    same_annotations(got, mc.postprocess_small_regions(anns, 8, 0.7))
    # exactly: (i) untouched; (iii) with its hole filled; (iv) reduced to its 5-pixel speck; (ii) became a duplicate of (i) with score 0: dropped
    assert len(got) == 3 and [a["predicted_iou"] for a in got] == [0.99, 0.97, 0.96]
    assert np.array_equal(got[0]["segmentation"], clean_disc) and got[0]["area"] == anns[0]["area"] and got[0]["bbox"] == anns[0]["bbox"]
    assert got[1]["area"] == anns[2]["area"] + 1 and got[1]["bbox"] == anns[2]["bbox"] and got[1]["segmentation"][60, 95]
    assert got[2]["area"] == 5 and got[2]["bbox"] == [100, 53, 4, 0] and got[2]["segmentation"][53, 100:105].all()
    unchanged = [a for a in got if any(np.array_equal(a["segmentation"], b["segmentation"]) for b in anns)]
    changed_kept = [a for a in got if not any(np.array_equal(a["segmentation"], b["segmentation"]) for b in anns)]
    assert len(unchanged) >= 1 and len(changed_kept) >= 1 and len(got) < len(anns)       # one of each: untouched, changed and kept, dropped
    assert all(a["stability_score"] == b["stability_score"] for a, b in zip(got, [anns[0], anns[2], anns[3]]))
    assert np.array_equal(anns[1]["segmentation"], specked)                              # the input list and its arrays are as they were


def smallest_component(mask):
    """The smallest size among the components, of either colour, that are not the largest of their colour: the mask changes for every
    min_area above it.  None when each colour is one component."""
    sizes = [s for fg in (True, False) for s in sorted(mc.components(mask, fg)[1].tolist())[:-1]]
    return min(sizes) if sizes else None


def choose_min_area(anns):
    """A min_area from the masks' own components: one for which a CHANGED mask stands in front of an UNCHANGED one (the second NMS then
    reorders), if the masks allow one; else the smallest that changes any mask.  -> (min_area, whether the order must change)."""
    least = [smallest_component(a["segmentation"]) for a in anns]
    candidates = sorted({v + 1 for v in least if v is not None})
    assert candidates, "no mask has a second component of either colour: nothing for the step to do"
    for m in candidates:
        changed = [mc.clean(a["segmentation"], m)[1] for a in anns]
        if any(c and not all(changed[k:]) for k, c in enumerate(changed)):
            return m, True
    return candidates[0], False


def test_generate_with_min_mask_region_area_on_the_fixture():
    gen = fixture_generator()
    image = np.zeros(sc.ORIGINAL_SIZE + (3,), np.uint8)
    plain = gen.generate(image)
    plans = gen.predictor.model.plans_recorded
    m, reorders = choose_min_area(plain)
    thresh = max(gen.box_nms_thresh, gen.crop_nms_thresh)
    want = mc.postprocess_small_regions(plain, m, thresh)
    got = gen.generate(image, min_mask_region_area=m)
    assert gen.predictor.model.plans_recorded == plans, "generate with min_mask_region_area recorded a plan"
    assert "regions_ms" in gen.last_timing and gen.last_timing["regions_ms"] > 0.0
    same_annotations(got, want)
    assert all(set(a) == KEYS for a in got)
    by_point = {tuple(a["point_coords"][0]) + (a["predicted_iou"],): a for a in plain}
    changed = [a for a in got if not np.array_equal(a["segmentation"], by_point[tuple(a["point_coords"][0]) + (a["predicted_iou"],)]["segmentation"])]
    dropped = len(plain) - len(got)
    moved = [a["predicted_iou"] for a in got] != [a["predicted_iou"] for a in plain][:len(got)]
    print(f"min_mask_region_area {m}: {len(plain)} masks -> {len(got)} returned, {len(changed)} of them changed, {dropped} dropped; the order "
          f"{'changes' if moved else 'stays'} (the fixture {'has' if reorders else 'has no'} min_area with a changed mask in front of an unchanged one)")
    assert len(got) >= 1 and len(changed) + dropped >= 1   # at least one mask changes, at least one annotation is returned
    assert moved or not reorders                           # (the reordering itself is pinned by the painted test below, whatever the fixture allows)
    for a in got:
        area, x0, y0, x1, y1 = mc.stats_of(a["segmentation"])
        assert a["area"] == area == int(a["segmentation"].sum()) and a["bbox"] == [x0, y0, x1 - x0, y1 - y0]
    again = gen.generate(image)                            # and without the argument the call is what it was
    same_annotations(again, plain)
    assert gen.last_timing["regions_ms"] == 0.0
    # blob_edit: the cleaned masks as blobs, largest first
    blobs = blob_edit.ellipses_from_image(gen, image, min_region_area=m)
    fitted = []
    for a in sorted(want, key=lambda a: -a["area"]):
        try:
            fitted.append(blob_edit.ellipse_from_mask(a["segmentation"]))
        except ValueError:
            continue
    assert [e for e, _ in blobs] == fitted and len(fitted) >= 1


def painted_masks():
    """96 x 128, in the order of their scores: the disc plus a 2-pixel speck far away; the clean disc; another disc with a 1-pixel hole; five
    specks of 1 .. 5 pixels; a second clean disc."""
    H, W = 96, 128
    clean_disc = disc(H, W, 40, 40, 18)
    specked = clean_disc.copy()
    specked[90, 120] = specked[91, 121] = True
    holed = disc(H, W, 95, 60, 15)
    holed[60, 95] = False
    specks = np.zeros((H, W), dtype=bool)
    for k in range(5):
        specks[5 + 12 * k, 100:101 + k] = True
    return [specked, clean_disc, holed, specks, disc(H, W, 30, 80, 10)], np.array([0.99, 0.98, 0.97, 0.96, 0.95], dtype=np.float32)


def painted_generator():
    """A generator whose decoder is replaced by painted logits (+5 inside a mask, -5 outside): point p of the 3 x 3 grid answers with painted
    mask p in its first slot and empty masks with a low score elsewhere.  Everything behind the decoder is the real `generate`: bc_mask_stats,
    the filters, both NMS passes, clean_masks, the annotations."""
    painted, scores = painted_masks()
    H, W = painted[0].shape
    gen = sam.SamAutomaticMaskGenerator(model_a(), points_per_side=3, points_per_batch=4, pred_iou_thresh=0.5, stability_score_thresh=0.9,
                                        stability_score_offset=1.0, box_nms_thresh=0.7)
    pred = gen.predictor
    state = {"next": 0}

    def set_image(image, image_format="RGB"):
        pred.reset_image()
        pred.original_size, pred.input_size, pred.is_image_set = (H, W), (H, W), True
        state["next"] = 0

    def predict_batch(point_coords, point_labels, multimask_output, return_logits, mark=None):
        B = point_coords.shape[0]
        logits = torch.full((B, 3, H, W), -5.0, device="cuda")
        iou = torch.full((B, 3), 0.1, device="cuda")
        for b in range(B):
            p = state["next"] + b
            if p < len(painted):
                logits[b, 0] = dev(painted[p]).float() * 10 - 5
                iou[b, 0] = float(scores[p])
        state["next"] += B
        if mark is not None:
            mark()
        return logits, iou, None

    pred.set_image, pred._predict_batch = set_image, predict_batch
    return gen, painted, scores


def test_generate_reorders_and_drops_on_painted_masks():
    gen, painted, scores = painted_generator()
    image = np.zeros(painted[0].shape + (3,), np.uint8)
    plain = gen.generate(image)
    assert [a["predicted_iou"] for a in plain] == [float(v) for v in scores]             # the first NMS keeps all five, by score
    for a, m in zip(plain, painted):
        assert np.array_equal(a["segmentation"], m) and a["area"] == int(m.sum())
    got = gen.generate(image, min_mask_region_area=8)
    same_annotations(got, mc.postprocess_small_regions(plain, 8, 0.7))
    # unchanged masks first (the two clean discs), then the changed ones; the specked disc has become the first disc's duplicate and is gone
    assert [a["predicted_iou"] for a in got] == [float(scores[k]) for k in (1, 4, 2, 3)]
    assert np.array_equal(got[0]["segmentation"], painted[1]) and np.array_equal(got[1]["segmentation"], painted[4])
    assert got[2]["area"] == int(painted[2].sum()) + 1 and got[2]["segmentation"][60, 95] and got[2]["bbox"] == plain[2]["bbox"]
    assert got[3]["area"] == 5 and got[3]["bbox"] == [100, 53, 4, 0]
    for a in got:
        area, x0, y0, x1, y1 = mc.stats_of(a["segmentation"])
        assert a["area"] == area and a["bbox"] == [x0, y0, x1 - x0, y1 - y0] and set(a) == KEYS
    assert gen.last_timing["regions_ms"] > 0.0 and gen.last_timing["masks"] == 4
    # min_area 2: only the 1-pixel hole and the 1-pixel speck are below it, nothing is dropped, and the second clean disc moves up two places
    got = gen.generate(image, min_mask_region_area=2)
    same_annotations(got, mc.postprocess_small_regions(plain, 2, 0.7))
    assert [a["predicted_iou"] for a in got] == [float(scores[k]) for k in (0, 1, 4, 2, 3)]


def test_out_rows_that_are_not_aligned_to_eight_bytes():
    """`out` offset by one int: every row then starts 4 bytes off an 8-byte boundary, and the 64-bit word the roots pass hands to the apply
    pass lies in ints 1-2 of the row instead of 0-1.  The result must be that of the aligned call."""
    lib = _lib.load()
    batch = np.stack([mc.noise(37, 53, p) for p in mc.DENSITIES] + [mc.last_pixel(37, 53), np.zeros((37, 53), dtype=bool)])
    specks = np.zeros((37, 53), dtype=bool)
    specks[3, 3] = specks[20, 40] = specks[20, 41] = specks[36, 0] = specks[36, 1] = True     # two equal largest: the keep-the-largest key decides
    batch = np.concatenate([batch, specks[None]])
    n, H, W = batch.shape
    for mode in ("holes", "islands"):
        for thresh in (4, 50):
            want_masks, want_out = run_remove(batch, thresh, mode)
            work = dev(batch.astype(np.uint8))
            scratch = torch.empty(2, n, H, W, dtype=torch.int32, device="cuda")
            buf = torch.full((n * 6 + 1,), -7, dtype=torch.int32, device="cuda")
            out = buf[1:]
            assert out.data_ptr() % 8 == 4
            _lib.check(lib.bc_mask_remove_small(work.data_ptr(), n, H, W, thresh, masks.MODES[mode], scratch[0].data_ptr(), scratch[1].data_ptr(),
                                                out.data_ptr(), torch.cuda.current_stream().cuda_stream), "bc_mask_remove_small")
            assert int(buf[0]) == -7 and np.array_equal(out.view(n, 6).cpu().numpy(), want_out), (mode, thresh)
            assert np.array_equal(work.bool().cpu().numpy(), want_masks)
            for k in range(n):
                assert np.array_equal(want_masks[k], mc.remove_small_regions(batch[k], thresh, mode)[0])


class PaintedPredictor:
    """The call surface `ellipse_from_click` uses, answering with a painted mask."""

    def __init__(self, mask):
        self.mask = mask

    def set_image(self, image):
        pass

    def predict(self, point_coords=None, point_labels=None, multimask_output=True):
        return self.mask[None], np.zeros(1, np.float32), np.zeros((1, 64, 64), np.float32)


def test_ellipse_from_click_with_min_region_area():
    # a painted mask, so that there is something to remove: the disc with a speck far away and a pinhole
    painted, _ = painted_masks()
    specked, clean_disc = painted[0].copy(), painted[1]
    specked[40, 40] = False
    stub = PaintedPredictor(specked)
    image = np.zeros(specked.shape + (3,), np.uint8)
    want = blob_edit.ellipse_from_mask(clean_disc)
    assert mc.clean(specked, 8)[1] and np.array_equal(mc.clean(specked, 8)[0], clean_disc)
    assert blob_edit.ellipse_from_click(stub, image, [[40, 40]], min_region_area=8) == want
    assert blob_edit.ellipse_from_click(stub, image, [[40, 40]]) == blob_edit.ellipse_from_mask(specked) != want
    # and the predictor's own mask on fixture (a)
    gen = fixture_generator()
    pred = gen.predictor
    pred.set_image(np.zeros(sc.ORIGINAL_SIZE + (3,), np.uint8))
    point = (np.array(sc.CLICKS["one"][0]) * [sc.ORIGINAL_SIZE[1] / sc.INPUT_SIZE[1], sc.ORIGINAL_SIZE[0] / sc.INPUT_SIZE[0]]).tolist()
    raw = pred.predict(point_coords=np.asarray(point, np.float32), point_labels=np.ones(1, np.int32), multimask_output=False)[0][0]
    least = smallest_component(raw)
    m = 8 if least is None else least + 1
    cleaned, changed = mc.clean(raw, m)
    print(f"ellipse_from_click on the fixture: min_region_area {m} changes {int((cleaned != raw).sum())} pixels of the predictor's mask")
    assert blob_edit.ellipse_from_click(pred, None, point, min_region_area=m) == blob_edit.ellipse_from_mask(cleaned)
    assert blob_edit.ellipse_from_click(pred, None, point) == blob_edit.ellipse_from_mask(raw)
