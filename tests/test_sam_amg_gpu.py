"""Batched SAM prompts and SamAutomaticMaskGenerator on the GPU (blobctrl_amd/sam.py: decode_batch, predict_torch, generate; include/
blobctrl_sam.h: bc_sam_tokens_batch, bc_mask_stats).  Parity of the batched decoder is held to the bar of tests/test_sam_gpu.py (max-abs
error < 1e-2 of the reference's scale, PSNR > 40 dB) against the CPU restatement of tests/sam_common.py, against what transformers wrote for
one batched call (tests/golden/sam_amg.npz) and against the single-prompt `decode`; everything that is a decision - counts, boxes, the kept
set and its order - is compared exactly, on the GPU's own logits."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from blobctrl_amd import _lib, blob_edit, sam  # noqa: E402
from tests import sam_common as sc  # noqa: E402
from tests.common import g, psnr  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REL, DB = 1e-2, 40.0


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


def primed_predictor():
    """A SamPredictor holding fixture (a)'s frame (its pixels are no uint8 image: the encoder runs on the stored tensor, as in test_sam_gpu)."""
    model = model_a()
    pred = sam.SamPredictor(model)
    pred.features = model.encode(torch.from_numpy(tiny()["a_pixels_q8"]).float() / 32)
    model._emb_owner = id(pred)
    pred.original_size, pred.input_size, pred.is_image_set = sc.ORIGINAL_SIZE, sc.INPUT_SIZE, True
    return pred, model


@functools.lru_cache(maxsize=None)
def cpu_reference(points, labels):
    """tests/sam_common.py on the fixture's embedding for one prompt (tuples, so that it is computed once): (logits [4][64][64], IoU [4])."""
    with torch.no_grad():
        low, iou = sc.mask_decoder(sc.weights_of(sc.TINY_A), torch.from_numpy(tiny()["a_emb"])[0], [list(p) for p in points], list(labels),
                                   sc.TINY_A["image"])
    return low.numpy(), iou.numpy()


def assert_bar(out, ref, what):
    out, ref = np.asarray(out, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = float(np.abs(out - ref).max()) / float(np.abs(ref).max())
    db = psnr(out, ref)
    print(f"{what}: max-abs/scale {err:.3e}, PSNR {db:.1f} dB")
    assert np.isfinite(out).all() and err < REL and db > DB, f"{what}: max-abs/scale {err:.3e}, PSNR {db:.1f} dB"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_sam_tokens_batch_against_the_single_launch_and_the_restatement():
    model, lib = model_a(), _lib.load()
    f, ntok, C = model.f, model.ntok, model.C
    B, npts = 3, 2
    pts = torch.tensor([[[70.0, 90.0], [180.25, 40.5]], [[0.0, 255.0], [128.0, 96.0]], [[33.3, 191.9], [250.0, 1.0]]])
    labs = torch.tensor([[1, 0], [-1, 1], [0, -1]], dtype=torch.int32)
    dp, dl = pts.cuda(), labs.cuda()
    out = torch.full((B, ntok + npts + 1, C), float("nan"), dtype=torch.float16, device="cuda")
    _lib.check(lib.bc_sam_tokens_batch(f["tokens"].data_ptr(), ntok, dp.data_ptr(), dl.data_ptr(), B, npts, f["gauss"].data_ptr(), model.F,
                                       f["label_embed"].data_ptr(), f["not_a_point"].data_ptr(), float(model.image_size), out.data_ptr(), _stream()),
               "bc_sam_tokens_batch")
    one = torch.full((ntok + npts + 1, C), float("nan"), dtype=torch.float16, device="cuda")
    _lib.check(lib.bc_sam_tokens(f["tokens"].data_ptr(), ntok, dp[0].data_ptr(), dl[0].data_ptr(), npts, f["gauss"].data_ptr(), model.F,
                                 f["label_embed"].data_ptr(), f["not_a_point"].data_ptr(), float(model.image_size), one.data_ptr(), _stream()),
               "bc_sam_tokens")
    assert torch.equal(out[0].view(torch.int16), one.view(torch.int16)), "prompt 0 is not bit-identical to bc_sam_tokens"
    sd = sc.cast(sc.weights_of(sc.TINY_A), torch.float64)
    tokens = torch.cat([sd["mask_decoder.iou_token.weight"], sd["mask_decoder.mask_tokens.weight"]], 0)
    for b in range(B):
        rows = sc.prompt_tokens(sd, pts[b].double(), [max(int(v), 0) for v in labs[b]], model.image_size)
        for i in range(npts):
            if int(labs[b, i]) == -1:
                rows[i] = sd["prompt_encoder.not_a_point_embed.weight"][0]
        ref = torch.cat([tokens, rows], 0)
        # one rounding to fp16 of a value the kernel forms in fp32 from an fp64 angle: half an fp16 ulp (2^-11 relative, 2^-25 absolute in the
        # subnormals) plus the fp32 roundings in front of it (a few 2^-24 of a value of magnitude <= 2)
        tol = 2.0 ** -11 * ref.abs() + 2.0 ** -24 + 1e-6
        assert bool(((out[b].cpu().double() - ref).abs() <= tol).all()), f"prompt {b}: {float((out[b].cpu().double() - ref).abs().max()):.3e}"


def _grid_prompts(which):
    pts = amg()["points"][list(which)]
    return pts[:, None, :], np.ones((len(which), 1), dtype=np.int32)


def test_decode_batch_on_the_fixture():
    _, model = primed_predictor()
    z = amg()
    which = (0, 5, 10, 15, 3)
    pts, labs = _grid_prompts(which)
    plans = model.plans_recorded
    low, iou = model.decode_batch(pts, labs, multimask_output=None)
    assert model.plans_recorded == plans + 1
    assert tuple(low.shape) == (5, 4, 64, 64) and tuple(iou.shape) == (5, 4) and low.dtype == iou.dtype == torch.float32 and low.is_cuda
    low_m, iou_m = model.decode_batch(torch.from_numpy(pts).cuda(), torch.from_numpy(labs).cuda(), multimask_output=True)
    assert model.plans_recorded == plans + 1 and torch.equal(low_m, low[:, 1:]) and torch.equal(iou_m, iou[:, 1:])
    low_s, iou_s = model.decode_batch(pts, labs, multimask_output=False)
    assert torch.equal(low_s, low[:, :1]) and torch.equal(iou_s, iou[:, :1])
    stored = {int(p): k for k, p in enumerate(z["stored"])}
    identical = 0
    for k, p in enumerate(which):
        ref_low, ref_iou = cpu_reference((tuple(z["points"][p].tolist()),), (1,))
        assert_bar(low[k].cpu().numpy(), ref_low, f"prompt {p}: logits against the restatement")
        assert_bar(iou[k].cpu().numpy(), ref_iou, f"prompt {p}: IoU against the restatement")
        if p in stored:
            assert_bar(low[k, 1:].cpu().numpy(), z["low"][stored[p]], f"prompt {p}: logits against the fixture")
        one_low, one_iou = model.decode(z["points"][p][None], [1], multimask_output=None)
        assert_bar(low[k].cpu().numpy(), one_low.cpu().numpy(), f"prompt {p}: logits against the single-prompt decode")
        assert_bar(iou[k].cpu().numpy(), one_iou.cpu().numpy(), f"prompt {p}: IoU against the single-prompt decode")
        identical += int(torch.equal(low[k], one_low) and torch.equal(iou[k], one_iou))
    print(f"decode_batch: {identical} of {len(which)} prompts bit-identical to the single-prompt decode")
    # (the three multimask scores of all 16 prompts are one output of the reference's batched call)
    assert_bar(iou[:4, 1:].cpu().numpy(), z["iou"][[0, 5, 10, 15]], "IoU of the stored prompts against the fixture")
    # a permutation of the prompts permutes the outputs bit for bit: no prompt reads another one's rows, no buffer is shared by mistake
    perm = [3, 0, 4, 2, 1]
    low_p, iou_p = model.decode_batch(pts[perm], labs[perm], multimask_output=None)
    assert torch.equal(low_p, low[perm]) and torch.equal(iou_p, iou[perm])
    # Bp = 1: a plan of its own, the same numbers to the bar
    plans = model.plans_recorded
    low1, iou1 = model.decode_batch(pts[2:3], labs[2:3], multimask_output=None)
    assert model.plans_recorded == plans + 1 and tuple(low1.shape) == (1, 4, 64, 64)
    ref_low, ref_iou = cpu_reference((tuple(z["points"][10].tolist()),), (1,))
    assert_bar(low1[0].cpu().numpy(), ref_low, "Bp = 1: logits against the restatement")
    assert_bar(iou1[0].cpu().numpy(), ref_iou, "Bp = 1: IoU against the restatement")


def test_decode_batch_with_two_points_per_prompt():
    _, model = primed_predictor()
    prompts = [(((70.0, 90.0), (180.0, 40.0)), (1, 0)), (((180.0, 40.0), (70.0, 90.0)), (1, 0)), (((30.0, 30.0), (200.0, 150.0)), (1, 1))]
    pts = np.array([p for p, _ in prompts], dtype=np.float32)
    labs = np.array([l for _, l in prompts], dtype=np.int32)
    low, iou = model.decode_batch(pts, labs, multimask_output=None)
    assert tuple(low.shape) == (3, 4, 64, 64)
    for k, (p, l) in enumerate(prompts):
        ref_low, ref_iou = cpu_reference(p, l)
        assert_bar(low[k].cpu().numpy(), ref_low, f"two points, prompt {k}: logits")
        assert_bar(iou[k].cpu().numpy(), ref_iou, f"two points, prompt {k}: IoU")
    assert_bar(low[0, 1:].cpu().numpy(), tiny()["a_two_multi_low"], "two points, prompt 0: logits against the click fixture")
    low_p, iou_p = model.decode_batch(pts[[2, 0, 1]], labs[[2, 0, 1]], multimask_output=None)
    assert torch.equal(low_p, low[[2, 0, 1]]) and torch.equal(iou_p, iou[[2, 0, 1]])


def test_decode_batch_at_the_real_decoder_width():
    """C = 256, 8 heads (head sizes 32 / 16), the 64 x 64 grid (T = 4096) and two decoder layers, three prompts, behind the cheapest encoder
    that gives that grid (one global layer, hidden 128).  The CPU restatement is fed the GPU's own embedding: only the decoder is judged."""
    cfg = dict(image=1024, patch=16, window=14, layers=1, global_attn_indexes=(0,), hidden=128, heads=2, mlp_dim=256, out_channels=256,
               decoder_layers=2, decoder_mlp_dim=2048, iou_head_hidden_dim=256, seed=151)
    sd = sc.weights_of(cfg)
    model = sam.SamModel(sd, sam.SamConfig(num_heads=2, window_size=14, global_attn_indexes=(0,), decoder_heads=8))
    emb = model.encode(g(152, 1, 3, 1024, 1024))
    pts = np.array([[[100.0, 900.0]], [[512.5, 511.5]], [[1000.0, 20.0]]], dtype=np.float32)
    labs = np.array([[1], [1], [0]], dtype=np.int32)
    low, iou = model.decode_batch(pts, labs, multimask_output=None)
    assert tuple(low.shape) == (3, 4, 256, 256) and tuple(iou.shape) == (3, 4)
    for k in range(3):
        with torch.no_grad():
            ref_low, ref_iou = sc.mask_decoder(sd, emb[0].cpu(), pts[k].tolist(), labs[k].tolist(), 1024, heads=8)
        assert_bar(low[k].cpu().numpy(), ref_low.numpy(), f"full width, prompt {k}: logits")
        assert_bar(iou[k].cpu().numpy(), ref_iou.numpy(), f"full width, prompt {k}: IoU")
    one_low, one_iou = model.decode(pts[1], labs[1], multimask_output=None)
    assert_bar(low[1].cpu().numpy(), one_low.cpu().numpy(), "full width: logits against the single-prompt decode")
    assert_bar(iou[1].cpu().numpy(), one_iou.cpu().numpy(), "full width: IoU against the single-prompt decode")


def _thresholds(t, o):
    """The two outer thresholds as include/blobctrl_sam.h defines them: fp32 roundings of the sums of the fp32 arguments."""
    t32, o32 = np.float64(np.float32(t)), np.float64(np.float32(o))
    return float(np.float32(t32 + o32)), float(np.float32(t32 - o32))


def stats_reference(logits, t, o):
    """transformers' _compute_stability_score counts and _batched_mask_to_box, restated: int [n][7]."""
    hi, lo = _thresholds(t, o)
    n, H, W = logits.shape
    m = logits > float(np.float32(t))
    out = torch.zeros(n, 7, dtype=torch.int64)
    out[:, 0] = (logits > hi).flatten(1).sum(1)
    out[:, 1] = (logits > lo).flatten(1).sum(1)
    out[:, 2] = m.flatten(1).sum(1)
    rows, cols = m.any(2), m.any(1)
    ys, xs = torch.arange(H)[None, :], torch.arange(W)[None, :]
    y1, x1 = (rows * ys).max(1).values, (cols * xs).max(1).values
    y0, x0 = (rows * ys + H * (~rows)).min(1).values, (cols * xs + W * (~cols)).min(1).values
    empty = (x1 < x0) | (y1 < y0)
    out[:, 3:] = torch.stack([x0, y0, x1, y1], 1) * (~empty)[:, None]
    return out


@pytest.mark.parametrize("n,H,W", [(5, 37, 53), (2, 150, 200)])
@pytest.mark.parametrize("t,o", [(0.25, 0.5), (0.0, 0.05)])
def test_mask_stats_exact(n, H, W, t, o):
    model = model_a()
    hi, lo = _thresholds(t, o)
    x = g(160 + n, n, H, W) * 0.7 + float(t)
    # values exactly at the three thresholds (none of them counts: the comparisons are strict) and one ulp above each (all of them count)
    flat = x.view(n, -1)
    for k, v in enumerate((np.float32(t), np.float32(hi), np.float32(lo))):
        flat[0, 11 + 2 * k] = float(v)
        flat[0, 12 + 2 * k] = float(np.nextafter(v, np.float32(np.inf)))
    x[1] = float(lo) - 1.0                                              # empty at every threshold
    if n > 2:
        x[2] = float(hi) + 1.0                                          # full
        x[3] = float(lo) - 1.0
        x[3, H - 1, W - 1] = float(t) + float(o) / 2                    # a single pixel in the last row and column, between t and t + o
        x[4, :, : W // 2] = float(lo)                                   # exactly at t - o: outside all three
    ref = stats_reference(x, t, o)
    got = model.mask_stats(x.cuda(), t, o)
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 7)
    assert torch.equal(got.cpu().long(), ref), f"\n{got.cpu()}\n{ref}"
    assert ref[1].tolist() == [0] * 7
    if n > 2:
        assert ref[2].tolist() == [H * W] * 3 + [0, 0, W - 1, H - 1] and ref[3].tolist() == [0, 1, 1, W - 1, H - 1, W - 1, H - 1]
    # the same masks behind a base address that is not 16-byte aligned (the scalar-load form of the kernel) and as n = 1
    buf = torch.empty(1 + x.numel(), device="cuda")
    view = buf[1:].view(n, H, W)
    view.copy_(x)
    assert torch.equal(model.mask_stats(view, t, o), got)
    assert torch.equal(model.mask_stats(x[:1].cuda(), t, o), got[:1])


def test_predict_torch_shapes_and_agreement_with_predict():
    pred, model = primed_predictor()
    z = amg()
    which = [0, 5, 10]
    coords = pred.transform.apply_coords_torch(torch.from_numpy(z["grid"][which])[:, None, :].cuda(), pred.original_size)
    assert np.array_equal(coords.cpu().numpy()[:, 0], z["points"][which])
    labels = torch.ones(3, 1, dtype=torch.int32, device="cuda")
    masks, iou, low = pred.predict_torch(coords, labels, multimask_output=True)
    H, W = sc.ORIGINAL_SIZE
    assert masks.dtype == torch.bool and tuple(masks.shape) == (3, 3, H, W) and masks.is_cuda
    assert iou.dtype == torch.float32 and tuple(iou.shape) == (3, 3) and low.dtype == torch.float32 and tuple(low.shape) == (3, 3, 64, 64)
    soft, iou2, low2 = pred.predict_torch(coords, labels, multimask_output=True, return_logits=True)
    assert soft.dtype == torch.float32 and tuple(soft.shape) == (3, 3, H, W) and torch.equal(iou2, iou) and torch.equal(low2, low)
    assert torch.equal(soft > 0, masks)
    m1, i1, l1 = pred.predict_torch(coords, labels, multimask_output=False)
    assert tuple(m1.shape) == (3, 1, H, W) and tuple(i1.shape) == (3, 1) and tuple(l1.shape) == (3, 1, 64, 64)
    # one prompt through `predict` (original-image coordinates, numpy out): the same logits to the bar, the same mask away from the threshold
    pm, pi, pl = pred.predict(z["grid"][5][None], np.array([1]), multimask_output=True)
    ps, _, _ = pred.predict(z["grid"][5][None], np.array([1]), multimask_output=True, return_logits=True)
    assert_bar(low[1].cpu().numpy(), pl, "predict_torch against predict: low-res logits")
    assert_bar(np.concatenate([i1[1].cpu().numpy(), iou[1].cpu().numpy()]), np.concatenate([
        pred.predict(z["grid"][5][None], np.array([1]), multimask_output=False)[1], pi]), "predict_torch against predict: IoU")
    sure = np.abs(ps) >= 1e-2 * np.abs(ps).max()
    print(f"predict_torch against predict: {1 - sure.mean():.3f} of the pixels lie within 1e-2 of the logits' scale of the threshold")
    assert sure.mean() > 0.5 and np.array_equal(masks[1].cpu().numpy()[sure], pm[sure])


def amg_chain(pred, z, points_per_batch):
    """SamAutomaticMaskGenerator.generate restated in torch over the logits `predict_torch(return_logits=True)` returns, in the same batches."""
    H, W = sc.ORIGINAL_SIZE
    grid = z["grid"]
    coords = pred.transform.apply_coords_torch(torch.from_numpy(grid)[:, None, :].cuda(), pred.original_size)
    logits, ious = [], []
    for lo in range(0, 16, points_per_batch):
        hi = min(16, lo + points_per_batch)
        soft, iou, _ = pred.predict_torch(coords[lo:hi], torch.ones(hi - lo, 1, dtype=torch.int32, device="cuda"), multimask_output=True,
                                          return_logits=True)
        logits.append(soft.flatten(0, 1).cpu())
        ious.append(iou.flatten().cpu())
    logits, ious = torch.cat(logits), torch.cat(ious)
    point = torch.arange(16).repeat_interleave(3)
    t, o = 0.0, float(z["offset"])
    keep = torch.nonzero(ious > float(z["pred_iou_thresh"])).flatten()
    stats = stats_reference(logits[keep], t, o)
    stability = stats[:, 0].to(torch.float32) / stats[:, 1].to(torch.float32)
    sel = torch.nonzero(stability >= float(z["stability_score_thresh"])).flatten()
    keep, stats, stability = keep[sel], stats[sel], stability[sel]
    out = []
    for i in sam.box_nms(stats[:, 3:].numpy(), ious[keep].numpy(), float(z["box_nms_thresh"])):
        x0, y0, x1, y1 = stats[i, 3:].tolist()
        k = int(keep[i])
        out.append({"segmentation": (logits[k] > t).numpy(), "area": int(stats[i, 2]), "bbox": [x0, y0, x1 - x0, y1 - y0],
                    "predicted_iou": float(ious[k]), "point_coords": [grid[int(point[k])].tolist()], "stability_score": float(stability[i]),
                    "crop_box": [0, 0, W, H]})
    return out, int((ious > float(z["pred_iou_thresh"])).sum())


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y) == {"segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box"}
        assert x["segmentation"].dtype == np.bool_ and np.array_equal(x["segmentation"], y["segmentation"])
        for key in ("area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box"):
            assert x[key] == y[key], key


@functools.lru_cache(maxsize=None)
def fixture_generator():
    z = amg()
    model = model_a()
    gen = sam.SamAutomaticMaskGenerator(model, points_per_side=4, points_per_batch=5, pred_iou_thresh=float(z["pred_iou_thresh"]),
                                        stability_score_thresh=float(z["stability_score_thresh"]), stability_score_offset=float(z["offset"]),
                                        box_nms_thresh=float(z["box_nms_thresh"]))
    pred = gen.predictor

    def set_image(image, image_format="RGB"):
        # fixture (a)'s frame is a stored tensor, not a uint8 image: the encoder runs on it (set_image's host side has its own tests)
        assert tuple(np.asarray(image).shape) == sc.ORIGINAL_SIZE + (3,)
        pred.reset_image()
        pred.features = model.encode(torch.from_numpy(tiny()["a_pixels_q8"]).float() / 32)
        model._emb_owner = id(pred)
        pred.original_size, pred.input_size, pred.is_image_set = sc.ORIGINAL_SIZE, sc.INPUT_SIZE, True

    pred.set_image = set_image
    return gen


def test_generate_on_the_fixture_equals_the_restated_chain():
    z = amg()
    gen = fixture_generator()
    image = np.zeros(sc.ORIGINAL_SIZE + (3,), np.uint8)
    first = gen.generate(image)
    plans = gen.predictor.model.plans_recorded
    second = gen.generate(image)
    assert gen.predictor.model.plans_recorded == plans, "a second generate on an image of the same size recorded a plan"
    _same(second, first)
    want, after_iou = amg_chain(gen.predictor, z, 5)
    assert gen.predictor.model.plans_recorded == plans                      # (predict_torch in the same batches runs the same two plans)
    print(f"generate: 48 masks -> {after_iou} after the IoU filter -> {len(want)} returned; reference kept {len(z['ref_kept'])}")
    _same(first, want)
    assert 2 <= len(first) < after_iou < 48                                # both filters drop masks, and masks survive
    ious = [a["predicted_iou"] for a in first]
    assert ious == sorted(ious, reverse=True)
    for a in first:
        x, y, w, h = a["bbox"]
        ys, xs = np.nonzero(a["segmentation"])
        assert a["area"] == len(xs) > 0 and [x, y, x + w, y + h] == [xs.min(), ys.min(), xs.max(), ys.max()]
        assert a["segmentation"].shape == sc.ORIGINAL_SIZE and a["stability_score"] >= float(z["stability_score_thresh"])
        assert any(a["point_coords"][0] == p for p in z["grid"].tolist())
    assert set(gen.last_timing) >= {"set_image_ms", "decode_ms", "resize_ms", "stats_ms", "host_ms", "generate_ms"}


def test_ellipses_from_image_on_the_generated_masks():
    gen = fixture_generator()
    image = np.zeros(sc.ORIGINAL_SIZE + (3,), np.uint8)
    anns = gen.generate(image)
    blobs = blob_edit.ellipses_from_image(gen, image)
    # every generated mask an ellipse can be fitted to (the hull of a noise mask that fills the frame is nearly its rectangle, and
    # fit_ellipse refuses points that determine no ellipse: such a mask is left out), largest area first
    want = []
    for a in sorted(anns, key=lambda a: -a["area"]):
        try:
            want.append((blob_edit.ellipse_from_mask(a["segmentation"].astype(np.uint8)), a["area"]))
        except ValueError:
            pass
    print(f"ellipses_from_image: {len(want)} of {len(anns)} generated masks have an ellipse")
    assert len(want) >= 2 and [(e, a["area"]) for e, a in blobs] == want
    areas = [a["area"] for _, a in blobs]
    assert areas == sorted(areas, reverse=True)
    for _, a in blobs:
        assert any(a["predicted_iou"] == b["predicted_iou"] and np.array_equal(a["segmentation"], b["segmentation"]) for b in anns)
    big = blob_edit.ellipses_from_image(gen, image, min_area=areas[0])
    assert [a["area"] for _, a in big] == [v for v in areas if v >= areas[0]]
