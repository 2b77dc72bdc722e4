"""Blob visualisation, feature grid and score pyramid on the MI355X against fixtures made by the real reference
(tests/golden/blob_viz.npz, tools/make_golden.py::golden_blob_viz): the app's blob image call (scripts/blobctrl_app.py:637-650), the
dictionary return of blobctrl/utils/utils.py:226-241, splat_features_from_scores (ut:57-77, pipeline_blobnet.py:706-721) and
pyramid_resize (ut:280-294).

Bars.  fp64: rtol 1e-9, atol 1e-12, the bar tests/test_kernels_gpu.py::test_splat_against_reference_fixtures holds the fp64 rasteriser
to; the new outputs add at most M + 6 fp64 roundings on top of it.  fp32: atol = (1e-6 + max(H_in, W_in) * 2**-23) * max|ref|, rtol 0:
M + 6 fp32 roundings of 6e-8 each, plus - only where the scores are resampled - the reference's own error: torch computes the sampling
position in fp32, one ulp of a position up to max(H_in, W_in), times a neighbour difference of at most max|ref|."""
import numpy as np
import pytest
import torch

from tests import blob_viz_common as bv

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
DEV = "cuda:0"


def _close(got, ref, what=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    err = np.abs(got - ref).max()
    print(f"{what}: max abs err {err:.3e} (|ref| max {np.abs(ref).max():.3e})")
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=what)


def _app_call(blob, viz_size, colors, fn=lambda score: score):
    """scripts/blobctrl_app.py:638-646 keyword for keyword, with the caller's palette."""
    from blobctrl_amd.splat import splat_features
    return splat_features(**blob, interp_size=64, viz_size=viz_size, is_viz=True, ret_layout=True, score_size=64, viz_score_fn=fn,
                          viz_colors=colors, only_vis=True, device=DEV)


def test_app_blob_images_against_reference_fixtures(golden_dir):
    z, meta = bv.load_fixture(golden_dir)
    colors = torch.from_numpy(z["viz_colors"])
    for i, c in enumerate(meta["app"]):
        ret = _app_call(bv.blob_kwargs(c["ellipse"], c["W"], c["H"], c["size"]), tuple(c["viz"]), colors)
        assert set(ret) == {"feature_img"} and ret["feature_img"].device.type == "cuda"
        _close(ret["feature_img"], z[f"app_{i}"], c["name"])
    c = meta["app"][1]
    seen = []

    def fn(score):                              # any callable, applied to the raw scores on the device, before compositing
        seen.append((score.device.type, tuple(score.shape), float(score[..., 0].min())))
        return bv.viz_boost(score)
    _close(_app_call(bv.blob_kwargs(c["ellipse"], 512, 512), (40, 40), colors, fn)["feature_img"], z["app_boost"], "boosted")
    assert seen == [("cuda", (1, 40, 40, 2), 1.0)]
    # colours per image [N, K, 3] (ut:254-256) give the same picture as the shared table
    ret = _app_call(bv.blob_kwargs(c["ellipse"], 512, 512), (40, 40), colors[None])
    _close(ret["feature_img"], z["app_1"], "per-image colours")


def test_dictionary_return_against_reference_fixtures(golden_dir):
    from blobctrl_amd.splat import splat_features
    z, meta = bv.load_fixture(golden_dir)
    colors, feats = torch.from_numpy(z["viz_colors"]), torch.from_numpy(z["dict_features"])
    d = meta["dict"]
    blob0, blob1 = bv.blob_kwargs(d["ellipse"], d["W"], d["H"]), bv.blob_kwargs(d["ns_ellipse"], d["ns_W"], d["ns_H"])
    r0 = splat_features(**blob0, score_size=(64, 64), interp_size=16, features=feats, device=DEV)
    r1 = splat_features(**blob1, score_size=(48, 80), interp_size=20, features=feats, is_viz=True, viz_size=32, viz_colors=colors, device=DEV)
    for tag, r, blob in (("d0", r0, blob0), ("d1", r1, blob1)):
        assert sorted(r.keys()) == meta[tag + "_keys"]
        assert r["feature_img"] is None and r["entropy_img"] is None
        assert sorted(r["scores_pyramid"]) == meta[tag + "_levels"]
        for k, lvl in r["scores_pyramid"].items():
            _close(lvl, z[f"{tag}_pyr_{k}"], f"{tag} pyramid level {k}")
        for k in ("feature_grid", "raw_scores", "composed_scores"):
            _close(r[k], z[f"{tag}_{k}"], f"{tag} {k}")
        assert r["xs"] is blob["xs"] and r["covs"] is blob["covs"] and r["features"] is feats
    assert tuple(r1["scores_pyramid"][40].shape) == (1, 2, 40, 40)                 # square below the first level
    no_layout = splat_features(**blob0, score_size=(64, 64), interp_size=16, features=feats, ret_layout=False, device=DEV)
    assert sorted(no_layout) == ["entropy_img", "feature_grid", "feature_img", "scores_pyramid"]
    k = meta["keyerror"]
    with pytest.raises(KeyError):
        splat_features(**blob1, score_size=tuple(k["score_size"]), interp_size=k["interp_size"], features=feats, device=DEV)


def test_int_viz_size_and_fg_bg_selection_against_reference_fixtures(golden_dir):
    from blobctrl_amd.splat import splat_features
    z, meta = bv.load_fixture(golden_dir)
    colors = torch.from_numpy(z["viz_colors"])
    blob = bv.blob_kwargs(meta["dict"]["ellipse"], 512, 512)
    r = splat_features(**blob, score_size=(64, 64), viz_size=32, is_viz=True, viz_colors=colors, only_vis=True, device=DEV)
    _close(r["feature_img"], z["vis_int32"], "int viz_size")
    fg = splat_features(**blob, score_size=(64, 64), return_d_score=True, only_splatting_fg=True, device=DEV)
    bg = splat_features(**blob, score_size=(64, 64), return_d_score=True, only_splatting_bg=True, device=DEV)
    _close(fg.contiguous(), z["fg_only"], "fg only")
    _close(bg.contiguous(), z["bg_only"], "bg only")
    both = splat_features(**blob, score_size=(64, 64), return_d_score=True, device=DEV)
    assert torch.equal(torch.cat([bg, fg], 1), both)


def test_composed_maps_equal_the_pipeline_rasteriser_bit_for_bit(golden_dir):
    from blobctrl_amd import ops  # noqa: F401
    z, meta = bv.load_fixture(golden_dir)
    cases = [(c["ellipse"], c["W"], c["H"], c["viz"], c["size"]) for c in meta["app"]]
    cases.append((meta["full"]["ellipse"], 512, 512, [512, 512], 1.0))
    s = np.load(golden_dir + "/splat.npz")
    import json
    cases += [(m["ellipse"], m["W"], m["H"], [m["h"], m["w"]], 1.0) for m in json.loads(str(s["meta"]))]
    for ell, W, H, (h, w), size in cases:
        b = bv.blob_kwargs(ell, W, H, size)
        prm = torch.zeros(1, 8, dtype=torch.float64)
        prm[0, 0], prm[0, 1], prm[0, 2:6], prm[0, 6] = b["xs"][0], b["ys"][0], b["covs"].reshape(4), size
        raw, comp = torch.ops.blobctrl.splat_maps(prm, h, w, 0)
        ref = torch.ops.blobctrl.splat_scores(prm, h, w, 0)
        assert torch.equal(comp.permute(0, 3, 1, 2), ref), ell
        assert torch.equal(raw[..., 1], ref[:, 1]) and bool((raw[..., 0] == 1).all())
        assert torch.equal(torch.ops.blobctrl.alpha_composite(raw), comp)


def test_splat_from_scores_and_pyramid_against_reference_fixtures(golden_dir):
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    from blobctrl_amd.splat import pyramid_resize, splat_features_from_scores
    z, meta = bv.load_fixture(golden_dir)
    S, F = z["sfs_scores"], z["sfs_features"]
    pipe = StableDiffusionBlobNetPipeline.__new__(StableDiffusionBlobNetPipeline)      # the method needs no component
    for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        s_cf, f = torch.from_numpy(S).to(tdt).to(DEV), torch.from_numpy(F).to(tdt)
        for cl in (0, 1):
            for tag, size in (("none", None), ("7", 7), ("9x14", (9, 14))):
                ref = z[f"sfs_{dt}_cl{cl}_{tag}"]
                # channels-last both as a contiguous tensor and as a strided view of the channels-first one: no transposed copy is needed
                variants = [s_cf.permute(0, 2, 3, 1).contiguous(), s_cf.permute(0, 2, 3, 1)] if cl else [s_cf]
                for sc in variants:
                    for call in (splat_features_from_scores, pipe.splat_features_from_scores):
                        got = call(sc, f, size, channels_last=bool(cl))
                        assert got.is_contiguous() and got.device.type == "cuda"
                        if dt == "f64":
                            _close(got, ref, f"from_scores {dt} cl{cl} {tag}")
                        else:
                            got = got.cpu().numpy()
                            assert got.dtype == np.float32 and got.shape == ref.shape
                            bound = (1e-6 + (max(9, 14) * 2.0 ** -23 if size == 7 else 0.0)) * np.abs(ref).max()
                            err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
                            print(f"from_scores {dt} cl{cl} {tag}: max abs err {err:.3e} (bound {bound:.3e})")
                            assert err <= bound
    with pytest.raises(TypeError):
        splat_features_from_scores(torch.from_numpy(S).half().to(DEV), torch.from_numpy(F), None, channels_last=False)
    pyr = pyramid_resize(torch.from_numpy(z["pyr_in"]).to(DEV), 20)
    assert sorted(pyr) == meta["pyr_levels"]
    for k in (40, 20):
        _close(pyr[k], z[f"pyr_{k}"], f"pyramid_resize level {k}")
    p32 = pyramid_resize(torch.from_numpy(z["pyr_in"]).float().to(DEV), 20)
    for k in (40, 20):                          # fp32 instantiation of the resize: the fp32 bar with H_in, W_in of the level above
        bound = (1e-6 + 80 * 2.0 ** -23) * np.abs(z[f"pyr_{k}"]).max()
        assert p32[k].dtype == torch.float32 and np.abs(p32[k].cpu().numpy().astype(np.float64) - z[f"pyr_{k}"]).max() <= bound


def test_blob_overlay_bytes_against_the_reference_image(golden_dir):
    from blobctrl_amd.blob_edit import blob_overlay
    z, meta = bv.load_fixture(golden_dir)
    full = meta["full"]
    ref = z["full_u8"]
    assert full["near"] == len(z["full_near_pos"]) <= 1e-4 * ref.size            # the condition on the fixture
    got = blob_overlay(full["ellipse"], full["H"], full["W"], torch.from_numpy(z["viz_colors"]), device=DEV)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == ref.shape == (512, 512, 3)
    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    allowed = np.zeros(diff.shape, dtype=bool)
    if full["near"]:
        allowed[tuple(z["full_near_pos"].T)] = True
    print(f"blob_overlay: {int((diff != 0).sum())} of {diff.size} bytes differ, {full['near']} near-integer positions recorded")
    assert (diff[~allowed] == 0).all() and diff.max() <= 1
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 2                        # a picture, not two flat colours


def test_a_second_call_on_the_same_stream_returns_the_new_image(golden_dir):
    from blobctrl_amd.blob_edit import blob_overlay
    z, meta = bv.load_fixture(golden_dir)
    colors = torch.from_numpy(z["viz_colors"])
    a, b = meta["app"][1], meta["app"][0]
    assert a["ellipse"] == meta["full"]["ellipse"] and a["ellipse"] != b["ellipse"]
    first = blob_overlay(a["ellipse"], 512, 512, colors, device=DEV)
    second = blob_overlay(b["ellipse"], 512, 512, colors, device=DEV)
    again = blob_overlay(a["ellipse"], 512, 512, colors, device=DEV)
    assert np.array_equal(first, z["full_u8"]) or meta["full"]["near"] > 0
    assert not np.array_equal(first, second) and np.array_equal(first, again)
    for c, img in ((a, first), (b, second)):        # each image shows its own blob: the blob colour sits at the ellipse centre
        (xc, yc), _, _ = c["ellipse"]
        assert np.abs(img[int(round(yc)), int(round(xc))].astype(np.float64) - 255 * z["viz_colors"][1]).max() <= 2
    i0 = _app_call(bv.blob_kwargs(a["ellipse"], 512, 512), (40, 40), colors)["feature_img"]
    i1 = _app_call(bv.blob_kwargs(b["ellipse"], 512, 512), (40, 40), colors)["feature_img"]
    _close(i0, z["app_1"], "first")
    _close(i1, z["app_0"], "second")


def test_new_ops_pass_opcheck():
    from blobctrl_amd import ops  # noqa: F401
    prm = torch.tensor([[0.4, 0.6, 0.01, 0.002, 0.002, 0.02, 1.0, 0.0]], dtype=torch.float64)
    tests = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.blobctrl.splat_maps, (prm, 8, 16, 0), test_utils=tests)
    raw = torch.ops.blobctrl.splat_maps(prm, 8, 16, 0)[0]
    torch.library.opcheck(torch.ops.blobctrl.alpha_composite, (raw,), test_utils=tests)
    colors = torch.rand(1, 2, 3, dtype=torch.float64, device=DEV)
    torch.library.opcheck(torch.ops.blobctrl.splat_from_scores, (raw, colors, 5, 7, True), test_utils=tests)
    torch.library.opcheck(torch.ops.blobctrl.resize_bilinear, (raw.permute(0, 3, 1, 2).contiguous(), 4, 4), test_utils=tests)
    img = torch.ops.blobctrl.splat_from_scores(raw, colors, 8, 16, True)
    torch.library.opcheck(torch.ops.blobctrl.pack_rgb8, (img,), test_utils=tests)
