"""Blob visualisation, feature grid and score pyramid without a GPU: the five new `torch.ops.blobctrl.*` ops exist with their schemas and
fake kernels, the Python surface keeps the reference's refusals, and the fixture made by the real reference (tests/golden/blob_viz.npz,
tools/make_golden.py::golden_blob_viz) agrees with the plain numpy restatement of tests/blob_viz_common.py - which pins the tests' own
reading of blobctrl/utils/utils.py:57-77, 120-241, 280-294.  The kernels themselves: tests/test_blob_viz_gpu.py."""
import numpy as np
import pytest
import torch

from tests import blob_viz_common as bv

RTOL, ATOL = 1e-9, 1e-12


def _blob():
    return dict(xs=torch.tensor([0.5]), ys=torch.tensor([0.5]), covs=torch.eye(2).reshape(1, 1, 2, 2) * 0.01, sizes=torch.tensor([[1.0]]))


def test_new_ops_are_registered_with_the_expected_schemas():
    from blobctrl_amd import ops  # noqa: F401
    schema = lambda n: str(getattr(torch.ops.blobctrl, n).default._schema)
    assert schema("splat_maps") == "blobctrl::splat_maps(Tensor params, SymInt h, SymInt w, SymInt device_index) -> Tensor[]"
    assert schema("alpha_composite") == "blobctrl::alpha_composite(Tensor raw) -> Tensor"
    assert schema("splat_from_scores") == ("blobctrl::splat_from_scores(Tensor scores, Tensor features, SymInt out_h, SymInt out_w, "
                                           "bool channels_last) -> Tensor")
    assert schema("resize_bilinear") == "blobctrl::resize_bilinear(Tensor img, SymInt out_h, SymInt out_w) -> Tensor"
    assert schema("pack_rgb8") == "blobctrl::pack_rgb8(Tensor img) -> Tensor"
    # the four earlier ops keep their schemas
    assert schema("splat_scores") == "blobctrl::splat_scores(Tensor params, SymInt h, SymInt w, SymInt device_index) -> Tensor"


def test_fake_kernels_state_the_fixture_shapes(golden_dir):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from blobctrl_amd import ops  # noqa: F401
    z, meta = bv.load_fixture(golden_dir)
    with FakeTensorMode():
        raw, comp = torch.ops.blobctrl.splat_maps(torch.zeros(1, 8, dtype=torch.float64), 48, 80, 0)
        for t in (raw, comp):
            assert tuple(t.shape) == z["d1_raw_scores"].shape == (1, 48, 80, 2) and t.dtype == torch.float64 and t.device.type == "cuda"
        d = torch.ops.blobctrl.alpha_composite(raw)
        assert tuple(d.shape) == tuple(raw.shape) and d.dtype == torch.float64 and d.device == raw.device
        colors = torch.empty(1, 2, 3, dtype=torch.float64, device=raw.device)
        img = torch.ops.blobctrl.splat_from_scores(raw, colors, 32, 32, True)
        assert tuple(img.shape) == z["vis_int32"].shape == (1, 3, 32, 32) and img.dtype == torch.float64 and img.device == raw.device
        s32 = torch.empty(2, 3, 9, 14, dtype=torch.float32, device=raw.device)
        g = torch.ops.blobctrl.splat_from_scores(s32, torch.empty(2, 3, 5, dtype=torch.float32, device=raw.device), 7, 7, False)
        assert tuple(g.shape) == z["sfs_f32_cl0_7"].shape == (2, 5, 7, 7) and g.dtype == torch.float32
        lvl = torch.ops.blobctrl.resize_bilinear(comp.permute(0, 3, 1, 2), 40, 40)
        assert tuple(lvl.shape) == z["d1_pyr_40"].shape == (1, 2, 40, 40) and lvl.dtype == torch.float64 and lvl.device == raw.device
        full = torch.empty(1, 3, 512, 512, dtype=torch.float64, device=raw.device)
        u8 = torch.ops.blobctrl.pack_rgb8(full)
        assert tuple(u8.shape) == z["full_u8"].shape == (512, 512, 3) and u8.dtype == torch.uint8 and u8.device == raw.device


def test_new_branches_refuse_to_run_without_the_gpu():
    from blobctrl_amd import _lib
    from blobctrl_amd.splat import pyramid_resize, splat_features, splat_features_from_scores
    colors = torch.rand(4, 3)
    with pytest.raises(_lib.BlobCtrlHipError):
        splat_features(**_blob(), is_viz=True, only_vis=True, viz_size=(8, 8), viz_colors=colors, device="cpu")
    with pytest.raises(_lib.BlobCtrlHipError):
        splat_features(**_blob(), score_size=(8, 8), interp_size=4, features=torch.zeros(1, 2, 3), device="cpu")
    with pytest.raises(_lib.BlobCtrlHipError):
        splat_features(**_blob(), score_size=(8, 8), return_d_score=True, only_splatting_fg=True, device="cpu")
    with pytest.raises(_lib.BlobCtrlHipError):
        splat_features_from_scores(torch.zeros(1, 4, 4, 2, dtype=torch.float64), torch.zeros(1, 2, 3), None)
    with pytest.raises(_lib.BlobCtrlHipError):
        pyramid_resize(torch.zeros(1, 2, 8, 8, dtype=torch.float64), 4)
    with pytest.raises(_lib.BlobCtrlHipError):
        torch.ops.blobctrl.pack_rgb8(torch.zeros(1, 3, 4, 4, dtype=torch.float64))


def test_refusals_the_reference_surface_keeps():
    from blobctrl_amd.splat import splat_features, splat_features_from_scores
    colors = torch.rand(4, 3)
    with pytest.raises(NotImplementedError):                     # the square int branch (ut:137-144) has no caller in the reference
        splat_features(**_blob(), score_size=64, return_d_score=True)
    with pytest.raises(NotImplementedError):
        splat_features(**_blob(), score_size=64, viz_size=32, is_viz=True, viz_colors=colors, only_vis=True)
    two = dict(xs=torch.tensor([[0.4, 0.6]]), ys=torch.tensor([[0.5, 0.5]]), covs=(torch.eye(2) * 0.01).expand(1, 2, 2, 2),
               sizes=torch.tensor([[1.0, 1.0]]))
    with pytest.raises(ValueError):                              # ut:132-133, 157-158 hard-code one blob
        splat_features(**two, viz_size=(8, 8), is_viz=True, viz_colors=colors, only_vis=True)
    with pytest.raises(NotImplementedError, match="viz_colors"):  # random colours from the global RNG (ut:249-265) are out of scope
        splat_features(**_blob(), viz_size=(8, 8), is_viz=True, only_vis=True)
    for bad in (torch.zeros(1, 4, 4, 2, dtype=torch.float16), torch.zeros(1, 4, 4, 2, dtype=torch.int64)):
        with pytest.raises(TypeError):
            splat_features_from_scores(bad, torch.zeros(1, 2, 3), None)


def test_fixture_app_images_agree_with_the_numpy_restatement(golden_dir):
    z, meta = bv.load_fixture(golden_dir)
    colors = z["viz_colors"].astype(np.float64)
    assert colors.shape == (29, 3) and z["viz_colors"].dtype == np.float32
    names = [c["name"] for c in meta["app"]]
    assert {"nonsquare", "degenerate", "absent"} <= set(names) and len(names) >= 7
    assert meta["app"][names.index("nonsquare")]["viz"] == [48, 80] and meta["app"][names.index("absent")]["size"] == 0.2
    for i, c in enumerate(meta["app"]):
        h, w = c["viz"]
        raw = bv.raw_scores(c["ellipse"], c["W"], c["H"], h, w, c["size"])
        img = bv.from_scores(bv.composite(raw), colors[None, :2], (h, w))
        assert z[f"app_{i}"].dtype == np.float64
        np.testing.assert_allclose(z[f"app_{i}"], img, rtol=RTOL, atol=ATOL, err_msg=c["name"])
    c = meta["app"][1]
    raw = torch.from_numpy(bv.raw_scores(c["ellipse"], 512, 512, 40, 40))
    img = bv.from_scores(bv.composite(bv.viz_boost(raw).numpy()), colors[None, :2], (40, 40))
    np.testing.assert_allclose(z["app_boost"], img, rtol=RTOL, atol=ATOL)
    assert np.abs(z["app_boost"] - z["app_1"]).max() > 1e-3      # the boost is visible: the case is not the identity in disguise


def test_fixture_full_resolution_image_and_its_near_integer_record(golden_dir):
    z, meta = bv.load_fixture(golden_dir)
    full = meta["full"]
    assert z["full_u8"].shape == (512, 512, 3) and z["full_u8"].dtype == np.uint8
    assert len(z["full_near_pos"]) == len(z["full_near_val"]) == full["near"] <= 1e-4 * z["full_u8"].size
    raw = bv.raw_scores(full["ellipse"], 512, 512, 512, 512)
    img = bv.from_scores(bv.composite(raw), z["viz_colors"].astype(np.float64)[None, :2], (512, 512))[0].transpose(1, 2, 0)
    u8 = (img * 255).astype(np.uint8)
    diff = np.abs(u8.astype(np.int16) - z["full_u8"].astype(np.int16))
    allowed = np.zeros(diff.shape, dtype=bool)
    if full["near"]:
        allowed[tuple(z["full_near_pos"].T)] = True
    assert (diff[~allowed] == 0).all() and diff.max() <= 1
    assert full["reference_cpu_ms_median_of_5"] > 0


def test_fixture_dictionary_returns_agree_with_the_numpy_restatement(golden_dir):
    z, meta = bv.load_fixture(golden_dir)
    feats = z["dict_features"]
    assert feats.shape == (1, 2, 16)
    d = meta["dict"]
    layout = {"xs", "ys", "covs", "raw_scores", "sizes", "composed_scores", "features"}
    for tag, ell, W, H, h, w, interp in (("d0", d["ellipse"], d["W"], d["H"], 64, 64, 16), ("d1", d["ns_ellipse"], d["ns_W"], d["ns_H"], 48, 80, 20)):
        assert set(meta[tag + "_keys"]) == layout | {"scores_pyramid", "feature_grid", "feature_img", "entropy_img"}
        raw = bv.raw_scores(ell, W, H, h, w)
        comp = bv.composite(raw)
        np.testing.assert_allclose(z[f"{tag}_raw_scores"], raw, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(z[f"{tag}_composed_scores"], comp, rtol=RTOL, atol=ATOL)
        pyr = bv.pyramid(comp.transpose(0, 3, 1, 2), interp)
        assert sorted(pyr) == meta[tag + "_levels"]
        for k, lvl in pyr.items():
            assert z[f"{tag}_pyr_{k}"].shape == lvl.shape
            np.testing.assert_allclose(z[f"{tag}_pyr_{k}"], lvl, rtol=RTOL, atol=ATOL)
        grid = bv.from_scores(pyr[interp], feats, interp, channels_last=False)
        assert z[f"{tag}_feature_grid"].shape == (1, 16, interp, interp)
        np.testing.assert_allclose(z[f"{tag}_feature_grid"], grid, rtol=RTOL, atol=ATOL)
    assert meta["d1_levels"] == [20, 40, 80] and z["d1_pyr_40"].shape == (1, 2, 40, 40)      # square below the first level
    assert meta["keyerror"] == {"score_size": [48, 80], "interp_size": 16} and 16 not in bv.pyramid(np.zeros((1, 2, 48, 80)), 16)
    # int viz_size, fg / bg selection
    raw = bv.raw_scores(d["ellipse"], 512, 512, 64, 64)
    comp = bv.composite(raw)
    np.testing.assert_allclose(z["vis_int32"], bv.from_scores(comp, z["viz_colors"].astype(np.float64)[None, :2], 32), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(z["fg_only"], comp.transpose(0, 3, 1, 2)[:, 1:], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(z["bg_only"], comp.transpose(0, 3, 1, 2)[:, :1], rtol=RTOL, atol=ATOL)


def test_fixture_stand_alone_helpers_agree_with_the_numpy_restatement(golden_dir):
    z, meta = bv.load_fixture(golden_dir)
    S, F = z["sfs_scores"], z["sfs_features"]
    assert S.shape == (2, 3, 9, 14) and F.shape == (2, 3, 5)
    for dt, npdt in (("f64", np.float64), ("f32", np.float32)):
        s, f = S.astype(npdt), F.astype(npdt)
        for cl in (0, 1):
            sc = s.transpose(0, 2, 3, 1) if cl else s
            for tag, size in (("none", None), ("7", 7), ("9x14", (9, 14))):
                got = z[f"sfs_{dt}_cl{cl}_{tag}"]
                ref = bv.from_scores(sc, f, size, channels_last=bool(cl))
                assert got.dtype == npdt and got.shape == ref.shape == ((2, 5, 7, 7) if size == 7 else (2, 5, 9, 14))
                if dt == "f64":
                    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
                else:            # the reference's own fp32 error against the exact value: the bar of the fp32 GPU test
                    bound = (1e-6 + (14 * 2.0 ** -23 if size == 7 else 0.0)) * np.abs(ref).max()
                    assert np.abs(got - ref).max() <= bound
    pyr = bv.pyramid(z["pyr_in"], 20)
    assert sorted(pyr) == meta["pyr_levels"] == [20, 40, 80]
    for k in (40, 20):
        assert z[f"pyr_{k}"].shape == (1, 2, k, k)
        np.testing.assert_allclose(z[f"pyr_{k}"], pyr[k], rtol=RTOL, atol=ATOL)
