"""Host side of the Segment-Anything path (blobctrl_amd/sam.py) and the yardstick of its GPU tests: the plain-torch restatement of
tests/sam_common.py reproduces the fixture transformers' SamModel wrote (tests/golden/sam_tiny.npz) to 1e-5 of scale; the checkpoint
rename table round-trips; SamPredictor's preprocessing, point scaling and window geometry; the refusals."""
import os

import numpy as np
import pytest
import torch

from blobctrl_amd import _lib, sam, synth
from tests import sam_common as sc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_tiny.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _pixels(gold, tag):
    return torch.from_numpy(gold[f"{tag}_pixels_q8"]).float() / 32


@pytest.mark.parametrize("tag,cfg,scale", [("a", sc.TINY_A, 1.0), ("b", sc.TINY_B, 1.0), ("a8", sc.TINY_A, 8.0)])
def test_restatement_reproduces_the_fixture(gold, tag, cfg, scale):
    sd = sc.weights_of(cfg, scale)
    with torch.no_grad():
        emb = sc.vision_encoder(_pixels(gold, tag), sd, cfg["heads"], cfg["window"], cfg["global_attn_indexes"])
        assert sc.rel_err(emb, gold[f"{tag}_emb"]) < 1e-5
        ref_emb = torch.from_numpy(gold[f"{tag}_emb"])[0]
        for name, (pts, labs) in sc.CLICKS.items():
            low, iou = sc.mask_decoder(sd, ref_emb, pts, labs, cfg["image"])
            # (the scale of an IoU score is that of the four scores of a click, not of the one a slice picks: one of them is near zero)
            all_iou = np.concatenate([gold[f"{tag}_{name}_single_iou"], gold[f"{tag}_{name}_multi_iou"]])
            assert sc.rel_err(iou, all_iou) < 1e-5, (tag, name)
            for kind, sel in (("single", slice(0, 1)), ("multi", slice(1, None))):
                key = f"{tag}_{name}_{kind}"
                assert sc.rel_err(low[sel], gold[key + "_low"]) < 1e-5, key
                if key + "_mask" in gold:
                    logits = sc.postprocess(low[sel], cfg["image"], sc.INPUT_SIZE, sc.ORIGINAL_SIZE)
                    sure = logits.abs() >= float(gold[key + "_margin"])
                    assert float((~sure).float().mean()) <= 0.10
                    assert torch.equal((logits > 0)[sure], torch.from_numpy(gold[key + "_mask"])[sure])


def test_fixture_is_not_degenerate(gold):
    for tag in ("a", "b", "a8"):
        assert 0.1 < float(gold[f"{tag}_emb_absmax"]) < 100 and np.isclose(np.abs(gold[f"{tag}_emb"]).max(), gold[f"{tag}_emb_absmax"])
    assert float(gold["a8_masked_padding_moves_bars"]) > 10
    sd = sc.weights_of(sc.TINY_A)
    for k in ("vision_encoder.layers.0.attn.rel_pos_h", "vision_encoder.layers.1.attn.rel_pos_w", "vision_encoder.pos_embed",
              "vision_encoder.neck.conv1.weight", "vision_encoder.neck.conv2.weight"):
        assert float(sd[k].std()) > 0.02, k
    assert sd["vision_encoder.layers.0.attn.rel_pos_h"].shape == (13, 80) and sd["vision_encoder.layers.1.attn.rel_pos_h"].shape == (31, 80)
    vit_h = synth.sam_param_shapes()
    assert vit_h["vision_encoder.layers.7.attn.rel_pos_h"] == (127, 80) and vit_h["vision_encoder.layers.0.attn.rel_pos_w"] == (27, 80)
    assert vit_h["vision_encoder.pos_embed"] == (1, 64, 64, 1280) and vit_h["mask_decoder.upscale_conv2.weight"] == (64, 32, 2, 2)


def test_checkpoint_rename_table_round_trips():
    sd = sc.weights_of(sc.TINY_B)
    original = {}
    for k, v in sd.items():
        ok = sam.original_checkpoint_key(k)
        if ok is not None:
            assert ok not in original, ok
            original[ok] = v
    assert "image_encoder.blocks.1.norm2.weight" in original and "image_encoder.neck.2.weight" in original
    assert "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix" in original and "prompt_encoder.point_embeddings.3.weight" in original
    assert "mask_decoder.output_hypernetworks_mlps.3.layers.2.bias" in original and "mask_decoder.output_upscaling.3.weight" in original
    assert "mask_decoder.transformer.norm_final_attn.weight" in original and "mask_decoder.iou_prediction_head.layers.1.weight" in original
    assert "prompt_encoder.mask_downscaling.6.weight" in original
    assert not any(k.startswith("vision_encoder.") or ".layer_norm" in k or "proj_in" in k for k in original)
    back = sam.rename_checkpoint(original)
    assert set(back) == set(sd)
    # (the original stores the Gaussian matrix once: both transformers copies come from it)
    cfg = sam.SamConfig(num_heads=2, window_size=5, global_attn_indexes=(1,), decoder_heads=2)
    a = sam.SamModel(sd, cfg, device="cpu")
    b = sam.SamModel.from_checkpoint(original, device="cpu", config=cfg)
    assert set(a.h) == set(b.h) and set(a.f) == set(b.f)
    for k in a.h:
        assert torch.equal(a.h[k], b.h[k]), k
    for k in a.f:
        assert torch.equal(a.f[k], b.f[k]), k
    with pytest.raises(ValueError):
        sam.SamConfig.for_model_type("vit_x")
    assert sam.SamConfig.for_model_type("vit_h").global_attn_indexes == (7, 15, 23, 31)


def test_from_pretrained_reads_a_directory_transformers_wrote(tmp_path):
    """transformers ties the prompt encoder's Gaussian matrix to `shared_image_embedding` and stores the latter only: a saved directory has
    one of the two names, and `from_pretrained` must still pack what the full state dict packs."""
    transformers = pytest.importorskip("transformers")
    from blobctrl_amd.checkpoint import _model_file, read_safetensors
    cfg, sd = sc.TINY_B, sc.weights_of(sc.TINY_B)
    C = cfg["out_channels"]
    vc = transformers.SamVisionConfig(hidden_size=cfg["hidden"], output_channels=C, num_hidden_layers=cfg["layers"],
                                      num_attention_heads=cfg["heads"], image_size=cfg["image"], patch_size=cfg["patch"],
                                      window_size=cfg["window"], global_attn_indexes=list(cfg["global_attn_indexes"]), mlp_dim=cfg["mlp_dim"],
                                      num_pos_feats=C // 2)
    pc = transformers.SamPromptEncoderConfig(hidden_size=C, image_size=cfg["image"], patch_size=cfg["patch"], mask_input_channels=16)
    mc = transformers.SamMaskDecoderConfig(hidden_size=C, num_hidden_layers=cfg["decoder_layers"], num_attention_heads=sc.DECODER_HEADS,
                                           mlp_dim=cfg["decoder_mlp_dim"], iou_head_hidden_dim=cfg["iou_head_hidden_dim"])
    hf = transformers.SamModel(transformers.SamConfig(vision_config=vc, prompt_encoder_config=pc, mask_decoder_config=mc))
    hf.load_state_dict(sd, strict=True)
    hf.save_pretrained(str(tmp_path))
    stored = read_safetensors(_model_file(str(tmp_path)))
    assert "shared_image_embedding.positional_embedding" in stored
    assert "prompt_encoder.shared_embedding.positional_embedding" not in stored        # (what makes this test worth having)
    a = sam.SamModel.from_pretrained(str(tmp_path), device="cpu")
    b = sam.SamModel(sd, sam.SamConfig(num_heads=2, window_size=5, global_attn_indexes=(1,), decoder_heads=2), device="cpu")
    assert (a.config.num_heads, a.config.window_size, a.config.global_attn_indexes, a.config.decoder_heads) == (2, 5, (1,), 2)
    assert set(a.h) == set(b.h) and set(a.f) == set(b.f)
    for k in a.h:
        assert torch.equal(a.h[k], b.h[k]), k
    for k in a.f:
        assert torch.equal(a.f[k], b.f[k]), k
    # and the other way round: a state dict that has only the prompt encoder's copy
    only = {k: v for k, v in sd.items() if k != "shared_image_embedding.positional_embedding"}
    c = sam.SamModel(only, b.config, device="cpu")
    assert torch.equal(c.h["image_pe"], b.h["image_pe"])


def test_predictor_preprocessing_matches_the_fixture(gold):
    resized, x = sam.preprocess_image(gold["predictor_pre_image"], 64)
    assert resized.dtype == np.uint8 and np.array_equal(resized, gold["predictor_pre_resized"])
    assert tuple(x.shape) == (1, 3, 64, 64) and float((x - torch.from_numpy(gold["predictor_pre_tensor"])).abs().max()) <= 1e-6
    assert float(x[..., :, 48:].abs().max()) == 0.0
    bgr, _ = sam.preprocess_image(gold["predictor_pre_image"][..., ::-1], 64, "BGR")
    assert np.array_equal(bgr, resized)
    with pytest.raises(ValueError):
        sam.preprocess_image(gold["predictor_pre_image"].astype(np.float32), 64)
    with pytest.raises(ValueError):
        sam.preprocess_image(gold["predictor_pre_image"], 64, "HSV")


def test_point_scaling_and_shapes():
    assert sam.preprocess_shape(200, 150, 1024) == (1024, 768) and sam.preprocess_shape(150, 200, 256) == (192, 256)
    assert sam.preprocess_shape(1365, 2048, 1024) == (683, 1024)
    p = sam.scale_points([[75.0, 100.0], [0.0, 199.0]], (200, 150), 1024)
    assert p.dtype == np.float32 and np.allclose(p, [[384.0, 512.0], [0.0, 199.0 * 1024 / 200]])
    p = sam.scale_points([[100.0, 75.0]], (150, 200), 256)
    assert np.allclose(p, [[128.0, 96.0]])


def test_window_geometry():
    assert sam.window_geometry(64, 14) == (70, 5) and sam.window_geometry(16, 7) == (21, 3) and sam.window_geometry(12, 5) == (15, 3)
    assert sam.window_geometry(14, 14) == (14, 1)
    t = torch.arange(13 * 4, dtype=torch.float32).reshape(13, 4)
    assert sam.resize_rel_pos(t, 7) is t
    r = sam.resize_rel_pos(t, 14)
    assert r.shape == (27, 4) and torch.allclose(r, torch.nn.functional.interpolate(t.t()[None], size=27, mode="linear")[0].t())


def test_refusals_and_the_abi_table():
    sd = sc.weights_of(sc.TINY_B)
    cfg = sam.SamConfig(num_heads=2, window_size=5, global_attn_indexes=(1,), decoder_heads=2)
    model = sam.SamModel(sd, cfg, device="cpu")
    assert (model.D, model.C, model.grid, model.image_size, model.L, model.ntok) == (128, 32, 12, 192, 2, 5)
    with pytest.raises(_lib.BlobCtrlHipError):
        model.encode(torch.zeros(1, 3, 192, 192))
    pred = sam.SamPredictor(model)
    with pytest.raises(RuntimeError):
        pred.predict(np.array([[1.0, 2.0]]), np.array([1]))
    pred.is_image_set, pred.original_size, pred.input_size = True, (150, 200), (144, 192)
    with pytest.raises(NotImplementedError, match="box"):
        pred.predict(np.array([[1.0, 2.0]]), np.array([1]), box=np.array([0, 0, 5, 5]))
    with pytest.raises(NotImplementedError, match="mask_input"):
        pred.predict(np.array([[1.0, 2.0]]), np.array([1]), mask_input=np.zeros((1, 48, 48)))
    with pytest.raises(_lib.BlobCtrlHipError):
        sam.SamModel(sc.weights_of(dict(sc.TINY_B, heads=4)), sam.SamConfig(num_heads=4, window_size=5, global_attn_indexes=(1,)), device="cpu")
    # the entry points: declared in their own header, bound in their own table, recordable, checked before anything is launched
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(GOLD), "..", "..", "include", "blobctrl_sam.h")).read()
    assert set(_lib.SAM_OPS) == set(_lib.SAM_SIGNATURES) and not set(_lib.SAM_OPS) & (set(_lib.OPS) | set(_lib.REQUEST_OPS))
    assert sorted(_lib.SAM_OPS.values()) == list(range(42, 51)) and not set(_lib.SAM_SIGNATURES) & set(_lib.EXPORTED_SYMBOLS)
    for name in _lib.SAM_OPS:
        assert getattr(lib, name) is not None and f"int {name}(" in header and _lib.op_code(name) == _lib.SAM_OPS[name]
    assert _lib.op_signature("bc_attention_relpos") == "pppp" + "i" * 11 + "llllf" + "ppp" and _lib.op_signature("bc_act_rows") == "pli"
    p = 4096
    assert lib.bc_attention_relpos(p, p, p, p, 1, 2, 80, 7, 7, 7, 8, 320, 320, 64, 160, 0, 0, 0, 0, 0.1, p, p, p, None) == 1
    assert b"key grid" in lib.bc_last_error()
    assert lib.bc_attention_relpos(p, p, p, p, 1, 2, 32, 7, 7, 7, 7, 128, 128, 64, 64, 0, 0, 0, 0, 0.1, p, p, p, None) == 1 and b"head_dim" in lib.bc_last_error()
    assert lib.bc_attention_relpos(p, p, p, p, 1, 2, 80, 7, 7, 7, 7, 320, 320, 48, 160, 0, 0, 0, 0, 0.1, p, p, p, None) == 1 and b"ldvt" in lib.bc_last_error()
    assert lib.bc_window_partition(p, 1, 16, 16, 36, 7, p, None) == 1 and lib.bc_window_unpartition(p, None, 1, 16, 16, 40, 7, p, None) == 1
    assert lib.bc_bilinear_resize_f32(p, 1, 64, 64, 65, 64, 8, 8, 0, 0.0, p, None) == 1 and b"crop" in lib.bc_last_error()
    assert lib.bc_sam_masks(p, 8, p, 4, 1, 4, 4, 4, p, None) == 1 and lib.bc_act_rows(p, 12, 0, None) == 1 and lib.bc_add_rows(p, p, 7, 2, 8, p, None) == 1


def test_sam_launches_are_never_written_to_a_plan_file(tmp_path):
    """SAM segments are in-process only: `bc_plan_save` refuses a plan that holds one of these launches (and the file reader admits no
    version that has them), while a plan without them is saved as before."""
    from blobctrl_amd.launch import Recorder
    rec = Recorder(torch.device("cpu"))
    rec.begin("seg")
    buf = torch.zeros(16, dtype=torch.float16)
    rec.call("bc_silu", buf, buf, 16, kind="silu", keep=buf)
    path = str(tmp_path / "ok.bcplan")
    rec.save(path)
    assert os.path.getsize(path) > 0
    rec.call("bc_act_rows", buf, 16, 1, kind="relu", keep=buf)
    with pytest.raises(_lib.BlobCtrlHipError, match="in-process only"):
        rec.save(str(tmp_path / "sam.bcplan"))
    assert not os.path.exists(str(tmp_path / "sam.bcplan"))
    rec.close()
