"""The CLIP vision tower without a GPU: a float64 restatement (tests/clip_vision_common.py) against transformers'
CLIPVisionModelWithProjection (tests/golden/clip_vision_tiny.npz) - which pins the key names, hidden_states[-2], the bias-free patch
convolution and projection and both activations -, construction from a state dict with and without the `vision_model.` prefix,
from_pretrained from a local folder, and the refusal to run without a device."""
import json
import os

import numpy as np
import pytest
import torch

from tests import clip_vision_common as cv


@pytest.fixture(scope="module")
def zc(golden_dir):
    return np.load(os.path.join(golden_dir, "clip_vision_tiny.npz"))


@pytest.mark.parametrize("name", sorted(cv.CLIP_VISION_CONFIGS))
def test_float64_tower_reproduces_transformers(zc, name):
    sd = cv.clip_vision_weights(name)
    px = cv.clip_vision_pixels(name)
    for tag, x in (("", px), ("_zero", torch.zeros_like(px))):
        emb, hid = cv.clip_vision64(name, sd, x)
        for what, got, ref in (("image_embeds", emb.numpy(), zc[f"{name}_image_embeds{tag}"]), ("hidden_states[-2]", hid.numpy(), zc[f"{name}_hidden{tag}"])):
            err = float(np.abs(got - ref).max() / np.abs(ref).max())
            print(f"clip_vision64 {name}{tag} {what}: max-abs / scale {err:.2e}")
            assert got.shape == ref.shape and err < 2e-5                                        # the reference is fp32
    c = cv.CLIP_VISION_CONFIGS[name]
    n = (c["image_size"] // c["patch_size"]) ** 2 + 1
    assert zc[f"{name}_hidden"].shape == (cv.CLIP_VISION_BATCH, n, c["hidden_size"]) and zc[f"{name}_image_embeds"].shape == (2, c["projection_dim"])
    assert not any(k.endswith("patch_embedding.bias") or k == "visual_projection.bias" for k in sd) and "vision_model.pre_layrnorm.weight" in sd


@pytest.mark.parametrize("name", sorted(cv.CLIP_VISION_CONFIGS))
def test_construction_with_and_without_the_prefix_and_from_a_folder(tmp_path, name):
    from blobctrl_amd import _lib
    from blobctrl_amd.checkpoint import write_safetensors
    from blobctrl_amd.clip_vision import CLIPVisionModelWithProjection
    c = cv.CLIP_VISION_CONFIGS[name]
    kw = dict(num_heads=c["num_attention_heads"], patch_size=c["patch_size"], image_size=c["image_size"], hidden_act=c["hidden_act"], device="cpu")
    a = CLIPVisionModelWithProjection(cv.clip_vision_weights(name), **kw)
    bare = {k[len("vision_model."):] if k.startswith("vision_model.") else k: v for k, v in cv.clip_vision_weights(name).items()}
    assert "pre_layrnorm.weight" in bare and "visual_projection.weight" in bare
    b = CLIPVisionModelWithProjection(bare, **kw)
    assert set(a.h) == set(b.h) and all(a.h[k].equal(b.h[k]) for k in a.h) and all(a.f[k].equal(b.f[k]) for k in a.f)
    assert a.L == c["num_hidden_layers"] and a.D == c["hidden_size"] and a.P == c["projection_dim"] and a.config.image_size == c["image_size"]
    assert a.dtype == torch.float16 and next(a.parameters()).dtype == torch.float16 and tuple(a.h["proj.weight"].shape) == (c["projection_dim"], c["hidden_size"])
    assert a.h["patch.weight"].shape[1] % 8 == 0 and a.h["patch.weight"].shape[1] >= 3 * c["patch_size"] ** 2
    d = tmp_path / "image_encoder"
    d.mkdir()
    write_safetensors(str(d / "model.safetensors"), cv.clip_vision_weights(name))
    (d / "config.json").write_text(json.dumps(dict(c, layer_norm_eps=1e-5)))
    f = CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), subfolder="image_encoder", device="cpu")
    assert f.act == a.act and f.heads == a.heads and f.config.image_size == c["image_size"] and all(f.h[k].equal(a.h[k]) for k in a.h)
    assert {"gelu": _lib.ACT_GELU, "quick_gelu": _lib.ACT_QUICK_GELU}[c["hidden_act"]] == a.act
    with pytest.raises(_lib.BlobCtrlHipError, match="no CPU fallback"):
        a(torch.zeros(1, 3, c["image_size"], c["image_size"]))
    with pytest.raises(ValueError, match="hidden_act"):
        CLIPVisionModelWithProjection(cv.clip_vision_weights(name), **dict(kw, hidden_act="relu"))


# ---------------------------------------------------------------------------------------------------- the image processor
@pytest.fixture(scope="module")
def zpx(golden_dir):
    return np.load(os.path.join(golden_dir, "clip_processor.npz"))


@pytest.mark.parametrize("size", cv.CLIP_PROCESSOR_SIZES)
@pytest.mark.parametrize("image", sorted(cv.CLIP_PROCESSOR_IMAGES))
def test_host_processor_equals_transformers_exactly(zpx, image, size):
    """blobctrl_amd.image_processor.CLIPImageProcessor against the installed transformers one (Pillow backend), every bit; `size` as a bare
    int and as {"shortest_edge": n}; and resample's table route (resize_reference + the processor's look-up table) gives the same pixels."""
    from PIL import Image
    from blobctrl_amd import resample
    from blobctrl_amd.image_processor import CLIPImageProcessor
    arr, ref = cv.clip_processor_image(image), zpx[f"{image}_{size}"]
    for proc in (CLIPImageProcessor(size, size), CLIPImageProcessor({"shortest_edge": size}, {"height": size, "width": size})):
        for src in (arr, Image.fromarray(arr)):
            got = proc(images=src, return_tensors="pt").pixel_values
            assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, size, size) and np.array_equal(got[0].numpy(), ref)
    proc = CLIPImageProcessor(size, size)
    (nh, nw), (top, left, ch, cw) = resample.dinov2_geometry(arr.shape[0], arr.shape[1], proc.shortest_edge, proc.crop_size)
    resized = resample.resize_reference(arr, (nh, nw), "bicubic")[top:top + ch, left:left + cw]
    lut = resample.clip_lut(proc)
    table = np.stack([lut[c][resized[..., c]] for c in range(3)], 0)
    assert lut.shape == (3, 256) and lut.dtype == np.float32 and np.array_equal(table, ref)


def test_processor_from_pretrained_reads_both_shapes_of_size(tmp_path):
    from blobctrl_amd.image_processor import CLIP_MEAN, CLIP_STD, CLIPImageProcessor
    for i, (size, crop) in enumerate(((224, 224), ({"shortest_edge": 56}, {"height": 56, "width": 56}))):
        d = tmp_path / str(i)
        d.mkdir()
        (d / "preprocessor_config.json").write_text(json.dumps(dict(size=size, crop_size=crop, image_mean=list(CLIP_MEAN), image_std=list(CLIP_STD),
                                                                    do_resize=True, do_center_crop=True, resample=3)))
        p = CLIPImageProcessor.from_pretrained(str(d))
        want = size if isinstance(size, int) else 56
        assert (p.shortest_edge, p.crop_size) == (want, want) and p.size == {"shortest_edge": want} and p.image_mean == CLIP_MEAN
    with pytest.raises(ValueError, match="square"):
        CLIPImageProcessor(224, {"height": 224, "width": 200})


# ---------------------------------------------------------------------------------------------------- the pipeline surface, host side
def _stub(adapters=()):
    import types
    from blobctrl_amd.modules import UNet2DConditionModel
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline as Pipe
    from tests.common import tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    unet = UNet2DConditionModel(tiny_weights()[0], tiny_trunk_configs()[0], device="cpu", lazy=True)
    if adapters:
        unet.load_ip_adapter_weights(list(adapters))
    stub = types.SimpleNamespace(unet=unet, _engine=None, device=torch.device("cpu"), image_encoder=None, feature_extractor=None,
                                 _loaded_image_encoder=False, _zero_image_states={}, _callback_tensor_inputs=["latents"])
    for name in ("load_ip_adapter", "unload_ip_adapter", "encode_image", "prepare_ip_adapter_image_embeds", "check_inputs"):
        setattr(stub, name, types.MethodType(getattr(Pipe, name), stub))
    return stub


def test_load_ip_adapter_with_a_folder_and_a_dict_source_raises_the_references_error():
    from tests import ip_adapter_common as ip
    stub = _stub()
    with pytest.raises(ValueError, match="`image_encoder` cannot be loaded because `pretrained_model_name_or_path_or_dict` is a state dict."):
        stub.load_ip_adapter(ip.tiny_ip_adapter(0), image_encoder_folder="image_encoder")
    assert not stub.unet.ip_adapters and stub.image_encoder is None                      # refused before anything was loaded
    stub.load_ip_adapter(ip.tiny_ip_adapter(0))                                          # the default: no folder, nothing but the adapter
    assert len(stub.unet.ip_adapters) == 1 and stub.image_encoder is None and stub.feature_extractor is None


def test_load_ip_adapter_loads_the_encoder_from_a_folder_and_unload_drops_it(tmp_path):
    """A path source: path/subfolder/folder, a folder with "/" relative to path; a default processor of the encoder's image size; an
    encoder the caller registered stays through load and unload; without an encoder `ip_adapter_image` keeps today's error."""
    from blobctrl_amd.checkpoint import write_safetensors
    from blobctrl_amd.clip_vision import CLIPVisionModelWithProjection
    from blobctrl_amd.image_processor import CLIPImageProcessor
    c = cv.CLIP_VISION_CONFIGS["a"]
    sd = cv.tiny_plus_adapter("q16")
    for enc_dir in (tmp_path / "models" / "image_encoder", tmp_path / "elsewhere" / "enc"):
        enc_dir.mkdir(parents=True)
        write_safetensors(str(enc_dir / "model.safetensors"), cv.clip_vision_weights("a"))
        (enc_dir / "config.json").write_text(json.dumps(c))
    write_safetensors(str(tmp_path / "models" / "plus.safetensors"), {f"{part}.{k}": v.contiguous() for part in sd for k, v in sd[part].items()})
    for folder in ("image_encoder", "elsewhere/enc"):
        stub = _stub()
        with pytest.raises(NotImplementedError, match="ip_adapter_image_embeds"):
            stub.check_inputs(prompt="a", callback_steps=None, ip_adapter_image=object())
        stub.load_ip_adapter(str(tmp_path), subfolder="models", weight_name="plus.safetensors", image_encoder_folder=folder)
        assert isinstance(stub.image_encoder, CLIPVisionModelWithProjection) and stub.image_encoder.config.image_size == c["image_size"]
        assert isinstance(stub.feature_extractor, CLIPImageProcessor) and stub.feature_extractor.crop_size == stub.feature_extractor.shortest_edge == c["image_size"]
        assert stub.unet.ip_adapters[0]["layout"] == "plus"
        stub.check_inputs(prompt="a", callback_steps=None, ip_adapter_image=object())                 # with an encoder: proceeds
        with pytest.raises(ValueError, match="must have same length as the number of IP Adapters"):
            stub.prepare_ip_adapter_image_embeds([object(), object()], None, "cpu", 1, True)
        stub.unload_ip_adapter()
        assert stub.image_encoder is None and stub.feature_extractor is None and not stub.unet.ip_adapters
        with pytest.raises(NotImplementedError, match="ip_adapter_image_embeds"):
            stub.prepare_ip_adapter_image_embeds(object(), None, "cpu", 1, True)
    mine, proc = object(), CLIPImageProcessor(56, 56)
    stub = _stub()
    stub.image_encoder, stub.feature_extractor = mine, proc
    stub.load_ip_adapter(str(tmp_path), subfolder="models", weight_name="plus.safetensors", image_encoder_folder="image_encoder")
    stub.unload_ip_adapter()
    assert stub.image_encoder is mine and stub.feature_extractor is proc
