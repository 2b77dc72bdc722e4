"""The CLIP vision tower (blobctrl_amd/clip_vision.py) on the GPU against transformers' CLIPVisionModelWithProjection
(tests/golden/clip_vision_tiny.npz): image_embeds and hidden_states[-2] for a seeded and for an all-zero input, at the bar
tests/test_clip_text_gpu.py holds the text tower to; one plan per shape, replayed."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import clip_vision_common as cv  # noqa: E402


def _close(a, b, tol=1e-2, db=40.0):
    """The bar of tests/test_clip_text_gpu.py: max-abs over the reference's scale under 1e-2 and PSNR over 40 dB."""
    from tests.common import psnr
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-6)
    assert err < tol and psnr(a, b) > db, f"max-abs/scale {err:.3e}, PSNR {psnr(a, b):.1f} dB"
    return err


@pytest.mark.parametrize("name", sorted(cv.CLIP_VISION_CONFIGS))
def test_clip_vision_matches_transformers(golden_dir, name):
    from blobctrl_amd.clip_vision import CLIPVisionModelWithProjection
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    z = np.load(os.path.join(golden_dir, "clip_vision_tiny.npz"))
    c = cv.CLIP_VISION_CONFIGS[name]
    model = CLIPVisionModelWithProjection(cv.clip_vision_weights(name), num_heads=c["num_attention_heads"], patch_size=c["patch_size"],
                                          image_size=c["image_size"], hidden_act=c["hidden_act"])
    px = cv.clip_vision_pixels(name)
    for tag, x in (("", px), ("_zero", torch.zeros_like(px))):
        out = model(x, output_hidden_states=True)
        assert len(out.hidden_states) == c["num_hidden_layers"] + 1
        for what, got, ref in (("image_embeds", out.image_embeds, z[f"{name}_image_embeds{tag}"]), ("hidden_states[-2]", out.hidden_states[-2], z[f"{name}_hidden{tag}"])):
            got = got.float().cpu().numpy()
            assert got.shape == ref.shape
            print(f"clip vision {name}{tag} {what}: max-abs/scale {_close(got, ref):.3e}")
    assert len(model._plans) == 1 and model.replays == 2                      # one plan for the shape, two replays
    plain = model(px)
    assert plain.hidden_states is None
    _close(plain.image_embeds.float().cpu().numpy(), z[f"{name}_image_embeds"])
    with pytest.raises(ValueError, match="position embedding"):
        model(torch.zeros(1, 3, c["image_size"] + c["patch_size"], c["image_size"]))


@pytest.mark.parametrize("size", cv.CLIP_PROCESSOR_SIZES)
def test_clip_pixel_values_on_the_device_are_the_host_processors(golden_dir, size):
    """resample.clip_pixel_values on uint8 device images: bit-identical to the host CLIPImageProcessor - and with it to transformers'
    (tests/golden/clip_processor.npz) - on the three fixture images."""
    from blobctrl_amd import resample
    from blobctrl_amd.image_processor import CLIPImageProcessor
    z = np.load(os.path.join(golden_dir, "clip_processor.npz"))
    proc = CLIPImageProcessor(size, size)
    for image in sorted(cv.CLIP_PROCESSOR_IMAGES):
        arr = cv.clip_processor_image(image)
        got = resample.clip_pixel_values(torch.from_numpy(arr).to("cuda:0"), proc)
        host = proc(images=arr).pixel_values
        assert got.dtype == torch.float32 and got.device.type == "cuda" and tuple(got.shape) == (1, 3, size, size)
        assert torch.equal(got.cpu(), host) and np.array_equal(got[0].cpu().numpy(), z[f"{image}_{size}"]), (image, size)
    with pytest.raises(Exception, match="clip_pixel_values"):
        resample.clip_pixel_values(torch.zeros(8, 8, 3, dtype=torch.uint8), proc)              # a host tensor: no CPU fallback


# ---------------------------------------------------------------------------------------------------- __call__ with ip_adapter_image
def _tiny_pipeline(**extra):
    from blobctrl_amd.clip_text import CLIPTextModel
    from blobctrl_amd.dinov2 import Dinov2Model
    from blobctrl_amd.modules import BlobNetModel, UNet2DConditionModel
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    from blobctrl_amd.schedulers import DDIMScheduler
    from blobctrl_amd.vae import AutoencoderKL
    from tests.common import PIPE, FakeTokenizer, tiny_pipeline_weights, tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    from tests.test_freeu_gpu import SD
    vsd, csd, dsd = tiny_pipeline_weights()
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    return StableDiffusionBlobNetPipeline(
        tokenizer=FakeTokenizer(), scheduler=DDIMScheduler(**SD), safety_checker=None, requires_safety_checker=False,
        unet=UNet2DConditionModel(usd, ucfg), blobnet=BlobNetModel(bsd, bcfg), vae=AutoencoderKL(vsd, norm_num_groups=PIPE["vae_groups"]),
        text_encoder=CLIPTextModel(csd, num_heads=PIPE["clip"]["heads"]),
        dinov2=Dinov2Model(dsd, num_heads=PIPE["dino"]["heads"], patch_size=PIPE["dino"]["patch"]), **extra)


@pytest.mark.parametrize("kind", ("plus", "base"))
def test_pipeline_call_with_an_image_prompt_matches_the_reference_call(golden_dir, tmp_path, kind):
    """The reference's own `__call__` with `ip_adapter_image=<PIL image>` (tests/golden/pipeline_call_ip_image.npz: classifier-free guidance,
    two images per prompt, DDIM, 3 steps) with the adapter and the tower loaded from a folder by load_ip_adapter, at the bar of
    tests/test_ip_adapter_gpu.py's pipeline case.  A different image gives the other golden on the same plan; the device route (a uint8
    image on the GPU) gives the host route's latents bit for bit; the all-zero branch of a Plus adapter runs the tower once; after
    unload_ip_adapter the latents are bit-identical to those of a pipeline that never loaded one."""
    import json
    from PIL import Image
    from blobctrl_amd.checkpoint import write_safetensors
    from blobctrl_amd.image_processor import CLIPImageProcessor
    from tests import ip_adapter_common as ip
    from tests.common import pipeline_cases, psnr
    z = np.load(os.path.join(golden_dir, "pipeline_call.npz"))
    zi = np.load(os.path.join(golden_dir, "pipeline_call_ip_image.npz"))
    rel_err = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    kw = dict(pipeline_cases()["ddim_neg2"])
    for k in ("scheduler", "seed", "rng_seed", "num_inference_steps"):
        kw.pop(k)
    seed, rng_seed, steps = int(zi["seed"]), int(zi["rng_seed"]), int(zi["num_inference_steps"])
    assert (seed, rng_seed) == cv.IP_IMAGE_CALL_SEEDS
    common = dict(fg_image=Image.fromarray(z["fg"]), bg_image=Image.fromarray(z["bg"]), gs_score=torch.from_numpy(z["gs_score"]),
                  height=64, width=64, output_type="latent", num_inference_steps=steps, **kw)

    def call(p, **extra):
        torch.manual_seed(rng_seed)
        return p(generator=torch.Generator().manual_seed(seed), **common, **extra).images.cpu().numpy()
    # the adapter file and the encoder folder, as a local IP-Adapter repository lays them out
    c = cv.CLIP_VISION_CONFIGS["a"]
    enc_dir = tmp_path / "models" / "image_encoder"
    enc_dir.mkdir(parents=True)
    write_safetensors(str(enc_dir / "model.safetensors"), cv.clip_vision_weights("a"))
    (enc_dir / "config.json").write_text(json.dumps(c))
    sd = cv.tiny_plus_adapter("q16") if kind == "plus" else ip.tiny_ip_adapter(0)
    write_safetensors(str(tmp_path / "models" / "adapter.safetensors"), {f"{part}.{k}": v.contiguous() for part in sd for k, v in sd[part].items()})
    arrays = {k: cv.clip_processor_image(v) for k, v in cv.IP_IMAGE_CALL_IMAGES.items()}

    plain = call(_tiny_pipeline())
    pipe = _tiny_pipeline()
    pipe.load_ip_adapter(str(tmp_path), subfolder="models", weight_name="adapter.safetensors", image_encoder_folder="image_encoder")
    enc = pipe.image_encoder
    assert enc is not None and isinstance(pipe.feature_extractor, CLIPImageProcessor) and pipe.feature_extractor.crop_size == c["image_size"]
    got = call(pipe, ip_adapter_image=Image.fromarray(arrays["a"]))
    ref = zi[f"{kind}_latents"]
    print(f"__call__ ip image {kind}: max-abs/scale {rel_err(got, ref):.3e}, PSNR {psnr(got, ref):.1f} dB; reference on vs off {rel_err(ref, zi['latents_off']):.3f}")
    assert got.shape == ref.shape and rel_err(got, ref) < 1e-2 and psnr(got, ref) > 40.0
    eng = pipe.engine
    want_key = ("ip", 1, (16, cv.PLUS_EMBED, 10)) if kind == "plus" else ("ip", 1, (4, ip.IP_EMBED_DIM))
    assert list(eng._plans)[-1][-1] == want_key and enc.replays == (2 if kind == "plus" else 1)       # the image, and once the zero image
    # another image: the other golden, a plan hit, and no second pass over the zero image
    st = dict(eng.cache_stats)
    got_b, ref_b = call(pipe, ip_adapter_image=[Image.fromarray(arrays["b"])]), zi[f"{kind}_latents_b"]
    print(f"__call__ ip image {kind}, image B: max-abs/scale {rel_err(got_b, ref_b):.3e}; vs image A {rel_err(got_b, got):.3f}")
    assert rel_err(got_b, ref_b) < 1e-2 and psnr(got_b, ref_b) > 40.0 and rel_err(got_b, got) > 0.1
    assert eng.cache_stats["plans_recorded"] == st["plans_recorded"] and eng.cache_stats["plan_hits"] == st["plan_hits"] + 1
    assert enc.replays == (3 if kind == "plus" else 2) and len(enc._plans) == 1
    # the device route: the same pixels without a host copy, so the same latents bit for bit
    before = enc.replays
    assert np.array_equal(call(pipe, ip_adapter_image=torch.from_numpy(arrays["a"]).to("cuda:0")), got) and enc.replays == before + 1
    # float pixel values are taken as they are
    px = pipe.feature_extractor(Image.fromarray(arrays["a"]), return_tensors="pt").pixel_values
    assert np.array_equal(call(pipe, ip_adapter_image=px), got)
    with pytest.raises(ValueError, match="must have same length as the number of IP Adapters"):
        call(pipe, ip_adapter_image=[Image.fromarray(arrays["a"])] * 2)
    # unload: the encoder that load_ip_adapter loaded goes too; bit-identical to a pipeline that never loaded one, and the reference's
    pipe.unload_ip_adapter()
    assert pipe.image_encoder is None and pipe.feature_extractor is None
    off = call(pipe)
    assert np.array_equal(off, plain) and rel_err(off, zi["latents_off"]) < 1e-2 and psnr(off, zi["latents_off"]) > 40.0
    with pytest.raises(NotImplementedError, match="ip_adapter_image_embeds"):
        call(pipe, ip_adapter_image=Image.fromarray(arrays["a"]))
