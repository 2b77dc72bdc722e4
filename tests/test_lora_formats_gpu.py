"""GPU twin of tests/test_lora_formats_cpu.py: a kohya / sd-scripts adapter file gives the bits of its diffusers form, text-encoder LoRA
reaches the embeddings (also through a plan recorded before the adapter was loaded), and `cross_attention_kwargs={"scale": s}` is the
adapter weight s for one call, in the UNet and in the text encoder."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.common import PIPE, g, psnr, write_model_tree  # noqa: E402
from tests.test_clip_text_gpu import _close  # noqa: E402
from tests.test_lora_formats_cpu import RANK, diffusers_form, te_adapter, write_adapter_dirs  # noqa: E402
from tests.test_pipeline_construct_cpu import construct_pipeline  # noqa: E402

PROMPT, NEGATIVE = "a frog sits on a rock in a pond", "blurry, low quality"


def _edit(pipe, **kw):
    """One seeded 2-step edit of a 64 x 64 image -> the final latents."""
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(3))
    fg = Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8))
    bg = Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8))
    score = torch.rand(1, 1, 8, 8, generator=torch.Generator().manual_seed(1))
    score = torch.cat([1 - score, score], 1)
    torch.manual_seed(17)                                   # VAE posterior samples come from the global generator (pipe:304)
    if "prompt_embeds" not in kw:
        kw = dict(kw, prompt=PROMPT, negative_prompt=NEGATIVE)
    out = pipe(fg_image=fg, bg_image=bg, gs_score=score, height=64, width=64, num_inference_steps=2, guidance_scale=7.5,
               generator=torch.Generator().manual_seed(5), output_type="latent", **kw).images.cpu()
    assert out.shape == (1, 4, 8, 8) and bool(torch.isfinite(out).all())
    return out


def test_kohya_file_gives_the_bits_of_its_diffusers_form(tmp_path):
    paths, pieces = write_model_tree(tmp_path)
    d, k = write_adapter_dirs(tmp_path, pieces)
    first, again = construct_pipeline(dict(paths, unet_lora=d), "cuda:0"), construct_pipeline(dict(paths, unet_lora=d), "cuda:0")
    a, b = _edit(first), _edit(again)
    # two builds from the same file repeat bit for bit: a difference below is the kohya path's, not the engine's
    assert torch.equal(first.unet.packed_fp16, again.unet.packed_fp16) and torch.equal(first.unet.packed_fp32, again.unet.packed_fp32)
    assert torch.equal(a, b)
    del again
    kohya = construct_pipeline(dict(paths, unet_lora=k), "cuda:0")
    assert kohya.get_list_adapters() == {"unet": ["default"], "text_encoder": ["default"]}
    assert torch.equal(kohya.unet.packed_fp16, first.unet.packed_fp16) and torch.equal(kohya.unet.packed_fp32, first.unet.packed_fp32)
    assert torch.equal(_edit(kohya), a)
    assert all(torch.equal(v, first.text_encoder.h[n]) for n, v in kohya.text_encoder.h.items())     # (filled when the prompt was encoded)
    # and the adapter is not a no-op
    plain = construct_pipeline(paths, "cuda:0")
    assert not torch.equal(plain.unet.packed_fp16, first.unet.packed_fp16) and not torch.equal(_edit(plain), a)


def test_text_encoder_lora_reaches_the_embeddings(tmp_path):
    from oracle.clip_text import clip_text_hidden
    paths, pieces = write_model_tree(tmp_path)
    csd, heads = pieces["clip"], PIPE["clip"]["heads"]
    adapter = te_adapter()            # sized on the CPU: the smallest of 0.1 / 0.2 / 0.4 that meets the oracle-vs-oracle fact below with room
    merged = dict(csd)
    for m, a, b, alpha in adapter:
        alpha = float(RANK) if alpha is None else alpha
        merged[m + ".weight"] = (csd[m + ".weight"].double() + (alpha / RANK) * (b.double() @ a.double())).float()
    pipe = construct_pipeline(paths, "cuda:0")               # (its own adapter has UNet tensors only)
    ids = pipe._tokenize(PROMPT, 77)
    ref_base, ref_lora = clip_text_hidden(csd, ids, heads).numpy(), clip_text_hidden(merged, ids, heads).numpy()
    # the adapter moves the oracle by 10 x the bar of `_close` (max-abs / scale 1e-2, 40 dB): a loader that drops it cannot pass
    moved = np.abs(ref_lora - ref_base).max() / np.abs(ref_base).max()
    print(f"oracle(merged) vs oracle(base): max-abs/scale {moved:.3e}, PSNR {psnr(ref_lora, ref_base):.1f} dB")
    assert moved >= 1e-1 and psnr(ref_lora, ref_base) <= 20.0
    encode = lambda **kw: pipe.encode_prompt(PROMPT, pipe.device, 1, False, **kw)[0].float().cpu().numpy()
    _close(encode()[0], ref_base[0])
    plans = dict(pipe.text_encoder._plans)
    assert len(plans) == 1
    pipe.load_lora_weights(diffusers_form(adapter, "text_encoder."), adapter_name="te")
    assert pipe.get_list_adapters() == {"unet": ["default"], "text_encoder": ["te"]}
    e = _close(encode()[0], ref_lora[0])
    print(f"encode_prompt with the adapter vs oracle(merged): max-abs/scale {e:.3e}")
    assert pipe.text_encoder._plans == plans                 # the plan recorded before the adapter was loaded gave the new embeddings
    # lora_scale of encode_prompt: 0 is the base model, and the next call without it is the adapter again
    _close(encode(lora_scale=0.0)[0], ref_base[0])
    _close(encode()[0], ref_lora[0])
    pipe.unload_lora_weights()
    _close(encode()[0], ref_base[0])


def test_cross_attention_kwargs_scale_is_the_adapter_weight_for_one_call(tmp_path):
    paths, pieces = write_model_tree(tmp_path)
    _, k = write_adapter_dirs(tmp_path, pieces)
    pipe, half = construct_pipeline(dict(paths, unet_lora=k), "cuda:0"), construct_pipeline(dict(paths, unet_lora=k), "cuda:0")
    half.set_adapters(["default"], [0.5])                    # UNet and text encoder
    assert half.unet._adapters["default"]["weight"] == half.text_encoder._adapters["default"]["weight"] == 0.5
    full = _edit(pipe)
    want = _edit(half)
    assert not torch.equal(want, full)
    v = pipe.unet._version
    assert torch.equal(_edit(pipe, cross_attention_kwargs={"scale": 0.5}), want)
    assert pipe.unet._version == v + 1
    assert torch.equal(pipe.unet.packed_fp16, half.unet.packed_fp16)              # lazy: the packed copy stays at 0.5 ...
    assert torch.equal(_edit(pipe), full)                                         # ... and the next call without the argument re-packs at 1.0
    assert pipe.unet._version == v + 2
    # with prompt_embeds the text encoder is not touched
    emb, neg = pipe.encode_prompt(PROMPT, pipe.device, 1, True, NEGATIVE)
    te = pipe.text_encoder
    before, filled = {n: t.clone() for n, t in te.h.items()}, te._filled
    scaled = _edit(pipe, prompt_embeds=emb, negative_prompt_embeds=neg, cross_attention_kwargs={"scale": 0.5})
    assert te._filled == filled and all(torch.equal(t, before[n]) for n, t in te.h.items())
    assert not torch.equal(scaled, full) and not torch.equal(scaled, want)        # UNet at 0.5, embeddings at 1.0
    # no adapter: the argument is a no-op and nothing is re-packed
    pipe.unload_lora_weights()
    plain = _edit(pipe)
    v = pipe.unet._version
    assert torch.equal(_edit(pipe, cross_attention_kwargs={"scale": 0.5}), plain)
    assert pipe.unet._version == v
    # the UNet shell's forward honours the argument the same way
    x, ctx = g(41, 1, 5, 8, 8).cuda(), g(42, 1, 7, 16).cuda()
    at_half = half.unet(x, 500, ctx, return_dict=False)[0]
    one = construct_pipeline(dict(paths, unet_lora=k), "cuda:0").unet
    assert torch.equal(one(x, 500, ctx, cross_attention_kwargs={"scale": 0.5}, return_dict=False)[0], at_half)
    assert not torch.equal(one(x, 500, ctx, return_dict=False)[0], at_half)
