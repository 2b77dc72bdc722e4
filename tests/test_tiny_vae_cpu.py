"""AutoencoderTiny without a GPU: the parameter schema against the reference's, the float64 restatement the GPU tests check against tied to
the reference's outputs, the packed weights, the recorded launch list, from_pretrained, the header and op tables, and every refusal."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest
import torch

from blobctrl_amd import _lib, synth
from blobctrl_amd.tiny_vae import AutoencoderTiny
from tests import tiny_vae_common as tv

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def module():
    return AutoencoderTiny(tv.weights(), device="cpu")


def test_param_shapes_are_the_reference_decoders():
    _, _, schema = tv.fixture()
    mine = [(k, tuple(v)) for k, v in synth.tiny_vae_param_shapes().items()]
    assert mine == schema and len(mine) == 67
    assert [n for n, _, _ in tv.layer_list()] == [k[:-len(".weight")] for k, _ in schema if k.endswith(".weight")]


@pytest.mark.parametrize("tag", tv.CASES)
def test_float64_restatement_reproduces_the_reference(tag):
    """The checker of the GPU tests: `sample` to 1e-5 of max |.|, the preview bytes exactly wherever the float value is not within 1e-4 of a
    rounding boundary."""
    z, meta, _ = tv.fixture()
    sample = tv.decoder64(tv.weights(), torch.from_numpy(z[f"{tag}_z"]))
    ref = torch.from_numpy(z[f"{tag}_sample"]).double()
    err = float((sample - ref).abs().max() / ref.abs().max())
    print(f"case {tag}: float64 restatement vs reference max-abs/scale {err:.3e}")
    assert sample.shape == ref.shape and err < 1e-5
    by, dist = tv.quantise64(sample)
    want = torch.from_numpy(z[f"{tag}_preview"])
    clear = dist > 1e-4
    assert by.shape == want.shape and bool(clear.float().mean() > 0.99) and torch.equal(by[clear], want[clear])
    sat = float(((want == 0) | (want == 255)).float().mean())
    assert abs(sat - meta["cases"][tag]["saturated_bytes"]) < 1e-6 and sat > 0.05                  # both clamps are exercised
    assert bool((want == 0).any()) and (tag == "b" or bool((want == 255).any()))                   # (the 1 x 1 latent's image is dark)


def test_fixture_meta_keeps_every_layer_alive():
    _, meta, _ = tv.fixture()
    stds = meta["layer_output_std"]
    assert len(stds) == 35 and 0.25 < min(stds) and max(stds) < 1.4
    emu = [c["fp16_storage_emulation_max_abs_over_scale"] for c in meta["cases"].values()]
    print("fp16-storage emulation of the reference, max-abs/scale per case:", emu)
    assert max(emu) * 3 <= 1e-2                                        # the whole-decoder bar of the GPU test keeps a margin of at least 3x


def test_packed_weights(module):
    sd = tv.weights()
    w_in = module.h["decoder.layers.0.weight"].float().view(64, 3, 3, 8)
    assert w_in.dtype == torch.float32 and module.h["decoder.layers.0.weight"].dtype == torch.float16
    assert torch.equal(w_in[..., :4], sd["decoder.layers.0.weight"].permute(0, 2, 3, 1).half().float()) and float(w_in[..., 4:].abs().max()) == 0.0
    w_out = module.h["decoder.layers.18.weight"].float().view(8, 3, 3, 64)
    assert torch.equal(w_out[:3], sd["decoder.layers.18.weight"].permute(0, 2, 3, 1).half().float()) and float(w_out[3:].abs().max()) == 0.0
    assert module.f["decoder.layers.18.bias"].shape == (3,) and module.f["decoder.layers.18.bias"].dtype == torch.float32
    ups = [n for n, f, _ in tv.layer_list() if f == "up"]
    assert ups == ["decoder.layers.6", "decoder.layers.11", "decoder.layers.16"]
    for n, f, _ in tv.layer_list():
        assert (n + ".bias" in module.f) == (f != "up")
        if f not in ("in", "out"):
            assert module.h[n + ".weight"].shape == (64, 576)
    assert len(module.h) == 35 and len(module.f) == 32


def test_recorded_launch_list(module):
    """(2, 5, 7): the latent prologue and the 35 convolutions of the default architecture - 1 + 3 * (3 + 3 + 3 + 1) + 3 + 1 - with their forms
    and sizes, in both segments: 36 launches each."""
    P = module._plan(2, 5, 7)
    assert module._plan(2, 5, 7) is P
    want = [("tiny_latents_in", 2, 5, 7)]
    for _, form, s in tv.layer_list():
        want.append(("tiny_" + form, 2, 5 << s, 7 << s, 8 if form == "in" else 64, 3 if form == "out" else 64))
    for seg in (P.decode, P.preview):
        assert [m["shape"] for m in seg.meta] == want and len(seg) == 36
        assert module.lib.bc_plan_num_launches(P.rec.plan, seg.id) == 36
        assert [m["kind"] for m in seg.meta] == ["tiny_latents_in"] + ["tiny_conv"] * 35
        assert seg.meta[1]["variant"] == "tiny_conv3x3_kernel<8,2>" and seg.meta[-1]["variant"] == "tiny_conv3x3_kernel<64,1>"
        assert all(m["variant"] == "tiny_conv3x3_kernel<64,2>" for m in seg.meta[2:-1])
    flops = sum(m["flops"] for m in P.decode.meta)
    pix = 2 * 5 * 7
    assert flops == 2 * 9 * pix * (8 * 64 + 64 * 64 * (9 + 10 * 4 + 10 * 16 + 4 * 64) + 64 * 3 * 64)
    sizes = [m["shape"][2:4] for m in P.decode.meta[1:]]
    assert sizes.count((5, 7)) == 10 and sizes.count((10, 14)) == 10 and sizes.count((20, 28)) == 10 and sizes.count((40, 56)) == 5


def test_header_and_op_tables():
    text = open(os.path.join(HERE, "..", "include", "blobctrl_tiny_vae.h")).read()
    assert "enum { BC_OP_TINY_CONV3X3 = BC_OP_IP_MASK_END + 1, BC_OP_TINY_LATENTS_IN, BC_OP_TINY_VAE_END };" in text
    assert "int bc_tiny_conv3x3(const bc_tiny_conv_args* args, bc_stream stream);" in text
    assert "int bc_tiny_latents_in(const float* z, int B, int h, int w, bc_half* out, bc_stream stream);" in text
    assert _lib.TINY_VAE_OPS == {"bc_tiny_conv3x3_flat": 57, "bc_tiny_latents_in": 58}
    assert _lib.op_code("bc_tiny_conv3x3_flat") == 57 and _lib.op_signature("bc_tiny_conv3x3_flat") == "pppppiiiiiiii"
    assert _lib.op_code("bc_tiny_latents_in") == 58 and _lib.op_signature("bc_tiny_latents_in") == "piiip"
    assert _lib.op_code("bc_attention_ip_masked") == 55 and _lib.op_signature("bc_freeu") == "pipiiipippppp"     # the older tables still resolve
    with pytest.raises(KeyError):
        _lib.op_code("bc_tiny_conv3x3")
    lib = _lib.load()
    plan = C.c_void_p()
    assert lib.bc_plan_create(C.byref(plan)) == 0
    seg = lib.bc_plan_segment(plan, b"t")
    words = (C.c_uint64 * 13)()
    assert lib.bc_plan_add_op(plan, seg, 0, 57, words, 13) == 0 and lib.bc_plan_add_op(plan, seg, 0, 58, words, 5) == 1
    assert lib.bc_plan_add_op(plan, seg, 0, 57, words, 12) < 0 and lib.bc_plan_add_op(plan, seg, 0, 59, words, 13) < 0
    assert lib.bc_plan_add_op(plan, seg, 0, 56, words, 13) < 0
    assert lib.bc_plan_destroy(plan) == 0
    assert C.sizeof(_lib.BcTinyConvArgs) == 5 * 8 + 8 * 4


def _args(**over):
    a = dict(x=0x1000, w=0x2000, bias=0x3000, skip=None, out=0x4000, B=2, H=6, W=6, Ci=64, Co=64, up=0, relu=1, out_mode=0)
    a.update(over)
    return _lib.BcTinyConvArgs(**a)


@pytest.mark.parametrize("over,word", [
    (dict(x=None), b"null"), (dict(w=None), b"null"), (dict(out=None), b"null"), (dict(B=0), b"B=0"), (dict(H=0), b"H=0"), (dict(W=-1), b"W=-1"),
    (dict(Ci=16), b"Ci=16"), (dict(Co=8), b"Co=8"), (dict(out_mode=3), b"out_mode=3"), (dict(out_mode=1), b"Co=64 stores fp16"),
    (dict(Co=3, relu=0), b"Co=3 stores the image"), (dict(Co=3, out_mode=2, relu=1), b"no up, skip or relu"),
    (dict(Co=3, out_mode=1, relu=0, up=1), b"no up, skip or relu"), (dict(Ci=8, up=1), b"Ci=8 form"), (dict(Ci=8, skip=0x5000), b"Ci=8 form"),
    (dict(up=1, H=5), b"even output size"), (dict(x=0x1008), b"16-byte"), (dict(skip=0x5004), b"16-byte"), (dict(out=0x4002), b"16-byte"),
    (dict(bias=0x3002), b"aligned fp32"), (dict(Co=3, out_mode=1, relu=0, out=0x4002), b"aligned fp32"),
])
def test_conv_refuses_bad_arguments_before_any_launch(over, word):
    """Every refusal comes from the host wrapper (the pointers are not device memory: a launch would not return an argument error)."""
    lib = _lib.load()
    assert lib.bc_tiny_conv3x3(C.byref(_args(**over)), None) == 1
    assert b"bc_tiny_conv3x3" in lib.bc_last_error() and word in lib.bc_last_error(), lib.bc_last_error()
    assert lib.bc_tiny_conv3x3(None, None) == 1
    assert lib.bc_tiny_latents_in(None, 1, 1, 1, 0x1000, None) == 1 and lib.bc_tiny_latents_in(0x1000, 1, 0, 1, 0x2000, None) == 1
    assert lib.bc_tiny_latents_in(0x1000, 1, 1, 1, 0x2008, None) == 1 and b"16-byte" in lib.bc_last_error()


def _write_safetensors(path, sd):
    head, blobs, off = {}, [], 0
    for k, v in sd.items():
        raw = v.contiguous().numpy().astype("<f4").tobytes()
        head[k] = dict(dtype="F32", shape=list(v.shape), data_offsets=[off, off + len(raw)])
        blobs.append(raw)
        off += len(raw)
    hj = json.dumps(head).encode()
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(hj)) + hj + b"".join(blobs))


def test_from_pretrained_and_config(tmp_path, module):
    sd = dict(tv.weights())
    sd["encoder.layers.0.weight"] = torch.zeros(64, 3, 3, 3)            # encoder keys may be present and are ignored
    _write_safetensors(str(tmp_path / "diffusion_pytorch_model.safetensors"), sd)
    cfg = dict(_class_name="AutoencoderTiny", act_fn="relu", decoder_block_out_channels=[64, 64, 64, 64], num_decoder_blocks=[3, 3, 3, 1],
               latent_channels=4, latent_magnitude=3, latent_shift=0.5, scaling_factor=1.0, upsample_fn="nearest", out_channels=3,
               block_out_channels=[64, 64, 64, 64], upsampling_scaling_factor=2)
    json.dump(cfg, open(tmp_path / "config.json", "w"))
    m = AutoencoderTiny.from_pretrained(str(tmp_path), device="cpu")
    assert all(torch.equal(m.h[k], module.h[k]) for k in module.h) and all(torch.equal(m.f[k], module.f[k]) for k in module.f)
    c = m.config
    assert c.scaling_factor == 1.0 and c.latent_magnitude == 3 and c.latent_shift == 0.5 and c.latent_channels == 4
    assert c.num_decoder_blocks == (3, 3, 3, 1) and c.decoder_block_out_channels == (64,) * 4 and c.block_out_channels == (64,) * 4
    assert c.num_encoder_blocks == (1, 3, 3, 3) and c.encoder_block_out_channels == (64,) * 4
    x = torch.linspace(-4, 4, 9)
    assert torch.equal(m.scale_latents(x), x.div(6).add(0.5).clamp(0, 1)) and torch.equal(m.unscale_latents(x), x.sub(0.5).mul(6))
    for field, value in (("act_fn", "swish"), ("upsample_fn", "bilinear"), ("latent_channels", 16), ("num_decoder_blocks", [3, 3, 1]),
                         ("decoder_block_out_channels", [32, 32, 32, 32]), ("out_channels", 4), ("upsampling_scaling_factor", 4)):
        json.dump(dict(cfg, **{field: value}), open(tmp_path / "config.json", "w"))
        with pytest.raises(ValueError, match=field):
            AutoencoderTiny.from_pretrained(str(tmp_path), device="cpu")


def test_refusals(module):
    sd = tv.weights()
    small = synth.synth_state_dict(synth.tiny_vae_param_shapes(channels=32), 1)
    with pytest.raises(ValueError, match="decoder_block_out_channels"):
        AutoencoderTiny(small, device="cpu")
    with pytest.raises(ValueError, match="num_decoder_blocks"):
        AutoencoderTiny(synth.synth_state_dict(synth.tiny_vae_param_shapes(num_decoder_blocks=(3, 3, 1)), 1), device="cpu")
    with pytest.raises(ValueError, match="latent_channels"):
        AutoencoderTiny(synth.synth_state_dict(synth.tiny_vae_param_shapes(latent_channels=16), 1), device="cpu")
    with pytest.raises(ValueError, match="out_channels"):
        AutoencoderTiny(synth.synth_state_dict(synth.tiny_vae_param_shapes(out_channels=4), 1), device="cpu")
    with pytest.raises(ValueError, match="no decoder"):
        AutoencoderTiny({k: v for k, v in sd.items() if "layers.0." not in k}, device="cpu")
    with pytest.raises(NotImplementedError, match="latent_dist"):
        module.encode(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="memory"):
        module.enable_tiling()
    module.disable_tiling()
    module.enable_slicing()
    assert module.use_slicing
    module.disable_slicing()
    assert not module.use_slicing and not module.use_tiling
    with pytest.raises(ValueError, match="latents"):
        module.decode(torch.zeros(1, 3, 4, 4))
    with pytest.raises(_lib.BlobCtrlHipError, match="no CPU fallback"):                  # a host module records and refuses to run
        module.decode(torch.zeros(1, 4, 4, 4))


def test_pipeline_preview_needs_a_loaded_vae():
    from blobctrl_amd.pipeline import BlobCtrlEngine, StableDiffusionBlobNetPipeline
    for cls in (BlobCtrlEngine, StableDiffusionBlobNetPipeline):
        obj = cls.__new__(cls)
        obj.device = torch.device("cpu")
        with pytest.raises(ValueError, match="load_preview_vae"):
            obj.preview(torch.zeros(1, 4, 4, 4), "uint8")
        tiny = obj.load_preview_vae(tv.weights())
        assert obj.preview_vae is tiny and isinstance(tiny, AutoencoderTiny)
        with pytest.raises(ValueError, match="output_type"):
            obj.preview(torch.zeros(1, 4, 4, 4), "latent")
        obj.unload_preview_vae()
        assert obj.preview_vae is None
