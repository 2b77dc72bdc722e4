"""LoRA files as they ship: kohya / sd-scripts keys (`lora_unet_*`, `lora_te_*`) next to the diffusers spellings, text-encoder LoRA, and
the per-call LoRA scale (`cross_attention_kwargs={"scale": s}`) - the host side.  The key tables are pinned against the reference's own
conversion through tests/golden/lora_kohya_keys.json (tools/make_golden.py golden_lora_kohya); the GPU twin is
tests/test_lora_formats_gpu.py."""
import json
import os
from collections import OrderedDict

import pytest
import torch

from tests.common import PIPE, TINY, g, write_model_tree
from tests.test_pipeline_construct_cpu import construct_pipeline, expected_unet_state_dict

RANK = 4
WQ = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q"
FF = "mid_block.attentions.0.transformer_blocks.0.ff.net.2"
CONV1 = "down_blocks.0.resnets.0.conv1"
TE_KINDS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2")


def unet_adapter(pieces):
    """The adapter of `write_model_tree` plus a 3x3 down / 1x1 up pair on a resnet convolution, as [(module, A, B, alpha or None)]: one
    alpha equal to the rank (twice: the most common one), one different alpha, one module without alpha."""
    t = pieces["lora"]
    c0 = TINY["boc"][0]
    pair = lambda m: (t[f"unet.{m}.lora_A.weight"], t[f"unet.{m}.lora_B.weight"])
    return [(WQ,) + pair(WQ) + (float(RANK),), ("conv_in",) + pair("conv_in") + (float(RANK),), (FF,) + pair(FF) + (2.0,),
            (CONV1, g(7, RANK, c0, 3, 3) * 0.2, g(8, c0, RANK, 1, 1) * 0.2, None)]


def te_adapter(layers=(0, 1), scale=0.2):
    """All six module kinds of the tiny CLIP text encoder's layers: alpha = rank on most, another alpha on fc1, none on fc2."""
    c = PIPE["clip"]
    out, seed = [], 100
    for i in layers:
        for kind in TE_KINDS:
            n_out, n_in = {"mlp.fc1": (c["inter"], c["hidden"]), "mlp.fc2": (c["hidden"], c["inter"])}.get(kind, (c["hidden"],) * 2)
            alpha = {"mlp.fc1": 2.0, "mlp.fc2": None}.get(kind, float(RANK))
            out.append((f"text_model.encoder.layers.{i}.{kind}", g(seed, RANK, n_in) * scale, g(seed + 1, n_out, RANK) * scale, alpha))
            seed += 2
    return out


def diffusers_form(adapter, prefix="unet.", down=".lora_A.weight", up=".lora_B.weight", rename=lambda m: m):
    sd = OrderedDict()
    for m, a, b, alpha in adapter:
        sd[prefix + rename(m) + down], sd[prefix + rename(m) + up] = a, b
        if alpha is not None:
            sd[prefix + rename(m) + down + ".alpha"] = torch.tensor(alpha)
    return sd


def kohya_form(adapter, prefix="lora_unet_"):
    sd = OrderedDict()
    for m, a, b, alpha in adapter:
        k = prefix + m.replace(".", "_")
        sd[k + ".lora_down.weight"], sd[k + ".lora_up.weight"] = a, b
        if alpha is not None:
            sd[k + ".alpha"] = torch.tensor(alpha)
    return sd


def _old_attn(m):                                           # the attention-processor spelling: q_proj -> to_q_lora (no separate module level)
    for new, old in (("q_proj", "to_q_lora"), ("k_proj", "to_k_lora"), ("v_proj", "to_v_lora"), ("out_proj", "to_out_lora")):
        if m.endswith("self_attn." + new):
            return m[: -len(new)] + old
    return m


def te_spellings(adapter):
    """The three spellings `convert_state_dict_to_peft` accepts, and the kohya one."""
    old = OrderedDict()
    for part in (diffusers_form([e], "text_encoder.", ".down.weight", ".up.weight", _old_attn) if "self_attn" in e[0] else
                 diffusers_form([e], "text_encoder.", ".lora_linear_layer.down.weight", ".lora_linear_layer.up.weight") for e in adapter):
        old.update(part)
    return {"to_q_lora.down": old,
            "q_proj.lora_linear_layer.down": diffusers_form(adapter, "text_encoder.", ".lora_linear_layer.down.weight",
                                                            ".lora_linear_layer.up.weight"),
            "q_proj.lora_A": diffusers_form(adapter, "text_encoder."),
            "kohya": kohya_form(adapter, "lora_te_")}


def write_adapter_dirs(root, pieces):
    """<root>/lora_diffusers and <root>/lora_kohya: the same adapter - UNet and text-encoder tensors - in the two forms."""
    from blobctrl_amd import checkpoint as ck
    d, k = os.path.join(str(root), "lora_diffusers"), os.path.join(str(root), "lora_kohya")
    for p in (d, k):
        os.makedirs(p, exist_ok=True)
    both = diffusers_form(unet_adapter(pieces))
    both.update(diffusers_form(te_adapter(), "text_encoder."))
    ck.write_safetensors(os.path.join(d, "pytorch_lora_weights.safetensors"), both)
    both = kohya_form(unet_adapter(pieces))
    both.update(kohya_form(te_adapter(), "lora_te_"))
    ck.write_safetensors(os.path.join(k, "pytorch_lora_weights.safetensors"), both)
    return d, k


def test_every_sd15_module_converts_like_the_reference(golden_dir):
    from blobctrl_amd import checkpoint as ck
    entries = json.load(open(os.path.join(golden_dir, "lora_kohya_keys.json")))["entries"]
    assert len(entries) == 278 + 72
    raw = OrderedDict()
    for i, e in enumerate(entries):                          # alpha i + 1 marks entry i
        raw[e["kohya"] + ".lora_down.weight"], raw[e["kohya"] + ".lora_up.weight"] = torch.zeros(1, 1), torch.zeros(1, 1)
        raw[e["kohya"] + ".alpha"] = torch.tensor(float(i + 1))
    assert ck.is_kohya(raw)
    conv = ck.convert_kohya_state_dict(raw)
    assert len(conv) == len(raw)
    unet, te = ck.split_lora_state_dict(raw)
    for i, e in enumerate(entries):
        lora, alphas = unet if e["model"] == "unet" else te
        assert e["model"] + "." + e["module"] + ".lora_A.weight" in conv, e["kohya"]
        assert e["module"] + ".lora_A.weight" in lora and e["module"] + ".lora_B.weight" in lora, e["kohya"]
        assert alphas[e["alpha_module"]] == float(i + 1), e["kohya"]
        assert e["alpha_module"] == e["module"] == e.get("peft_alpha_pattern", e["module"])
    assert len(unet[1]) == 278 and len(te[1]) == 72
    # the model's own module names give the same table as the SD-1.5 default
    um, tm = ck.sd15_lora_modules()
    assert ck.convert_kohya_state_dict(raw, um, tm).keys() == conv.keys()


def test_kohya_file_equals_its_diffusers_form(tmp_path):
    from blobctrl_amd import checkpoint as ck
    from blobctrl_amd.modules import UNet2DConditionModel
    paths, pieces = write_model_tree(tmp_path)
    d, k = write_adapter_dirs(tmp_path, pieces)
    (lora_d, alpha_d), (lora_k, alpha_k) = ck.load_lora(d), ck.load_lora(k)
    assert list(lora_d) == list(lora_k) and len(lora_d) == 8
    assert all(torch.equal(lora_d[n], lora_k[n]) for n in lora_d)
    assert alpha_d == alpha_k == {WQ: 4.0, "conv_in": 4.0, FF: 2.0, CONV1: 4.0}      # (no alpha key: the most common alpha)
    assert lora_k[CONV1 + ".lora_A.weight"].shape[2:] == (3, 3) and lora_k[CONV1 + ".lora_B.weight"].shape[2:] == (1, 1)
    # through the two public ways in: from_pretrained(lora_path=) and pipeline.load_lora_weights
    make = lambda p: UNet2DConditionModel.from_pretrained(paths["sd15"], subfolder="unet", extra_in_channels=1, lora_path=p, device="cpu")
    sd_d, sd_k = make(d).effective_state_dict(), make(k).effective_state_dict()
    pipe_d, pipe_k = construct_pipeline(dict(paths, unet_lora=d), "cpu"), construct_pipeline(dict(paths, unet_lora=k), "cpu")
    pd, pk = pipe_d.unet.effective_state_dict(), pipe_k.unet.effective_state_dict()
    base = ck.expand_conv_in(pieces["unet4"], 1)
    for n in base:
        assert torch.equal(sd_d[n], sd_k[n]) and torch.equal(pd[n], pk[n]) and torch.equal(pd[n], sd_d[n]), n
    for m in (WQ, "conv_in", FF, CONV1):
        assert not torch.equal(pk[m + ".weight"], base[m + ".weight"]), m
    # the text-encoder keys of either file went to the text encoder, under the same adapter name
    assert pipe_k.get_list_adapters() == pipe_d.get_list_adapters() == {"unet": ["default"], "text_encoder": ["default"]}
    te_d, te_k = pipe_d.text_encoder.effective_state_dict(), pipe_k.text_encoder.effective_state_dict()
    assert all(torch.equal(te_d[n], te_k[n]) for n in te_d)
    assert not torch.equal(te_k["encoder.layers.1.mlp.fc2.weight"], pieces["clip"]["text_model.encoder.layers.1.mlp.fc2.weight"])


@pytest.mark.parametrize("spelling", ["to_q_lora.down", "q_proj.lora_linear_layer.down", "q_proj.lora_A", "kohya"])
def test_text_encoder_merge_is_the_closed_form(spelling):
    from blobctrl_amd import checkpoint as ck
    from blobctrl_amd.clip_text import CLIPTextModel
    from tests.common import tiny_pipeline_weights
    _, csd, _ = tiny_pipeline_weights()
    adapter = te_adapter()
    raw = te_spellings(adapter)[spelling]
    assert any(spelling in k for k in raw) or spelling == "kohya"
    unet, (lora, alphas) = ck.split_lora_state_dict(raw)
    assert unet is None and len(alphas) == 12
    w = 0.75
    te = CLIPTextModel(csd, num_heads=PIPE["clip"]["heads"], device="cpu")
    te.load_lora_adapter(lora, alphas, adapter_name="a", weight=w)
    for s in (1.0, 0.5, 0.0):
        got = te.effective_state_dict(lora_scale=s)
        for m, a, b, alpha in adapter:
            alpha = float(RANK) if alpha is None else alpha                   # (the most common alpha is the default)
            want = csd[m + ".weight"].double() + s * w * (alpha / RANK) * (b.double() @ a.double())
            err = (got[m[len("text_model."):] + ".weight"].double() - want).abs().max().item()
            assert err < 1e-6, (m, s, err)
    assert all(torch.equal(v, csd["text_model." + n]) for n, v in te.effective_state_dict(lora_scale=0.0).items())
    te.unload_lora()
    assert te.effective_state_dict() is te._sd


def test_unet_lora_scale_is_the_adapter_weight(tmp_path):
    paths, pieces = write_model_tree(tmp_path)
    pipe = construct_pipeline(paths, "cpu")
    half, want_half = pipe.unet.effective_state_dict(lora_scale=0.5), expected_unet_state_dict(pieces, 0.5)
    for n in want_half:
        assert (half[n] - want_half[n]).abs().max().item() <= 1e-7, n
    full, want = pipe.unet.effective_state_dict(), expected_unet_state_dict(pieces)
    assert all(torch.equal(full[n], want[n]) for n in want)
    # the packed copy is made for one (adapters, scale) state: a new scale drops it, the same scale does not
    v = pipe.unet._version
    pipe.unet.set_lora_scale(0.5)
    assert pipe.unet._version == v + 1
    pipe.unet.set_lora_scale(0.5)
    assert pipe.unet._version == v + 1
    assert all(torch.equal(a, b) for a, b in zip(pipe.unet.effective_state_dict().values(), want.values()))     # no argument: scale 1.0
    pipe.unload_lora_weights()
    v = pipe.unet._version
    pipe.unet.set_lora_scale(0.25)                           # nothing to scale: nothing dropped
    assert pipe.unet._version == v


def test_refusals(tmp_path):
    from blobctrl_amd import checkpoint as ck
    from blobctrl_amd.weights import lora_scale_of
    paths, pieces = write_model_tree(tmp_path)
    ok = kohya_form(unet_adapter(pieces))
    ly = OrderedDict(ok)
    for k in ("lora_unet_" + WQ.replace(".", "_") + ".hada_w1_a", "lora_unet_" + FF.replace(".", "_") + ".lokr_w1"):
        ly[k] = torch.zeros(2, 2)
    with pytest.raises(ValueError, match="hada_w1_a.*lokr_w1"):
        ck.split_lora_state_dict(ly)
    with pytest.raises(NotImplementedError, match="DoRA"):
        ck.split_lora_state_dict(OrderedDict(ok, **{"lora_unet_" + WQ.replace(".", "_") + ".dora_scale": torch.ones(1, 16)}))
    with pytest.raises(ValueError, match="lora_te2_"):
        ck.split_lora_state_dict(OrderedDict(ok, **kohya_form(te_adapter((0,)), "lora_te2_")))
    ldm = OrderedDict((k.replace("lora_unet_down_blocks_0_attentions_0", "lora_unet_input_blocks_1_1")
                       .replace("lora_unet_mid_block_attentions_0", "lora_unet_middle_block_1"), v) for k, v in ok.items())
    with pytest.raises(NotImplementedError, match="lora_unet_input_blocks_"):
        ck.split_lora_state_dict(ldm)
    pipe = construct_pipeline(paths, "cpu")
    pipe.text_encoder = None
    with pytest.raises(ValueError, match="text encoder"):
        pipe.load_lora_weights(OrderedDict(ok, **kohya_form(te_adapter(), "lora_te_")), adapter_name="te")
    assert pipe.get_list_adapters() == {"unet": ["default"]}
    with pytest.raises(ValueError, match="foo"):
        pipe(prompt="a frog", cross_attention_kwargs={"scale": 0.5, "foo": 1})
    with pytest.raises(TypeError):
        pipe(prompt="a frog", cross_attention_kwargs={"scale": "0.5"})
    assert lora_scale_of(None) == 1.0 and lora_scale_of({}) == 1.0 and lora_scale_of({"scale": 2}) == 2.0


def test_adapter_registry_of_the_pipeline(tmp_path):
    paths, pieces = write_model_tree(tmp_path)
    _, k = write_adapter_dirs(tmp_path, pieces)
    pipe = construct_pipeline(paths, "cpu")                  # "default": UNet only
    pipe.load_lora_weights(k, adapter_name="kohya")          # UNet and text encoder
    with pytest.raises(ValueError, match="already in use"):
        pipe.load_lora_weights(k, adapter_name="kohya")
    assert pipe.get_list_adapters() == {"unet": ["default", "kohya"], "text_encoder": ["kohya"]}
    assert pipe.get_active_adapters() == ["default", "kohya"]
    base = pipe.text_encoder._sd
    pipe.disable_lora()
    assert pipe.get_active_adapters() == [] and pipe.text_encoder.effective_state_dict() is base
    assert pipe.get_list_adapters() == {"unet": ["default", "kohya"], "text_encoder": ["kohya"]}
    pipe.enable_lora()
    assert pipe.get_active_adapters() == ["default", "kohya"] and pipe.text_encoder.effective_state_dict() is not base
    pipe.set_adapters(["kohya"], [0.5])
    assert pipe.get_active_adapters() == ["kohya"]
    assert pipe.unet._adapters["kohya"]["weight"] == pipe.text_encoder._adapters["kohya"]["weight"] == 0.5
    pipe.delete_adapters("kohya")
    assert pipe.get_list_adapters() == {"unet": ["default"]} and pipe.get_active_adapters() == []
    pipe.set_adapters(["default"])
    want = expected_unet_state_dict(pieces)
    assert all(torch.equal(v, want[n]) for n, v in pipe.unet.effective_state_dict().items())
    pipe.unload_lora_weights()
    assert pipe.get_list_adapters() == {} and pipe.get_active_adapters() == []
