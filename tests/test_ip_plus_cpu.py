"""IP-Adapter Plus without a GPU: the layout test and the conversion of a Resampler projection in both key spellings, a float64
restatement of the Resampler against the reference's tokens (tests/golden/ip_plus_tiny.npz), the 4D / 3D shape rules of the engine, and
the launches a compile-only engine records for a Plus adapter (tests/clip_vision_common.py holds the seeds and case tables)."""
import os

import numpy as np
import pytest
import torch

from tests import clip_vision_common as cv
from tests import ip_adapter_common as ip


@pytest.fixture(scope="module")
def zp(golden_dir):
    return np.load(os.path.join(golden_dir, "ip_plus_tiny.npz"))


def _prefixes():
    from blobctrl_amd.weights import ip_attn2_prefixes
    from tests.common import tiny_weights
    return ip_attn2_prefixes(tiny_weights()[0].keys())


def test_layout_names_plus_in_both_spellings_and_refuses_an_incomplete_projection():
    from blobctrl_amd.weights import convert_ip_adapter, ip_adapter_layout, ip_plus_layers
    from tests.common import TINY
    sd = cv.tiny_plus_adapter("q16")
    orig, conv = sd["image_proj"], cv.plus_converted(sd["image_proj"])
    assert "layers.0.0.to_kv.weight" in orig and "layers.3.attn.to_k.weight" in conv and not set(orig) & {k for k in conv if k.startswith("layers.")}
    assert ip_adapter_layout(orig) == "plus" and ip_adapter_layout(conv) == "plus" and ip_adapter_layout(ip.tiny_ip_adapter(0)["image_proj"]) == "base"
    a, b = ip_plus_layers(orig), ip_plus_layers(conv)
    assert len(a) == len(b) == 4 and all(set(x) == set(y) and all(x[k].equal(y[k]) for k in x) for x, y in zip(a, b))
    for drop in ("layers.2.0.to_out.weight", "layers.3.1.3.weight", "proj_out.bias", "norm_out.weight", "layers.0.0.norm2.bias"):
        part = {k: v for k, v in orig.items() if k != drop}
        with pytest.raises(NotImplementedError, match="Plus"):
            ip_adapter_layout(part)
        with pytest.raises(NotImplementedError, match="Plus"):
            convert_ip_adapter(dict(image_proj=part, ip_adapter=sd["ip_adapter"]), _prefixes(), TINY["ctx"])
    with pytest.raises(NotImplementedError, match="Plus"):                                         # a deeper Resampler than the reference builds
        ip_adapter_layout(dict(orig, **{"layers.4.0.to_q.weight": orig["layers.0.0.to_q.weight"]}))
    with pytest.raises(NotImplementedError, match="FaceID Plus"):
        ip_adapter_layout(dict(orig, **{"perceiver_resampler.proj_in.weight": 0}))


@pytest.mark.parametrize("kind", sorted(cv.PLUS_QUERIES))
def test_convert_has_the_expected_shapes(kind):
    from blobctrl_amd.weights import convert_ip_adapter, ip_adapter_embed_dim, ip_adapter_on_device, ip_adapter_tokens
    from tests.common import TINY
    sd = cv.tiny_plus_adapter(kind)
    Q, Hd, ctx = cv.PLUS_QUERIES[kind], cv.PLUS_HIDDEN, TINY["ctx"]
    for proj in (sd["image_proj"], cv.plus_converted(sd["image_proj"])):
        host = convert_ip_adapter(dict(image_proj=proj, ip_adapter=sd["ip_adapter"]), _prefixes(), ctx)
        assert host["layout"] == "plus" and host["heads"] == 2 and ip_adapter_tokens(host) == Q and ip_adapter_embed_dim(host) == cv.PLUS_EMBED
        assert tuple(host["latents"].shape) == (Q, Hd) and tuple(host["proj_in_w"].shape) == (Hd, cv.PLUS_EMBED)
        assert tuple(host["proj_out_w"].shape) == (ctx, Hd) and tuple(host["norm_w"].shape) == (ctx,) and len(host["layers"]) == 4
        for i, layer in enumerate(host["layers"]):
            assert tuple(layer["qk"].shape) == (2 * Hd, Hd) and tuple(layer["to_v"].shape) == (Hd, Hd) and tuple(layer["ff1"].shape) == (4 * Hd, Hd)
            assert layer["qk"][Hd:].equal(sd["image_proj"][f"layers.{i}.0.to_kv.weight"][:Hd])     # to_k is the first half of to_kv
            assert layer["to_v"].equal(sd["image_proj"][f"layers.{i}.0.to_kv.weight"][Hd:])
        assert list(host["kv"]) == _prefixes()
        dev = ip_adapter_on_device(host, torch.device("cpu"))
        assert dev["latents"].dtype == torch.float16 and dev["layers"][0]["ln0_w"].dtype == torch.float32 and dev["layers"][0]["qk"].dtype == torch.float16
        assert dev["scales"].tolist() == [1.0] * 16 and dev["layout"] == "plus"
    with pytest.raises(ValueError, match="cross_attention_dim"):
        convert_ip_adapter(sd, _prefixes(), ctx + 8)
    base = convert_ip_adapter(ip.tiny_ip_adapter(0), _prefixes(), ctx)
    assert "layout" not in base and ip_adapter_tokens(base) == 4 and ip_adapter_embed_dim(base) == ip.IP_EMBED_DIM


@pytest.mark.parametrize("kind", sorted(cv.PLUS_QUERIES))
def test_float64_resampler_reproduces_the_reference_tokens(zp, kind):
    """The restatement of tests/clip_vision_common.py (original key spelling, fused to_kv, keys = [ln0(x); ln1(latents)], queries from
    ln1(latents), bias-free to_out and feed-forward) against the reference module's fp32 output."""
    proj = cv.tiny_plus_adapter(kind)["image_proj"]
    for name, (B, n) in cv.PLUS_TOKEN_SHAPES.items():
        x = cv.plus_hidden(name)
        tok = cv.resampler64(proj, x.reshape(B * n, cv.PLUS_SEQ, cv.PLUS_EMBED)).reshape(B, n * cv.PLUS_QUERIES[kind], -1).numpy()
        ref = zp[f"tokens_{kind}_{name}"]
        err = float(np.abs(tok - ref).max() / np.abs(ref).max())
        print(f"resampler64 {kind} {name}: max-abs / scale {err:.2e}")
        assert tok.shape == ref.shape and err < 1e-5                                           # the reference is fp32


def _engine(adapters):
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.weights import convert_ip_adapter, ip_adapter_on_device
    from tests.common import TINY, tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    usd, bsd = tiny_weights()
    ucfg, bcfg = tiny_trunk_configs()
    eng = BlobCtrlEngine(usd, bsd, ucfg, bcfg, device="cpu", scheduler="ddim", compile_only=True)
    eng.set_ip_adapters([ip_adapter_on_device(convert_ip_adapter(sd, _prefixes(), TINY["ctx"]), torch.device("cpu")) for sd in adapters])
    return eng


def test_engine_takes_4d_hidden_states_for_plus_and_3d_embeddings_for_base():
    eng = _engine([cv.tiny_plus_adapter("q16"), ip.tiny_ip_adapter(0)])
    h, e = torch.zeros(2, 1, cv.PLUS_SEQ, cv.PLUS_EMBED), torch.zeros(2, 1, ip.IP_EMBED_DIM)
    entries, out = eng._ip_layout([h, e], 2, 1, False)
    assert entries == ((1, cv.PLUS_SEQ), 1) and out[0].shape == h.shape
    assert eng._ip_layout([h[:1].repeat(1, 3, 1, 1), e[:1]], 2, 1, True)[0] == ((3, cv.PLUS_SEQ), 1)
    for bad, word in (([e, e], "hidden states"), ([h[:, 0], e], "hidden states"), ([h[..., :8], e], "hidden states"), ([h, h], "image embeddings"),
                      ([h[:1], e], "UNet batch")):
        with pytest.raises(ValueError, match=word):
            eng._ip_layout(bad, 2, 1, False)


def _count(seg, name):
    return sum(name in (m["variant"] or "") or m["kind"] == name for m in seg.meta)


def test_compile_only_engine_records_the_resampler_and_one_tile_launch_per_attn2():
    """One Plus adapter, one image: the prologue holds the Resampler - per layer two LayerNorms per image row set, a fused q | k GEMM, a
    V^T GEMM, one bc_attention over S + Q keys, to_out, the feed-forward - and K_ip / V_ip per attn2; every UNet forward holds 16
    bc_attention_ip launches with T = 16.  Two images make T = 32 and a plan of their own; the 1280-, 640- and 320-channel classes of the
    full-size UNet would name the tiles (tests/test_attention_ip_tiles_cpu.py), the tiny UNet's widths are unmeasured and stay scalar."""
    from tests.common import TINY
    args = (1, 8, 8, 7, TINY["ctx"], 3)
    eng = _engine([cv.tiny_plus_adapter("q16")])
    P = eng.plan_for(*args, ip=((1, cv.PLUS_SEQ),))
    assert list(eng._plans)[-1][-1] == ("ip", 1, (16, cv.PLUS_EMBED, cv.PLUS_SEQ))
    assert [tuple(e.shape) for e in P.ip_embeds] == [(2, cv.PLUS_SEQ, cv.PLUS_EMBED)]
    pro = P.prologue
    Bi, depth = 2, 4
    assert _count(pro, "ip_resampler") == 1 + depth * 5 + 1 and _count(pro, "ip_proj") == 0 and _count(pro, "ip_kv") == 32
    att = [m for m in pro.meta if m["kind"] == "attention"]
    assert len(att) == depth and all(m["shape"] == (Bi, 2, 64, 16, cv.PLUS_SEQ + 16) for m in att)
    assert _count(pro, "layernorm") >= depth * (2 * Bi + 1) + 1
    for seg in (P.step_active, P.step_inactive):
        ips = [m for m in seg.meta if m["kind"] == "attention_ip"]
        assert len(ips) == 16 and all(m["shape"][0] == "attention_ip" and m["shape"][-1] == 16 for m in ips)
        assert _count(seg, "midx") == 0 and _count(seg, "ctx_fold") == 0
    P2 = eng.plan_for(*args, ip=((2, cv.PLUS_SEQ),))
    assert P2 is not P and list(eng._plans)[-1][-1] == ("ip", 1, (32, cv.PLUS_EMBED, cv.PLUS_SEQ))
    assert all(m["shape"][-1] == 32 for m in P2.step_active.meta if m["kind"] == "attention_ip")
    with pytest.raises(ValueError, match="64"):                                                    # BC_ATTENTION_IP_MAX_T stays
        eng.plan_for(*args, ip=((5, cv.PLUS_SEQ),))
    # the base adapter's plan is what it was: 4 tokens, an ip_proj launch, no Resampler
    base = _engine([ip.tiny_ip_adapter(0)]).plan_for(*args, ip=(1,))
    assert _count(base.prologue, "ip_resampler") == 0 and _count(base.prologue, "ip_proj") == 1


def test_unet_module_checks_the_shapes_per_adapter_kind():
    from blobctrl_amd.modules import UNet2DConditionModel
    from tests.common import tiny_weights
    from tests.gpu_common import tiny_trunk_configs
    unet = UNet2DConditionModel(tiny_weights()[0], tiny_trunk_configs()[0], device="cpu", lazy=True)      # (held on the host: nothing runs)
    unet.load_ip_adapter_weights([cv.tiny_plus_adapter("q8"), ip.tiny_ip_adapter(0)])
    assert [a.get("layout", "base") for a in unet.ip_adapters] == ["plus", "base"] and unet.config.encoder_hid_dim_type == "ip_image_proj"
    h, e = torch.zeros(2, 1, cv.PLUS_SEQ, cv.PLUS_EMBED), torch.zeros(2, 1, ip.IP_EMBED_DIM)
    assert len(unet._check_image_embeds({"image_embeds": [h, e]}, 2)) == 2
    for bad, word in (([e, e], "Plus"), ([h, h], "images"), ([h[..., :8], e], "Plus"), ([h[:1], e], "Plus")):
        with pytest.raises(ValueError, match=word):
            unet._check_image_embeds({"image_embeds": bad}, 2)
