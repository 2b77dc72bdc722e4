"""Seeds, case tables and float64 restatements for the image side of an IP-Adapter: the CLIP vision tower and its image processor
(tests/test_clip_vision_cpu.py, tests/test_clip_vision_gpu.py; tests/golden/clip_vision_tiny.npz, clip_processor.npz), the pipeline call
with `ip_adapter_image` (pipeline_call_ip_image.npz) and IP-Adapter Plus (tests/test_ip_plus_cpu.py, tests/test_ip_plus_gpu.py;
ip_plus_tiny.npz).  The fixtures come from tools/make_golden.py (golden_clip_vision, golden_clip_processor, golden_pipeline_call_ip_image,
golden_ip_plus) and hold outputs only: weights and inputs come from seeds on both sides.  Nothing here needs a device.

The tiny Plus adapter for the tiny UNet of tests.common: IPAdapterPlusImageProjection (the Resampler, D/models/embeddings.py:1352-1441) with
embed_dims 64, hidden_dims 128 (2 heads of 64), depth 4 and 16 or 8 queries, stored in the ORIGINAL key spelling (`layers.{i}.0.norm1`,
a fused `to_kv`, `layers.{i}.1.{0,1,3}`) so that a loader's renaming is exercised; `plus_converted` spells the same weights as the
reference's module does."""
import torch

from tests.common import g

PLUS_EMBED, PLUS_HIDDEN, PLUS_SEQ, PLUS_DEPTH = 64, 128, 10, 4
PLUS_QUERIES = {"q16": 16, "q8": 8}
PLUS_SEED = 5200
PLUS_HIDDEN_SCALE = 2.0                  # seed scale of the hidden states (raised until the variants lie 10 bars apart, not the bar lowered)

# the UNet cases: geometry of tests/ip_adapter_common.py IP_GEOMETRIES, then the adapters as (kind, images): "q16" / "q8" a Plus adapter
# of that many queries, "base" tiny_ip_adapter.  plus_one: T = 16; plus_two: two images, T = 32; plus_base: a Plus and a base adapter
PLUS_UNET_CASES = {"plus_one": ("wide16", (("q16", 1),)), "plus_two": ("square16", (("q16", 2),)),
                   "plus_base": ("square16", (("q16", 1), ("base", 1)))}
PLUS_UNET_SCALES = {"plus_one": (0.8,), "plus_two": (0.7,), "plus_base": (0.7, 0.5)}
PLUS_TOKEN_SHAPES = {"one": (2, 1), "two": (2, 2)}            # hidden states [2][1][10][64] and [2][2][10][64]


# ---------------------------------------------------------------------------------------------------- the CLIP vision tower
# tests/golden/clip_vision_tiny.npz (tools/make_golden.py golden_clip_vision): transformers' CLIPVisionModelWithProjection at two random tiny
# configurations, batch 2.  "a": 10 tokens, d = 32, quick_gelu (ViT-L's activation); "b": d = 80 (ViT-H's head size), gelu, 17 tokens -
# one more than a 16-key tile.  Stored: image_embeds and hidden_states[-2] for a seeded input and for an all-zero one.
CLIP_VISION_CONFIGS = {
    "a": dict(hidden_size=64, num_attention_heads=2, num_hidden_layers=3, patch_size=14, image_size=42, hidden_act="quick_gelu",
              projection_dim=24, intermediate_size=256),
    "b": dict(hidden_size=160, num_attention_heads=2, num_hidden_layers=2, patch_size=14, image_size=56, hidden_act="gelu",
              projection_dim=24, intermediate_size=640),
}
CLIP_VISION_SEED, CLIP_VISION_BATCH = 5600, 2


def clip_vision_weights(name, prefix="vision_model."):
    """The seeded state dict of a configuration with transformers' key names (`pre_layrnorm` is its own spelling)."""
    from blobctrl_amd import synth
    c = CLIP_VISION_CONFIGS[name]
    D, F_, p, n = c["hidden_size"], c["intermediate_size"], c["patch_size"], (c["image_size"] // c["patch_size"]) ** 2 + 1
    v = prefix
    shapes = {v + "embeddings.class_embedding": (D,), v + "embeddings.patch_embedding.weight": (D, 3, p, p),
              v + "embeddings.position_embedding.weight": (n, D), v + "pre_layrnorm.weight": (D,), v + "pre_layrnorm.bias": (D,),
              v + "post_layernorm.weight": (D,), v + "post_layernorm.bias": (D,), "visual_projection.weight": (c["projection_dim"], D)}
    for i in range(c["num_hidden_layers"]):
        q = f"{v}encoder.layers.{i}."
        for m in ("q_proj", "k_proj", "v_proj", "out_proj"):
            shapes[q + f"self_attn.{m}.weight"], shapes[q + f"self_attn.{m}.bias"] = (D, D), (D,)
        shapes.update({q + "layer_norm1.weight": (D,), q + "layer_norm1.bias": (D,), q + "layer_norm2.weight": (D,), q + "layer_norm2.bias": (D,),
                       q + "mlp.fc1.weight": (F_, D), q + "mlp.fc1.bias": (F_,), q + "mlp.fc2.weight": (D, F_), q + "mlp.fc2.bias": (D,)})
    sd = synth.synth_state_dict(shapes, CLIP_VISION_SEED + sorted(CLIP_VISION_CONFIGS).index(name))
    sd[v + "embeddings.class_embedding"] = 0.05 * (sd[v + "embeddings.class_embedding"] - 1.0) / 0.1     # (a token, not a norm scale)
    sd[v + "embeddings.position_embedding.weight"] = 0.3 * sd[v + "embeddings.position_embedding.weight"] * D ** 0.5
    return dict(sd)


def clip_vision_pixels(name):
    c = CLIP_VISION_CONFIGS[name]
    return g(5700 + sorted(CLIP_VISION_CONFIGS).index(name), CLIP_VISION_BATCH, 3, c["image_size"], c["image_size"])


def clip_vision64(name, sd, pixels):
    """The tower restated in float64 from transformers' key names: (image_embeds [B][P], hidden_states[-2] [B][N][D])."""
    import torch.nn.functional as F
    c = CLIP_VISION_CONFIGS[name]
    p = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v.double() for k, v in sd.items()}
    D, heads, B = c["hidden_size"], c["num_attention_heads"], pixels.shape[0]
    x = F.conv2d(pixels.double(), p["embeddings.patch_embedding.weight"], stride=c["patch_size"]).flatten(2).transpose(1, 2)      # no bias
    x = torch.cat([p["embeddings.class_embedding"].expand(B, 1, D), x], 1) + p["embeddings.position_embedding.weight"]
    x = F.layer_norm(x, (D,), p["pre_layrnorm.weight"], p["pre_layrnorm.bias"])
    act = (lambda t: t * torch.sigmoid(1.702 * t)) if c["hidden_act"] == "quick_gelu" else F.gelu
    split = lambda t: t.reshape(B, -1, heads, D // heads).transpose(1, 2)
    hidden = [x]
    for i in range(c["num_hidden_layers"]):
        q = f"encoder.layers.{i}."
        lin = lambda t, m: t @ p[q + m + ".weight"].T + p[q + m + ".bias"]
        h = F.layer_norm(x, (D,), p[q + "layer_norm1.weight"], p[q + "layer_norm1.bias"])
        s = torch.softmax(split(lin(h, "self_attn.q_proj")) @ split(lin(h, "self_attn.k_proj")).transpose(-1, -2) * (D // heads) ** -0.5, -1)
        x = x + lin((s @ split(lin(h, "self_attn.v_proj"))).transpose(1, 2).reshape(B, -1, D), "self_attn.out_proj")
        h = F.layer_norm(x, (D,), p[q + "layer_norm2.weight"], p[q + "layer_norm2.bias"])
        x = x + lin(act(lin(h, "mlp.fc1")), "mlp.fc2")
        hidden.append(x)
    pooled = F.layer_norm(x[:, 0], (D,), p["post_layernorm.weight"], p["post_layernorm.bias"])
    return pooled @ p["visual_projection.weight"].T, hidden[-2]                                                                   # no bias


# ---------------------------------------------------------------------------------------------------- the CLIP image processor
# tests/golden/clip_processor.npz (tools/make_golden.py golden_clip_processor): transformers' CLIPImageProcessor (its Pillow backend) on a
# landscape, a portrait and an already-square seeded uint8 image, at size / crop 224 and at a tiny 56 / 56 configuration.
CLIP_PROCESSOR_IMAGES = {"landscape": (300, 400), "portrait": (257, 131), "square": (224, 224)}          # (H, W)
CLIP_PROCESSOR_SIZES = (224, 56)


def clip_processor_image(name):
    """Seeded uint8 RGB [H][W][3]: smooth ramps plus noise, so that a shifted crop window or a transposed resize changes the pixels."""
    import numpy as np
    H, W = CLIP_PROCESSOR_IMAGES[name]
    rng = np.random.Generator(np.random.PCG64(5800 + sorted(CLIP_PROCESSOR_IMAGES).index(name)))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([255 * x / W, 255 * y / H, 127 + 120 * np.sin(x / 17.0) * np.cos(y / 11.0)], -1)
    return np.clip(base + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8)


# tests/golden/pipeline_call_ip_image.npz (tools/make_golden.py golden_pipeline_call_ip_image): the reference's `__call__` with
# `ip_adapter_image`, tower "a" as the image encoder (42 pixels; hidden 64 = the Plus adapter's embed_dims, projection 24 = the base one's)
IP_IMAGE_CALL_IMAGES = {"a": "landscape", "b": "portrait"}               # image A, image B -> clip_processor_image
IP_IMAGE_CALL_SEEDS = (2051, 51)                                         # (generator seed, torch.manual_seed)


# ---------------------------------------------------------------------------------------------------- IP-Adapter Plus
def tiny_plus_adapter(kind="q16"):
    """{"image_proj", "ip_adapter"} of a Plus adapter for the tiny UNet, image_proj in the original key spelling."""
    from blobctrl_amd import synth
    from blobctrl_amd.weights import ip_attn2_prefixes
    from tests.common import TINY, tiny_weights
    usd, ctx, Q, Hd = tiny_weights()[0], TINY["ctx"], PLUS_QUERIES[kind], PLUS_HIDDEN
    seed = PLUS_SEED + 100 * sorted(PLUS_QUERIES).index(kind)
    shapes = {"latents": (1, Q, Hd), "proj_in.weight": (Hd, PLUS_EMBED), "proj_in.bias": (Hd,), "proj_out.weight": (ctx, Hd),
              "proj_out.bias": (ctx,), "norm_out.weight": (ctx,), "norm_out.bias": (ctx,)}
    for i in range(PLUS_DEPTH):
        p = f"layers.{i}."
        shapes.update({p + "0.norm1.weight": (Hd,), p + "0.norm1.bias": (Hd,), p + "0.norm2.weight": (Hd,), p + "0.norm2.bias": (Hd,),
                       p + "0.to_q.weight": (Hd, Hd), p + "0.to_kv.weight": (2 * Hd, Hd), p + "0.to_out.weight": (Hd, Hd),
                       p + "1.0.weight": (Hd,), p + "1.0.bias": (Hd,), p + "1.1.weight": (4 * Hd, Hd), p + "1.3.weight": (Hd, 4 * Hd)})
    proj = synth.synth_state_dict(shapes, seed)
    kv = {}
    for j, bp in enumerate(ip_attn2_prefixes(usd.keys())):
        C = usd[bp + "attn2.to_k.weight"].shape[0]
        kv[f"{1 + 2 * j}.to_k_ip.weight"], kv[f"{1 + 2 * j}.to_v_ip.weight"] = (C, ctx), (C, ctx)
    return {"image_proj": dict(proj), "ip_adapter": dict(synth.synth_state_dict(kv, seed + 1))}


def plus_converted(image_proj):
    """The same projection in the spelling of the reference's module (what D/loaders/unet.py:679-724 renames the original keys to)."""
    out = {k: v for k, v in image_proj.items() if not k.startswith("layers.")}
    for i in range(PLUS_DEPTH):
        o, c = f"layers.{i}.", f"layers.{i}."
        for a, b in (("0.norm1", "ln0"), ("0.norm2", "ln1"), ("1.0", "ff.0")):
            out[c + b + ".weight"], out[c + b + ".bias"] = image_proj[o + a + ".weight"], image_proj[o + a + ".bias"]
        out[c + "attn.to_q.weight"] = image_proj[o + "0.to_q.weight"]
        out[c + "attn.to_k.weight"], out[c + "attn.to_v.weight"] = image_proj[o + "0.to_kv.weight"].chunk(2, dim=0)
        out[c + "attn.to_out.0.weight"] = image_proj[o + "0.to_out.weight"]
        out[c + "ff.1.net.0.proj.weight"], out[c + "ff.1.net.2.weight"] = image_proj[o + "1.1.weight"], image_proj[o + "1.3.weight"]
    return out


def plus_hidden(shape_name, seed=5400):
    """Hidden states [B][images][PLUS_SEQ][PLUS_EMBED] of a token case."""
    B, n = PLUS_TOKEN_SHAPES[shape_name]
    return PLUS_HIDDEN_SCALE * g(seed + sorted(PLUS_TOKEN_SHAPES).index(shape_name), B, n, PLUS_SEQ, PLUS_EMBED)


def plus_unet_inputs(case):
    """(x [B][5][H][W], text [B][7][ctx], residual seed, [per adapter: hidden states [B][n][10][64] or embeds [B][n][24]]) of a UNet case."""
    from tests.common import TINY
    from tests.ip_adapter_common import IP_EMBED_DIM, IP_GEOMETRIES
    geo, adapters = PLUS_UNET_CASES[case]
    B, H, W = IP_GEOMETRIES[geo]
    seed = 9000 + 1000 * sorted(PLUS_UNET_CASES).index(case)
    ins = [g(seed + 510 + i, B, n, IP_EMBED_DIM) if kind == "base" else PLUS_HIDDEN_SCALE * g(seed + 510 + i, B, n, PLUS_SEQ, PLUS_EMBED)
           for i, (kind, n) in enumerate(adapters)]
    return g(seed + 500, B, 5, H, W), g(seed + 501, B, 7, TINY["ctx"]), seed, ins


def plus_unet_adapters(case):
    """The state dicts of a UNet case's adapters, in order."""
    from tests.ip_adapter_common import tiny_ip_adapter
    return [tiny_ip_adapter(0) if kind == "base" else tiny_plus_adapter(kind) for kind, _ in PLUS_UNET_CASES[case][1]]


def resampler64(image_proj, x):
    """IPAdapterPlusImageProjection.forward restated in float64 from the ORIGINAL-spelling keys: x [N][S][embed] -> [N][Q][ctx]."""
    import torch.nn.functional as F
    p = {k: v.double() for k, v in image_proj.items()}
    x = x.double()
    N, Hd = x.shape[0], p["latents"].shape[2]
    heads = p["layers.0.0.to_q.weight"].shape[0] // 64
    lat = p["latents"].repeat(N, 1, 1)
    x = x @ p["proj_in.weight"].T + p["proj_in.bias"]
    split = lambda t: t.reshape(N, -1, heads, 64).transpose(1, 2)
    for i in range(PLUS_DEPTH):
        o = f"layers.{i}."
        e = torch.cat([F.layer_norm(x, (Hd,), p[o + "0.norm1.weight"], p[o + "0.norm1.bias"]),
                       F.layer_norm(lat, (Hd,), p[o + "0.norm2.weight"], p[o + "0.norm2.bias"])], 1)
        q = F.layer_norm(lat, (Hd,), p[o + "0.norm2.weight"], p[o + "0.norm2.bias"]) @ p[o + "0.to_q.weight"].T
        wk, wv = p[o + "0.to_kv.weight"].chunk(2, dim=0)
        s = torch.softmax(split(q) @ split(e @ wk.T).transpose(-1, -2) / 8.0, -1)
        a = (s @ split(e @ wv.T)).transpose(1, 2).reshape(N, -1, heads * 64)
        lat = a @ p[o + "0.to_out.weight"].T + lat
        h = F.layer_norm(lat, (Hd,), p[o + "1.0.weight"], p[o + "1.0.bias"])
        lat = F.gelu(h @ p[o + "1.1.weight"].T) @ p[o + "1.3.weight"].T + lat
    out = lat @ p["proj_out.weight"].T + p["proj_out.bias"]
    return F.layer_norm(out, (out.shape[-1],), p["norm_out.weight"], p["norm_out.bias"])
