"""A plain-torch restatement of Segment-Anything's forward pass in fp32 / fp64: the windowed and global encoder layers, the neck, the
point-prompt encoder and the mask decoder, over a transformers-layout state dict.  tests/test_sam_cpu.py proves it against the fixture
that transformers' SamModel wrote (tests/golden/sam_tiny.npz); the GPU tests use it where no fixture exists (full width, two layers), and
the fixture builder uses `mask_padded=True` to measure what attending to the zero-padded window tokens is worth."""
import math

import torch
import torch.nn.functional as F

# the two fixture configurations (tools/make_golden.py golden_sam)
TINY_A = dict(image=256, patch=16, window=7, layers=4, global_attn_indexes=(1, 3), hidden=160, heads=2, mlp_dim=320, out_channels=32,
              decoder_layers=2, decoder_mlp_dim=64, iou_head_hidden_dim=32, seed=131)
TINY_B = dict(image=192, patch=16, window=5, layers=2, global_attn_indexes=(1,), hidden=128, heads=2, mlp_dim=256, out_channels=32,
              decoder_layers=2, decoder_mlp_dim=64, iou_head_hidden_dim=32, seed=132)
DECODER_HEADS = 2
CLICKS = {"one": ([[70.0, 90.0]], [1]), "two": ([[70.0, 90.0], [180.0, 40.0]], [1, 0])}
INPUT_SIZE, ORIGINAL_SIZE = (192, 256), (150, 200)          # the unpadded region of the 256-frame and the "original" image it came from


def shapes_of(cfg):
    from blobctrl_amd import synth
    kw = {k: v for k, v in cfg.items() if k != "seed"}
    return synth.sam_param_shapes(**kw)


def weights_of(cfg, qkv_bias_scale=1.0):
    from blobctrl_amd import synth
    sd = synth.synth_state_dict(shapes_of(cfg), cfg["seed"])
    # one Gaussian matrix under two names (tied in transformers; the original checkpoint stores it once)
    sd["prompt_encoder.shared_embedding.positional_embedding"] = sd["shared_image_embedding.positional_embedding"]
    if qkv_bias_scale != 1.0:
        for k in sd:
            if k.endswith("attn.qkv.bias"):
                sd[k] = sd[k] * qkv_bias_scale
    return sd


def rel_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


def _ln(x, sd, p, eps):
    return F.layer_norm(x, x.shape[-1:], sd[p + ".weight"], sd[p + ".bias"], eps)


def _lin(x, sd, p):
    return x @ sd[p + ".weight"].t() + sd[p + ".bias"]


def _rel_table(t, size):
    want = 2 * size - 1
    if t.shape[0] != want:
        t = F.interpolate(t.t()[None], size=want, mode="linear")[0].t()
    idx = torch.arange(size)[:, None] - torch.arange(size)[None, :] + size - 1
    return t[idx]                                            # [q][k][d]


def vision_attention(x, sd, p, heads, mask=None):
    """x [B][H][W][D] -> proj(softmax(scale q k^T + rel_h + rel_w [+ mask]) v); mask [B][H * W] True = key hidden."""
    B, H, W, D = x.shape
    d = D // heads
    qkv = _lin(x.reshape(B, H * W, D), sd, p + "qkv").reshape(B, H * W, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]                          # [B][heads][N][d]
    s = (q @ k.transpose(-1, -2)) * d ** -0.5
    q5 = q.reshape(B, heads, H, W, d)
    rel_h = torch.einsum("bnhwc,hkc->bnhwk", q5, _rel_table(sd[p + "rel_pos_h"], H))
    rel_w = torch.einsum("bnhwc,wkc->bnhwk", q5, _rel_table(sd[p + "rel_pos_w"], W))
    s = s + (rel_h[..., :, None] + rel_w[..., None, :]).reshape(B, heads, H * W, H * W)
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    o = torch.softmax(s, -1) @ v
    return _lin(o.transpose(1, 2).reshape(B, H, W, D), sd, p + "proj")


def vision_layer(x, sd, p, heads, window, eps, mask_padded=False):
    """One encoder layer on x [B][H][W][D]; window = 0: global attention."""
    B, H, W, D = x.shape
    y = _ln(x, sd, p + "layer_norm1", eps)
    if window:
        ph, pw = (window - H % window) % window, (window - W % window) % window
        Hp, Wp = H + ph, W + pw
        y = F.pad(y, (0, 0, 0, pw, 0, ph))
        y = y.reshape(B, Hp // window, window, Wp // window, window, D).permute(0, 1, 3, 2, 4, 5).reshape(-1, window, window, D)
        mask = None
        if mask_padded:
            real = F.pad(torch.ones(B, H, W), (0, pw, 0, ph))
            real = real.reshape(B, Hp // window, window, Wp // window, window).permute(0, 1, 3, 2, 4).reshape(-1, window * window)
            mask = real == 0
        y = vision_attention(y, sd, p + "attn.", heads, mask)
        y = y.reshape(B, Hp // window, Wp // window, window, window, D).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, D)[:, :H, :W]
    else:
        y = vision_attention(y, sd, p + "attn.", heads)
    x = x + y
    y = _ln(x, sd, p + "layer_norm2", eps)
    return x + _lin(F.gelu(_lin(y, sd, p + "mlp.lin1")), sd, p + "mlp.lin2")


def _ln_channels(x, sd, p, eps=1e-6):
    return _ln(x.permute(0, 2, 3, 1), sd, p, eps).permute(0, 3, 1, 2)


def neck(x, sd):
    """x [B][H][W][D] -> [B][C][H][W]."""
    n = "vision_encoder.neck."
    y = F.conv2d(x.permute(0, 3, 1, 2), sd[n + "conv1.weight"])
    y = _ln_channels(y, sd, n + "layer_norm1")
    y = F.conv2d(y, sd[n + "conv2.weight"], padding=1)
    return _ln_channels(y, sd, n + "layer_norm2")


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def vision_encoder(pixels, sd, heads, window, global_attn_indexes, eps=1e-6, mask_padded=False, layers=None):
    v = "vision_encoder."
    patch = sd[v + "patch_embed.projection.weight"].shape[-1]
    x = F.conv2d(pixels.to(sd[v + "pos_embed"].dtype), sd[v + "patch_embed.projection.weight"], sd[v + "patch_embed.projection.bias"], stride=patch)
    x = x.permute(0, 2, 3, 1) + sd[v + "pos_embed"]
    i = 0
    while f"{v}layers.{i}.attn.qkv.weight" in sd and (layers is None or i < layers):
        x = vision_layer(x, sd, f"{v}layers.{i}.", heads, 0 if i in global_attn_indexes else window, eps, mask_padded)
        i += 1
    return neck(x, sd)


# ------------------------------------------------------------------------------------------------------------ prompt encoder, mask decoder
def _fourier(xy01, gauss):
    a = 2 * math.pi * ((2 * xy01 - 1) @ gauss)
    return torch.cat([a.sin(), a.cos()], -1)


def prompt_tokens(sd, points, labels, image_size):
    """Sparse embeddings [n + 1][C] of n points (x, y in the input frame; labels 1 / 0) and the padding point."""
    pe = "prompt_encoder."
    gauss = sd[pe + "shared_embedding.positional_embedding"]
    pts = (torch.as_tensor(points, dtype=gauss.dtype).reshape(-1, 2) + 0.5) / image_size
    rows = _fourier(pts, gauss)
    for i, lab in enumerate(labels):
        rows[i] = rows[i] + sd[pe + f"point_embed.{int(lab)}.weight"][0]
    return torch.cat([rows, sd[pe + "not_a_point_embed.weight"]], 0)


def image_pe(sd, grid):
    gauss = sd["shared_image_embedding.positional_embedding"]
    t = (torch.arange(grid, dtype=gauss.dtype) + 0.5) / grid
    xy = torch.stack([t[None, :].expand(grid, grid), t[:, None].expand(grid, grid)], -1)
    return _fourier(xy, gauss).reshape(grid * grid, -1)


def _attention(sd, p, q, k, v, heads):
    q, k, v = _lin(q, sd, p + "q_proj"), _lin(k, sd, p + "k_proj"), _lin(v, sd, p + "v_proj")
    d = q.shape[-1] // heads
    split = lambda t: t.reshape(t.shape[0], heads, d).transpose(0, 1)
    o = torch.softmax(split(q) @ split(k).transpose(1, 2) * d ** -0.5, -1) @ split(v)
    return _lin(o.transpose(0, 1).reshape(q.shape[0], heads * d), sd, p + "out_proj")


def _mlp3(sd, p, x):
    return _lin(F.relu(_lin(F.relu(_lin(x, sd, p + "proj_in")), sd, p + "layers.0")), sd, p + "proj_out")


def mask_decoder(sd, emb, points, labels, image_size, heads=DECODER_HEADS, eps=1e-6):
    """emb [C][g][g] of one image -> (low-res logits [4][4 g][4 g], IoU scores [4]) for all four mask tokens."""
    md = "mask_decoder."
    C, g_, _ = emb.shape
    tokens = torch.cat([sd[md + "iou_token.weight"], sd[md + "mask_tokens.weight"], prompt_tokens(sd, points, labels, image_size)], 0)
    keys = (emb + sd["prompt_encoder.no_mask_embed.weight"].reshape(C, 1, 1)).reshape(C, -1).t()
    kpe, qpe, queries = image_pe(sd, g_), tokens, tokens
    i = 0
    while f"{md}transformer.layers.{i}.layer_norm1.weight" in sd:
        p = f"{md}transformer.layers.{i}."
        if i == 0:
            queries = _attention(sd, p + "self_attn.", queries, queries, queries, heads)
        else:
            queries = queries + _attention(sd, p + "self_attn.", queries + qpe, queries + qpe, queries, heads)
        queries = _ln(queries, sd, p + "layer_norm1", eps)
        queries = _ln(queries + _attention(sd, p + "cross_attn_token_to_image.", queries + qpe, keys + kpe, keys, heads), sd, p + "layer_norm2", eps)
        queries = _ln(queries + _lin(F.relu(_lin(queries, sd, p + "mlp.lin1")), sd, p + "mlp.lin2"), sd, p + "layer_norm3", eps)
        keys = _ln(keys + _attention(sd, p + "cross_attn_image_to_token.", keys + kpe, queries + qpe, queries, heads), sd, p + "layer_norm4", eps)
        i += 1
    p = md + "transformer."
    queries = queries + _attention(sd, p + "final_attn_token_to_image.", queries + qpe, keys + kpe, keys, heads)
    queries = _ln(queries, sd, p + "layer_norm_final_attn", 1e-5)
    up = F.conv_transpose2d(keys.t().reshape(1, C, g_, g_), sd[md + "upscale_conv1.weight"], sd[md + "upscale_conv1.bias"], stride=2)
    up = F.gelu(_ln_channels(up, sd, md + "upscale_layer_norm"))
    up = F.gelu(F.conv_transpose2d(up, sd[md + "upscale_conv2.weight"], sd[md + "upscale_conv2.bias"], stride=2))[0]
    n = sd[md + "mask_tokens.weight"].shape[0]
    hyper = torch.stack([_mlp3(sd, f"{md}output_hypernetworks_mlps.{t}.", queries[1 + t]) for t in range(n)])
    masks = (hyper @ up.reshape(up.shape[0], -1)).reshape(n, 4 * g_, 4 * g_)
    return masks, _mlp3(sd, md + "iou_prediction_head.", queries[0])


def postprocess(low, image_size, input_size, original_size):
    """low [n][h][w] -> logits at the original size [n][H][W] (threshold at 0 for the mask)."""
    full = F.interpolate(low[None].float(), size=(image_size, image_size), mode="bilinear", align_corners=False)
    full = full[..., : input_size[0], : input_size[1]]
    return F.interpolate(full, size=tuple(original_size), mode="bilinear", align_corners=False)[0]
