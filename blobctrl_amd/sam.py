"""Segment-Anything (ViT-H) on MI355X behind the `segment_anything.SamPredictor` call surface: the click -> mask step of the reference app
(`segmentation()`, scripts/blobctrl_app.py:1019-1043, model `sam_model_registry['vit_h']`, app:114-116).  Arithmetic of transformers'
`SamModel` (models/sam/modeling_sam.py); weights in its state-dict layout.

  vision encoder   one graph replay: patch embed (bc_patchify + GEMM) -> + pos_embed -> L x { LN -> [zero-padded windows] -> qk / v^T GEMMs ->
                   bc_attention_relpos -> proj -> [un-window] + x ; x + MLP(LN x) } -> neck (1x1 GEMM, LN, 3x3 conv, LN).
                   The reference ATTENDS to the zero rows of a padded window (they leave the qkv GEMM as its bias): bc_window_partition
                   writes real zero rows and nothing masks them.
  prompt encoder   point prompts only (what the app passes): bc_sam_tokens builds the decoder's token rows - output tokens, the points'
                   Fourier features + label embeddings, the padding point - in one launch inside the decoder's graph.
  mask decoder     one graph replay per `predict`: the two-way transformer on bc_attention (head sizes 32 / 16), the upscaler's two 2x2
                   stride-2 transposed convolutions as GEMMs whose sub-pixels stay rows, the hypernetwork MLPs, the IoU head, and
                   bc_sam_masks (hypernetwork product + pixel shuffle).  Then two bc_bilinear_resize_f32 launches.

  batched prompts  `decode_batch` / `SamPredictor.predict_torch`: the decoder's launches over [Bp] prompt sets in one graph replay; what does not
                   depend on the prompt (layer 0's image side) exists once and is read with a batch stride of 0.
  segment all      `SamAutomaticMaskGenerator.generate`: a grid of single-point prompts through `predict_torch` in batches, one
                   bc_mask_stats pass over the full-size logits (the stability counts, the area and the box of every mask), the two
                   filters on the device, box NMS on the host, and only the surviving masks cross to the host.  With
                   `generate(image, min_mask_region_area=N)` the survivors are despeckled on the device first (blobctrl_amd/masks.py:
                   connected components, holes filled and islands removed below N pixels), as the package's post-processing does.

`SamPredictor.set_image` runs the encoder once; every `predict` / `predict_torch` on that image costs the decoder only.
"""
import math
import re

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .launch import Recorder, run_graphed
from .weights import pack_conv3x3, pad8

PIXEL_MEAN = (123.675, 116.28, 103.53)
PIXEL_STD = (58.395, 57.12, 57.375)

# segment_anything checkpoint names <-> transformers names, as (pattern at the head of a key, replacement) rules in both directions; the
# first rule that matches a key is applied, a key that matches none keeps its name.
_MLP_FWD = {"0": "proj_in", "1": "layers.0", "2": "proj_out"}
_MLP_INV = {"proj_in": "layers.0", "layers.0": "layers.1", "proj_out": "layers.2"}
_NECK = {"0": "conv1", "1": "layer_norm1", "2": "conv2", "3": "layer_norm2"}
_DOWN = {"0": "conv1", "1": "layer_norm1", "3": "conv2", "4": "layer_norm2", "6": "conv3"}
_UP = {"0": "upscale_conv1", "1": "upscale_layer_norm", "3": "upscale_conv2"}


def _inv(table):
    return {v: k for k, v in table.items()}


_GAUSS = "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"
_FORWARD = (
    (r"^image_encoder\.blocks\.(\d+)\.norm(\d)\.", lambda m: f"vision_encoder.layers.{m[1]}.layer_norm{m[2]}."),
    (r"^image_encoder\.blocks\.", lambda m: "vision_encoder.layers."),
    (r"^image_encoder\.patch_embed\.proj\.", lambda m: "vision_encoder.patch_embed.projection."),
    (r"^image_encoder\.neck\.(\d)\.", lambda m: f"vision_encoder.neck.{_NECK[m[1]]}."),
    (r"^image_encoder\.", lambda m: "vision_encoder."),
    (r"^prompt_encoder\.pe_layer\.positional_encoding_gaussian_matrix$", lambda m: "prompt_encoder.shared_embedding.positional_embedding"),
    (r"^prompt_encoder\.point_embeddings\.", lambda m: "prompt_encoder.point_embed."),
    (r"^prompt_encoder\.mask_downscaling\.(\d)\.", lambda m: f"prompt_encoder.mask_embed.{_DOWN[m[1]]}."),
    (r"^mask_decoder\.output_upscaling\.(\d)\.", lambda m: f"mask_decoder.{_UP[m[1]]}."),
    (r"^mask_decoder\.(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.layers\.(\d)\.", lambda m: f"mask_decoder.{m[1]}.{_MLP_FWD[m[2]]}."),
    (r"^mask_decoder\.transformer\.layers\.(\d+)\.norm(\d)\.", lambda m: f"mask_decoder.transformer.layers.{m[1]}.layer_norm{m[2]}."),
    (r"^mask_decoder\.transformer\.norm_final_attn\.", lambda m: "mask_decoder.transformer.layer_norm_final_attn."),
)
_BACKWARD = (
    (r"^vision_encoder\.layers\.(\d+)\.layer_norm(\d)\.", lambda m: f"image_encoder.blocks.{m[1]}.norm{m[2]}."),
    (r"^vision_encoder\.layers\.", lambda m: "image_encoder.blocks."),
    (r"^vision_encoder\.patch_embed\.projection\.", lambda m: "image_encoder.patch_embed.proj."),
    (r"^vision_encoder\.neck\.(conv1|layer_norm1|conv2|layer_norm2)\.", lambda m: f"image_encoder.neck.{_inv(_NECK)[m[1]]}."),
    (r"^vision_encoder\.", lambda m: "image_encoder."),
    (r"^prompt_encoder\.shared_embedding\.positional_embedding$", lambda m: _GAUSS),
    (r"^prompt_encoder\.point_embed\.", lambda m: "prompt_encoder.point_embeddings."),
    (r"^prompt_encoder\.mask_embed\.(conv1|layer_norm1|conv2|layer_norm2|conv3)\.", lambda m: f"prompt_encoder.mask_downscaling.{_inv(_DOWN)[m[1]]}."),
    (r"^mask_decoder\.(upscale_conv1|upscale_layer_norm|upscale_conv2)\.", lambda m: f"mask_decoder.output_upscaling.{_inv(_UP)[m[1]]}."),
    (r"^mask_decoder\.(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.(proj_in|layers\.0|proj_out)\.", lambda m: f"mask_decoder.{m[1]}.{_MLP_INV[m[2]]}."),
    (r"^mask_decoder\.transformer\.layers\.(\d+)\.layer_norm(\d)\.", lambda m: f"mask_decoder.transformer.layers.{m[1]}.norm{m[2]}."),
    (r"^mask_decoder\.transformer\.layer_norm_final_attn\.", lambda m: "mask_decoder.transformer.norm_final_attn."),
)


def _apply(rules, key):
    for pat, fn in rules:
        m = re.match(pat, key)
        if m:
            return fn(m) + key[m.end():]
    return key


def rename_checkpoint_key(key: str):
    """One key of the original `sam_vit_*.pth` -> its transformers name(s): a list, because the Gaussian matrix of the prompt encoder is
    also the model's `shared_image_embedding`."""
    out = [_apply(_FORWARD, key)]
    if key == _GAUSS:
        out.append("shared_image_embedding.positional_embedding")
    return out


def original_checkpoint_key(key: str):
    """The inverse of `rename_checkpoint_key` (None for `shared_image_embedding`, which the original stores once): it writes a
    transformers state dict in the original naming - the only way the table can be tested without the original package."""
    if key == "shared_image_embedding.positional_embedding":
        return None
    return _apply(_BACKWARD, key)


def rename_checkpoint(sd):
    out = {}
    for k, v in sd.items():
        for n in rename_checkpoint_key(k):
            out[n] = v
    return out


class SamConfig:
    """What the weights do not say: head counts, window size, which layers attend globally, the epsilons."""

    def __init__(self, num_heads=16, window_size=14, global_attn_indexes=(7, 15, 23, 31), layer_norm_eps=1e-6, decoder_heads=8,
                 attention_downsample_rate=2, decoder_layer_norm_eps=1e-6, num_multimask_outputs=3):
        self.num_heads, self.window_size = num_heads, window_size
        self.global_attn_indexes = tuple(global_attn_indexes)
        self.layer_norm_eps, self.decoder_heads = layer_norm_eps, decoder_heads
        self.attention_downsample_rate, self.decoder_layer_norm_eps = attention_downsample_rate, decoder_layer_norm_eps
        self.num_multimask_outputs = num_multimask_outputs

    @classmethod
    def from_dict(cls, cfg: dict):
        v, m = cfg.get("vision_config", {}), cfg.get("mask_decoder_config", {})
        return cls(num_heads=v.get("num_attention_heads", 12), window_size=v.get("window_size", 14),
                   global_attn_indexes=v.get("global_attn_indexes", (2, 5, 8, 11)), layer_norm_eps=v.get("layer_norm_eps", 1e-6),
                   decoder_heads=m.get("num_attention_heads", 8), attention_downsample_rate=m.get("attention_downsample_rate", 2),
                   decoder_layer_norm_eps=m.get("layer_norm_eps", 1e-6), num_multimask_outputs=m.get("num_multimask_outputs", 3))

    @classmethod
    def for_model_type(cls, model_type: str):
        table = {"vit_h": (16, (7, 15, 23, 31)), "vit_l": (16, (5, 11, 17, 23)), "vit_b": (12, (2, 5, 8, 11))}
        if model_type not in table:
            raise ValueError(f"unknown SAM model type {model_type!r} (vit_h, vit_l, vit_b)")
        heads, glob = table[model_type]
        return cls(num_heads=heads, global_attn_indexes=glob)


def window_geometry(size: int, window: int):
    """(padded size, windows per side) of a `size`-token side cut into `window`-token windows, padded at the bottom / right."""
    n = -(-size // window)
    return n * window, n


def resize_rel_pos(table: torch.Tensor, size: int) -> torch.Tensor:
    """A relative-position table [L][d] for a `size`-token side: [2 size - 1][d], resized linearly when L differs (get_rel_pos)."""
    want = 2 * size - 1
    if table.shape[0] == want:
        return table
    t = F.interpolate(table.float().t()[None], size=want, mode="linear")
    return t[0].t().contiguous()


def preprocess_shape(h: int, w: int, long_side: int):
    scale = long_side / max(h, w)
    return int(h * scale + 0.5), int(w * scale + 0.5)


def preprocess_image(image: np.ndarray, long_side: int, image_format: str = "RGB"):
    """`SamPredictor.set_image`'s host side: (resized uint8 frame [h][w][3], padded normalised tensor fp32 [1][3][S][S])."""
    from PIL import Image
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
        raise ValueError("set_image takes a uint8 image [H][W][3]")
    if image_format not in ("RGB", "BGR"):
        raise ValueError(f"image_format must be 'RGB' or 'BGR', got {image_format!r}")
    if image_format == "BGR":
        image = image[..., ::-1]
    nh, nw = preprocess_shape(image.shape[0], image.shape[1], long_side)
    resized = np.asarray(Image.fromarray(np.ascontiguousarray(image)).resize((nw, nh), Image.BILINEAR))
    x = torch.from_numpy(resized.copy()).permute(2, 0, 1).float()
    x = (x - torch.tensor(PIXEL_MEAN).view(3, 1, 1)) / torch.tensor(PIXEL_STD).view(3, 1, 1)
    x = F.pad(x, (0, long_side - nw, 0, long_side - nh))
    return resized, x[None].contiguous()


def scale_points(coords, original_size, long_side: int) -> np.ndarray:
    """Click coordinates (x, y) in the original image -> the resized frame (ResizeLongestSide.apply_coords)."""
    oh, ow = original_size
    nh, nw = preprocess_shape(oh, ow, long_side)
    c = np.array(coords, dtype=np.float64).reshape(-1, 2).copy()
    c[:, 0] *= nw / ow
    c[:, 1] *= nh / oh
    return c.astype(np.float32)


class SamModel:
    def __init__(self, state_dict, config: SamConfig = None, device="cuda:0"):
        self.device = torch.device(device)
        # (a host device is accepted for CONSTRUCTION only - loading / inspecting checkpoints; running refuses it: `_need_gpu`)
        _lib.load()
        self.config = cfg = config or SamConfig()
        sd = {k: v.detach().float().cpu() for k, v in state_dict.items()}
        # one Gaussian matrix under two names: transformers ties them and `save_pretrained` stores `shared_image_embedding` only
        tied = ("shared_image_embedding.positional_embedding", "prompt_encoder.shared_embedding.positional_embedding")
        for a, b in (tied, tied[::-1]):
            if a not in sd and b in sd:
                sd[a] = sd[b]
        self.sd = sd
        dev = self.device
        pw = sd["vision_encoder.patch_embed.projection.weight"]
        self.D, self.patch = pw.shape[0], pw.shape[-1]
        self.grid = sd["vision_encoder.pos_embed"].shape[1]
        self.image_size = self.grid * self.patch
        self.heads = cfg.num_heads
        self.L = 0
        while f"vision_encoder.layers.{self.L}.attn.qkv.weight" in sd:
            self.L += 1
        self.C = sd["vision_encoder.neck.conv1.weight"].shape[0]            # prompt / decoder width
        D, d = self.D, self.D // self.heads
        if d not in (40, 64, 80):
            raise _lib.BlobCtrlHipError(f"SamModel: vision head size {d} has no bc_attention_relpos build (40, 64, 80)")
        h, f = {}, {}
        w = pw.flatten(1)
        self.Kpad = pad8(w.shape[1])
        wp = torch.zeros(D, self.Kpad)
        wp[:, : w.shape[1]] = w
        h["patch.weight"], f["patch.bias"] = wp.half().to(dev), sd["vision_encoder.patch_embed.projection.bias"].to(dev)
        f["pos"] = sd["vision_encoder.pos_embed"].reshape(-1, D).contiguous().to(dev)
        for i in range(self.L):
            p = f"vision_encoder.layers.{i}."
            side = self.grid if i in cfg.global_attn_indexes else cfg.window_size
            qkv_w, qkv_b = sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]
            h[p + "qk.weight"], f[p + "qk.bias"] = qkv_w[: 2 * D].half().to(dev), qkv_b[: 2 * D].contiguous().to(dev)
            h[p + "v.weight"], f[p + "v.bias"] = qkv_w[2 * D:].half().to(dev), qkv_b[2 * D:].contiguous().to(dev)
            h[p + "rel_h"] = resize_rel_pos(sd[p + "attn.rel_pos_h"], side).half().contiguous().to(dev)
            h[p + "rel_w"] = resize_rel_pos(sd[p + "attn.rel_pos_w"], side).half().contiguous().to(dev)
            for nm in ("attn.proj", "mlp.lin1", "mlp.lin2"):
                h[p + nm + ".weight"], f[p + nm + ".bias"] = sd[p + nm + ".weight"].half().to(dev), sd[p + nm + ".bias"].to(dev)
            for nm in ("layer_norm1", "layer_norm2"):
                f[p + nm + ".weight"], f[p + nm + ".bias"] = sd[p + nm + ".weight"].to(dev), sd[p + nm + ".bias"].to(dev)
        n = "vision_encoder.neck."
        h[n + "conv1.weight"] = sd[n + "conv1.weight"].flatten(1).half().to(dev)
        h[n + "conv2.weight"] = pack_conv3x3(sd[n + "conv2.weight"]).half().to(dev)
        for nm in ("layer_norm1", "layer_norm2"):
            f[n + nm + ".weight"], f[n + nm + ".bias"] = sd[n + nm + ".weight"].to(dev), sd[n + nm + ".bias"].to(dev)
        self._pack_decoder(sd, h, f)
        self.h, self.f = h, f
        self._plans = {}
        self.plans_recorded = 0
        # the image the decoder plans read: token-major fp16 embeddings [grid^2][C] of the last `encode`
        self._emb16 = torch.zeros(self.grid * self.grid, self.C, dtype=torch.float16, device=dev)

    def _pack_decoder(self, sd, h, f):
        dev, C = self.device, self.C
        pe, md = "prompt_encoder.", "mask_decoder."
        gauss = sd[pe + "shared_embedding.positional_embedding"]
        self.F = gauss.shape[1]
        if 2 * self.F != C:
            raise ValueError(f"SamModel: num_pos_feats {self.F} must be half the prompt width {C}")
        f["gauss"] = gauss.contiguous().to(dev)
        f["label_embed"] = torch.cat([sd[pe + "point_embed.0.weight"], sd[pe + "point_embed.1.weight"]], 0).contiguous().to(dev)
        f["not_a_point"] = sd[pe + "not_a_point_embed.weight"].reshape(-1).to(dev)
        h["no_mask"] = sd[pe + "no_mask_embed.weight"].reshape(1, C).half().to(dev)
        f["tokens"] = torch.cat([sd[md + "iou_token.weight"], sd[md + "mask_tokens.weight"]], 0).contiguous().to(dev)
        self.ntok = f["tokens"].shape[0]
        # the image positional encoding (get_image_wide_positional_embeddings): a constant of the weights, token-major [grid^2][C]
        g_ = self.grid
        gi = sd["shared_image_embedding.positional_embedding"].double()
        t = (torch.arange(g_, dtype=torch.float64) + 0.5) / g_
        xy = torch.stack([t[None, :].expand(g_, g_), t[:, None].expand(g_, g_)], -1)
        ang = 2 * math.pi * ((2 * xy - 1) @ gi)
        h["image_pe"] = torch.cat([ang.sin(), ang.cos()], -1).reshape(g_ * g_, C).half().to(dev)
        self.dec_layers = 0
        while f"{md}transformer.layers.{self.dec_layers}.self_attn.q_proj.weight" in sd:
            self.dec_layers += 1
        for k, v in sd.items():
            if not k.startswith(md) or "upscale_conv" in k or k.endswith("_token.weight") or k.endswith("_tokens.weight"):
                continue
            key = k[len(md):]
            if v.ndim == 2:
                w = v
                if w.shape[1] % 8:                                   # (a GEMM's K is a multiple of 8: zero columns)
                    w = F.pad(w, (0, pad8(w.shape[1]) - w.shape[1]))
                h[key] = w.half().contiguous().to(dev)
            else:
                f[key] = v.to(dev)
        # ConvTranspose2d(k = 2, s = 2) weight [Cin][Cout][2][2] -> GEMM weight [(dy, dx, co)][ci]; bias repeated per sub-pixel
        for nm in ("upscale_conv1", "upscale_conv2"):
            w = sd[md + nm + ".weight"]
            h[nm + ".weight"] = w.permute(2, 3, 1, 0).reshape(4 * w.shape[1], w.shape[0]).half().contiguous().to(dev)
            f[nm + ".bias"] = sd[md + nm + ".bias"].repeat(4).contiguous().to(dev)

    # ------------------------------------------------------------------------------------------------ loading
    @classmethod
    def from_pretrained(cls, path, device="cuda:0", **_ignored):
        """A transformers directory: config.json + model.safetensors."""
        from .checkpoint import _config, _model_file, read_safetensors
        return cls(read_safetensors(_model_file(path)), SamConfig.from_dict(_config(path)), device=device)

    @classmethod
    def from_checkpoint(cls, path_or_state_dict, model_type="vit_h", device="cuda:0", config: SamConfig = None):
        """The original `sam_vit_h_4b8939.pth` (or its state dict), through the rename table above."""
        sd = path_or_state_dict
        if not isinstance(sd, dict):
            sd = torch.load(sd, map_location="cpu", weights_only=True)
        return cls(rename_checkpoint(sd), config or SamConfig.for_model_type(model_type), device=device)

    def to(self, *a, **k):
        return self

    def _need_gpu(self):
        if self.device.type != "cuda":
            raise _lib.BlobCtrlHipError("blobctrl_amd.SamModel runs on MI355X only; there is no CPU fallback")

    # ------------------------------------------------------------------------------------------------ vision encoder
    def _encoder_plan(self, B):
        self._need_gpu()
        key = ("enc", B)
        if key in self._plans:
            return self._plans[key]
        rec = Recorder(self.device)
        P = type("Plan", (), {})()
        P.rec = rec
        cfg, hw, fw = self.config, self.h, self.f
        D, heads, g_, S, C = self.D, self.heads, self.grid, self.image_size, self.C
        d, T, eps = D // heads, g_ * g_, cfg.layer_norm_eps
        P.pixels = rec.zeros(B, 3, S, S, dtype=torch.float32)
        P.seg = rec.begin("sam_encoder")
        cols = rec.empty(B * T, self.Kpad)
        rec.call("bc_patchify", P.pixels.data_ptr(), B, S, S, self.patch, self.Kpad, cols.data_ptr(), kind="patchify")
        pe = rec.empty(B * T, D)
        rec.gemm(A=cols, W=hw["patch.weight"], M=B * T, N=D, K=self.Kpad, out=pe, bias=fw["patch.bias"], kind="patch_embed")
        x = rec.empty(B * T, D)
        rec.call("bc_add_pos", pe, fw["pos"], B, T, D, x, kind="add_pos", keep=(pe, fw["pos"], x))
        ws = cfg.window_size
        _, nW = window_geometry(g_, ws)
        rel_elems = max(B * heads * T * 2 * g_, B * nW * nW * heads * ws * ws * 2 * ws)
        rel = rec.empty(rel_elems, dtype=torch.float32)
        # One workspace for all layers (they run one after the other on one stream): the residual stream alternates between xa and xb, the
        # windowed and the global form have their own V^T (its zero padding columns are written once, here, and never again).
        Mw = B * nW * nW * ws * ws                                          # rows of the windowed form (padded) >= B * T
        Fm = max(hw[f"vision_encoder.layers.{i}.mlp.lin1.weight"].shape[0] for i in range(self.L))
        xa, xb, ln = x, rec.empty(B * T, D), rec.empty(B * T, D)
        xw_buf, qk_buf, a_buf, pw_buf = rec.empty(Mw, D), rec.empty(Mw, 2 * D), rec.empty(Mw, D), rec.empty(Mw, D)
        m1 = rec.empty(B * T, Fm)
        vt_bufs = {}
        for i in range(self.L):
            p = f"vision_encoder.layers.{i}."
            glob = i in cfg.global_attn_indexes
            x, x2 = (xa, xb)
            rec.layernorm(x, B * T, D, fw[p + "layer_norm1.weight"], fw[p + "layer_norm1.bias"], eps, out=ln)
            if glob:
                xw, Bw, side = ln, B, g_
            else:
                Bw, side = B * nW * nW, ws
                xw = xw_buf
                rec.call("bc_window_partition", ln, B, g_, g_, D, ws, xw, kind="window_partition", keep=(ln, xw))
            N = side * side
            M = Bw * N
            ldvt = (N + 63) // 64 * 64
            qk, a = qk_buf, a_buf
            rec.gemm(A=xw, W=hw[p + "qk.weight"], M=M, N=2 * D, K=D, out=qk, bias=fw[p + "qk.bias"], kind="qkv")
            if glob not in vt_bufs:
                vt_bufs[glob] = rec.zeros(Bw, D, ldvt)
            vt = vt_bufs[glob]
            rec.gemm(A=xw, W=hw[p + "v.weight"], M=M, N=D, K=D, out=vt, bias=fw[p + "v.bias"], out_mode=_lib.OUT_F16_T, ldc=ldvt,
                     rows_per_batch=N, kind="qkv")
            rec.call("bc_attention_relpos", qk.data_ptr(), qk.data_ptr() + 2 * D, vt, a, Bw, heads, d, side, side, side, side, 2 * D, 2 * D,
                     ldvt, D, N * 2 * D, N * 2 * D, D * ldvt, N * D, d ** -0.5, hw[p + "rel_h"], hw[p + "rel_w"], rel, kind="attention_relpos",
                     keep=(qk, vt, a, hw[p + "rel_h"], hw[p + "rel_w"], rel))
            rec.seg.flops += 4 * Bw * heads * N * N * d
            if glob:
                rec.gemm(A=a, W=hw[p + "attn.proj.weight"], M=M, N=D, K=D, out=x2, bias=fw[p + "attn.proj.bias"], R=x, ldr=D, kind="attn_out")
            else:
                pw = pw_buf
                rec.gemm(A=a, W=hw[p + "attn.proj.weight"], M=M, N=D, K=D, out=pw, bias=fw[p + "attn.proj.bias"], kind="attn_out")
                rec.call("bc_window_unpartition", pw, x, B, g_, g_, D, ws, x2, kind="window_unpartition", keep=(pw, x, x2))
            rec.layernorm(x2, B * T, D, fw[p + "layer_norm2.weight"], fw[p + "layer_norm2.bias"], eps, out=ln)
            Fi = hw[p + "mlp.lin1.weight"].shape[0]
            rec.gemm(A=ln, W=hw[p + "mlp.lin1.weight"], M=B * T, N=Fi, K=D, out=m1, bias=fw[p + "mlp.lin1.bias"], act=_lib.ACT_GELU, kind="ff")
            rec.gemm(A=m1, W=hw[p + "mlp.lin2.weight"], M=B * T, N=D, K=Fi, out=x, bias=fw[p + "mlp.lin2.bias"], R=x2, ldr=D, kind="ff")
        n = "vision_encoder.neck."
        n1 = rec.empty(B * T, C)
        rec.gemm(A=x, W=hw[n + "conv1.weight"], M=B * T, N=C, K=D, out=n1, kind="neck")
        l1 = rec.layernorm(n1, B * T, C, fw[n + "layer_norm1.weight"], fw[n + "layer_norm1.bias"], 1e-6)
        n2 = rec.empty(B * T, C)
        rec.gemm(A=l1, W=hw[n + "conv2.weight"], M=B * T, N=C, K=9 * C, out=n2, rows_per_batch=T, kind="neck",
                 conv=dict(Cin=C, Hin=g_, Win=g_, Hout=g_, Wout=g_, stride=1))
        P.emb16 = rec.layernorm(n2, B * T, C, fw[n + "layer_norm2.weight"], fw[n + "layer_norm2.bias"], 1e-6)
        P.emb = rec.empty(B, C, g_, g_, dtype=torch.float32)
        rec.call("bc_nhwc_to_nchw", P.emb16, B, C, T, C, P.emb, 1, kind="to_nchw", keep=(P.emb16, P.emb))
        self._plans[key] = P
        self.plans_recorded += 1
        return P

    @torch.no_grad()
    def encode(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """pixel_values [B][3][S][S] (normalised, zero padded) -> image_embeddings [B][C][grid][grid] fp32.  The embeddings of image 0
        stay in the model for `decode`."""
        B, Cc, H, W = pixel_values.shape
        if Cc != 3 or H != self.image_size or W != self.image_size:
            raise ValueError(f"pixel_values must be [B][3][{self.image_size}][{self.image_size}]")
        P = self._encoder_plan(B)
        P.pixels.copy_(pixel_values.to(self.device, torch.float32))
        run_graphed(P.seg, self.device)
        T = self.grid * self.grid
        self._emb16.copy_(P.emb16.view(B, T, self.C)[0])
        return P.emb.clone()

    # ------------------------------------------------------------------------------------------------ prompt encoder + mask decoder
    def _attn(self, rec, name, xq, nq, xk, xv, nk, R=None):
        """SamAttention: out_proj(attention(q_proj xq, k_proj xk, v_proj xv)) [+ R] -> [nq][C]."""
        hw, fw, C, heads = self.h, self.f, self.C, self.config.decoder_heads
        inner = hw[name + "q_proj.weight"].shape[0]
        d = inner // heads
        q, k = rec.empty(nq, inner), rec.empty(nk, inner)
        rec.gemm(A=xq, W=hw[name + "q_proj.weight"], M=nq, N=inner, K=C, out=q, bias=fw[name + "q_proj.bias"], kind="dec_qkv")
        rec.gemm(A=xk, W=hw[name + "k_proj.weight"], M=nk, N=inner, K=C, out=k, bias=fw[name + "k_proj.bias"], kind="dec_qkv")
        ldvt = (nk + 63) // 64 * 64
        vt = rec.zeros(1, inner, ldvt)
        rec.gemm(A=xv, W=hw[name + "v_proj.weight"], M=nk, N=inner, K=C, out=vt, bias=fw[name + "v_proj.bias"], out_mode=_lib.OUT_F16_T,
                 ldc=ldvt, rows_per_batch=nk, kind="dec_qkv")
        a = rec.empty(nq, inner)
        rec.attention(q, k, vt, a, 1, heads, d, nq, nk, inner, inner, ldvt, inner, nq * inner, nk * inner, inner * ldvt, nq * inner, d ** -0.5)
        out = rec.empty(nq, C)
        kw = dict(R=R, ldr=C) if R is not None else {}
        rec.gemm(A=a, W=hw[name + "out_proj.weight"], M=nq, N=C, K=inner, out=out, bias=fw[name + "out_proj.bias"], kind="dec_out", **kw)
        return out

    def _add(self, rec, a, b, rows, b_rows=None):
        out = rec.empty(rows, self.C)
        rec.call("bc_add_rows", a, b, rows, b_rows or rows, self.C, out, kind="add_rows", keep=(a, b, out))
        return out

    def _mlp3(self, rec, name, x, x_off, out, out_off, n_out, out_mode=_lib.OUT_F16):
        """SamFeedForward on ONE token row: proj_in -> ReLU -> layers.0 -> ReLU -> proj_out."""
        hw, fw = self.h, self.f
        Hd = hw[name + "proj_in.weight"].shape[0]
        t1, t2 = rec.zeros(1, pad8(Hd)), rec.zeros(1, pad8(Hd))
        rec.gemm(A=x, a_offset=x_off, W=hw[name + "proj_in.weight"], M=1, N=Hd, K=self.C, out=t1, bias=fw[name + "proj_in.bias"], kind="dec_mlp")
        rec.call("bc_act_rows", t1, pad8(Hd), 1, kind="relu", keep=t1)
        rec.gemm(A=t1, W=hw[name + "layers.0.weight"], M=1, N=Hd, K=pad8(Hd), out=t2, bias=fw[name + "layers.0.bias"], kind="dec_mlp")
        rec.call("bc_act_rows", t2, pad8(Hd), 1, kind="relu", keep=t2)
        rec.gemm(A=t2, W=hw[name + "proj_out.weight"], M=1, N=n_out, K=pad8(Hd), out=out, out_offset=out_off, out_mode=out_mode,
                 bias=fw[name + "proj_out.bias"], kind="dec_mlp")

    def _decoder_plan(self, npts):
        self._need_gpu()
        key = ("dec", npts)
        if key in self._plans:
            return self._plans[key]
        rec = Recorder(self.device)
        P = type("Plan", (), {})()
        P.rec = rec
        cfg, hw, fw = self.config, self.h, self.f
        C, g_, ntok = self.C, self.grid, self.ntok
        T, nq, eps = g_ * g_, ntok + npts + 1, cfg.decoder_layer_norm_eps
        P.points = rec.zeros(npts, 2, dtype=torch.float32)
        P.labels = rec.zeros(npts, dtype=torch.int32)
        P.seg = rec.begin("sam_decoder")
        qpe = rec.empty(nq, C)
        rec.call("bc_sam_tokens", fw["tokens"], ntok, P.points, P.labels, npts, fw["gauss"], self.F, fw["label_embed"], fw["not_a_point"],
                 float(self.image_size), qpe, kind="sam_tokens", keep=(fw["tokens"], fw["gauss"], fw["label_embed"], fw["not_a_point"], qpe))
        kpe = hw["image_pe"]
        keys = self._add(rec, self._emb16, hw["no_mask"], T, 1)              # image embeddings + the dense "no mask" embedding
        queries = qpe
        for i in range(self.dec_layers):
            p = f"transformer.layers.{i}."
            if i == 0:                                                       # (skip_first_layer_pe: no positional encoding, no residual)
                queries = self._attn(rec, p + "self_attn.", queries, nq, queries, queries, nq)
            else:
                qq = self._add(rec, queries, qpe, nq)
                queries = self._attn(rec, p + "self_attn.", qq, nq, qq, queries, nq, R=queries)
            queries = rec.layernorm(queries, nq, C, fw[p + "layer_norm1.weight"], fw[p + "layer_norm1.bias"], eps)
            qq, kk = self._add(rec, queries, qpe, nq), self._add(rec, keys, kpe, T)
            queries = self._attn(rec, p + "cross_attn_token_to_image.", qq, nq, kk, keys, T, R=queries)
            queries = rec.layernorm(queries, nq, C, fw[p + "layer_norm2.weight"], fw[p + "layer_norm2.bias"], eps)
            Fm = hw[p + "mlp.lin1.weight"].shape[0]
            m1 = rec.empty(nq, Fm)
            rec.gemm(A=queries, W=hw[p + "mlp.lin1.weight"], M=nq, N=Fm, K=C, out=m1, bias=fw[p + "mlp.lin1.bias"], kind="dec_mlp")
            rec.call("bc_act_rows", m1, nq * Fm, 1, kind="relu", keep=m1)
            m2 = rec.empty(nq, C)
            rec.gemm(A=m1, W=hw[p + "mlp.lin2.weight"], M=nq, N=C, K=Fm, out=m2, bias=fw[p + "mlp.lin2.bias"], R=queries, ldr=C, kind="dec_mlp")
            queries = rec.layernorm(m2, nq, C, fw[p + "layer_norm3.weight"], fw[p + "layer_norm3.bias"], eps)
            qq = self._add(rec, queries, qpe, nq)
            k2 = self._attn(rec, p + "cross_attn_image_to_token.", kk, T, qq, queries, nq, R=keys)
            keys = rec.layernorm(k2, T, C, fw[p + "layer_norm4.weight"], fw[p + "layer_norm4.bias"], eps)
        qq, kk = self._add(rec, queries, qpe, nq), self._add(rec, keys, kpe, T)
        queries = self._attn(rec, "transformer.final_attn_token_to_image.", qq, nq, kk, keys, T, R=queries)
        queries = rec.layernorm(queries, nq, C, fw["transformer.layer_norm_final_attn.weight"], fw["transformer.layer_norm_final_attn.bias"], 1e-5)
        # upscaler: the sub-pixels of both transposed convolutions stay GEMM rows until bc_sam_masks places them
        C1, C2 = C // 4, C // 8
        u1 = rec.empty(T, 4 * C1)
        rec.gemm(A=keys, W=hw["upscale_conv1.weight"], M=T, N=4 * C1, K=C, out=u1, bias=fw["upscale_conv1.bias"], kind="upscale")
        l1 = rec.layernorm(u1, 4 * T, C1, fw["upscale_layer_norm.weight"], fw["upscale_layer_norm.bias"], 1e-6)
        rec.call("bc_act_rows", l1, 4 * T * C1, 0, kind="gelu", keep=l1)
        u2 = rec.empty(4 * T, 4 * C2)
        rec.gemm(A=l1, W=hw["upscale_conv2.weight"], M=4 * T, N=4 * C2, K=C1, out=u2, bias=fw["upscale_conv2.bias"], act=_lib.ACT_GELU,
                 kind="upscale")
        ldh = pad8(C2)
        hyper = rec.zeros(ntok - 1, ldh)
        for t in range(ntok - 1):
            self._mlp3(rec, f"output_hypernetworks_mlps.{t}.", queries, (1 + t) * C, hyper, t * ldh, C2)
        P.iou = rec.zeros(1, ntok - 1, dtype=torch.float32)
        self._mlp3(rec, "iou_prediction_head.", queries, 0, P.iou, 0, ntok - 1, out_mode=_lib.OUT_F32)
        P.masks = rec.empty(1, ntok - 1, 4 * g_, 4 * g_, dtype=torch.float32)
        rec.call("bc_sam_masks", u2, C2, hyper, ldh, 1, g_, g_, ntok - 1, P.masks, kind="sam_masks", keep=(u2, hyper, P.masks))
        self._plans[key] = P
        self.plans_recorded += 1
        return P

    @torch.no_grad()
    def decode(self, points, labels, multimask_output=True):
        """Point prompts on the image of the last `encode` (coordinates in the model's input frame) -> (low-res logits [n][4 grid][4 grid],
        IoU scores [n]) fp32 on the device; n = 1 (mask token 0), the multimask tokens, or all of them (multimask_output=None)."""
        pts = torch.as_tensor(np.asarray(points, dtype=np.float32)).reshape(-1, 2)
        lab = torch.as_tensor(np.asarray(labels)).reshape(-1).to(torch.int32)
        if pts.shape[0] == 0 or pts.shape[0] != lab.shape[0]:
            raise ValueError("decode needs n >= 1 points [n][2] and n labels")
        P = self._decoder_plan(pts.shape[0])
        P.points.copy_(pts.to(self.device))
        P.labels.copy_(lab.to(self.device))
        run_graphed(P.seg, self.device)
        sel = slice(None) if multimask_output is None else slice(1, None) if multimask_output else slice(0, 1)
        return P.masks[0, sel].clone(), P.iou[0, sel].clone()

    # ------------------------------------------------------------------------------------------------ batched prompts
    def _attn_batch(self, rec, name, Bp, xq, nq, q_shared, xk, xv, nk, kv_shared, R=None):
        """`_attn` over Bp prompts: xq [Bp][nq][C], xk / xv [Bp][nk][C] -> [Bp][nq][C].  A side that is the same for every prompt
        (`q_shared` / `kv_shared`: [nq][C] / [nk][C]) is projected once and the attention reads it with a batch stride of 0."""
        hw, fw, C, heads = self.h, self.f, self.C, self.config.decoder_heads
        inner = hw[name + "q_proj.weight"].shape[0]
        d = inner // heads
        Bq, Bk = 1 if q_shared else Bp, 1 if kv_shared else Bp
        q, k = rec.empty(Bq * nq, inner), rec.empty(Bk * nk, inner)
        rec.gemm(A=xq, W=hw[name + "q_proj.weight"], M=Bq * nq, N=inner, K=C, out=q, bias=fw[name + "q_proj.bias"], kind="dec_qkv")
        rec.gemm(A=xk, W=hw[name + "k_proj.weight"], M=Bk * nk, N=inner, K=C, out=k, bias=fw[name + "k_proj.bias"], kind="dec_qkv")
        ldvt = (nk + 63) // 64 * 64
        vt = rec.zeros(Bk, inner, ldvt)
        rec.gemm(A=xv, W=hw[name + "v_proj.weight"], M=Bk * nk, N=inner, K=C, out=vt, bias=fw[name + "v_proj.bias"], out_mode=_lib.OUT_F16_T,
                 ldc=ldvt, rows_per_batch=nk, kind="dec_qkv")
        a = rec.empty(Bp * nq, inner)
        rec.attention(q, k, vt, a, Bp, heads, d, nq, nk, inner, inner, ldvt, inner, 0 if q_shared else nq * inner, 0 if kv_shared else nk * inner,
                      0 if kv_shared else inner * ldvt, nq * inner, d ** -0.5)
        out = rec.empty(Bp * nq, C)
        kw = dict(R=R, ldr=C) if R is not None else {}
        rec.gemm(A=a, W=hw[name + "out_proj.weight"], M=Bp * nq, N=C, K=inner, out=out, bias=fw[name + "out_proj.bias"], kind="dec_out", **kw)
        return out

    def _mlp3_batch(self, rec, name, Bp, x, x_off, ldx, out, out_off, ldo, n_out, out_mode=_lib.OUT_F16):
        """`_mlp3` on the same token row of Bp prompts: rows x[b * ldx + x_off ...] -> out[b * ldo + out_off ...]."""
        hw, fw = self.h, self.f
        Hd = hw[name + "proj_in.weight"].shape[0]
        Hp = pad8(Hd)
        t1, t2 = rec.zeros(Bp, Hp), rec.zeros(Bp, Hp)
        rec.gemm(A=x, a_offset=x_off, lda=ldx, W=hw[name + "proj_in.weight"], M=Bp, N=Hd, K=self.C, out=t1, ldc=Hp, bias=fw[name + "proj_in.bias"],
                 kind="dec_mlp")
        rec.call("bc_act_rows", t1, Bp * Hp, 1, kind="relu", keep=t1)
        rec.gemm(A=t1, W=hw[name + "layers.0.weight"], M=Bp, N=Hd, K=Hp, out=t2, ldc=Hp, bias=fw[name + "layers.0.bias"], kind="dec_mlp")
        rec.call("bc_act_rows", t2, Bp * Hp, 1, kind="relu", keep=t2)
        rec.gemm(A=t2, W=hw[name + "proj_out.weight"], M=Bp, N=n_out, K=Hp, out=out, out_offset=out_off, ldc=ldo, out_mode=out_mode,
                 bias=fw[name + "proj_out.bias"], kind="dec_mlp")

    def _decoder_plan_batch(self, Bp, npts):
        """`_decoder_plan` for Bp prompt sets of npts points on the one image of the last `encode`: the same launches in the same order over
        [Bp][nq][C] token rows and, from the first cross_attn_image_to_token on, [Bp][T][C] image rows.  Until then the image side is the
        same for every prompt - embedding + no_mask, + image_pe, layer 0's K / V (and the image-to-token Q) projections - and exists once."""
        self._need_gpu()
        key = ("dec_batch", Bp, npts)
        if key in self._plans:
            return self._plans[key]
        if self.dec_layers < 1:
            raise ValueError("SamModel: the batched decoder needs at least one two-way transformer layer")
        rec = Recorder(self.device)
        P = type("Plan", (), {})()
        P.rec = rec
        cfg, hw, fw = self.config, self.h, self.f
        C, g_, ntok = self.C, self.grid, self.ntok
        T, nq, eps = g_ * g_, ntok + npts + 1, cfg.decoder_layer_norm_eps
        P.points = rec.zeros(Bp, npts, 2, dtype=torch.float32)
        P.labels = rec.zeros(Bp, npts, dtype=torch.int32)
        P.seg = rec.begin("sam_decoder_batch")
        qpe = rec.empty(Bp * nq, C)
        rec.call("bc_sam_tokens_batch", fw["tokens"], ntok, P.points, P.labels, Bp, npts, fw["gauss"], self.F, fw["label_embed"], fw["not_a_point"],
                 float(self.image_size), qpe, kind="sam_tokens", keep=(fw["tokens"], fw["gauss"], fw["label_embed"], fw["not_a_point"], qpe))
        kpe = hw["image_pe"]
        keys, shared = self._add(rec, self._emb16, hw["no_mask"], T, 1), True    # [T][C] while `shared`, [Bp][T][C] afterwards
        queries = qpe
        for i in range(self.dec_layers):
            p = f"transformer.layers.{i}."
            if i == 0:
                queries = self._attn_batch(rec, p + "self_attn.", Bp, queries, nq, False, queries, queries, nq, False)
            else:
                qq = self._add(rec, queries, qpe, Bp * nq)
                queries = self._attn_batch(rec, p + "self_attn.", Bp, qq, nq, False, qq, queries, nq, False, R=queries)
            queries = rec.layernorm(queries, Bp * nq, C, fw[p + "layer_norm1.weight"], fw[p + "layer_norm1.bias"], eps)
            krows = T if shared else Bp * T
            qq, kk = self._add(rec, queries, qpe, Bp * nq), self._add(rec, keys, kpe, krows, T)
            queries = self._attn_batch(rec, p + "cross_attn_token_to_image.", Bp, qq, nq, False, kk, keys, T, shared, R=queries)
            queries = rec.layernorm(queries, Bp * nq, C, fw[p + "layer_norm2.weight"], fw[p + "layer_norm2.bias"], eps)
            Fm = hw[p + "mlp.lin1.weight"].shape[0]
            m1 = rec.empty(Bp * nq, Fm)
            rec.gemm(A=queries, W=hw[p + "mlp.lin1.weight"], M=Bp * nq, N=Fm, K=C, out=m1, bias=fw[p + "mlp.lin1.bias"], kind="dec_mlp")
            rec.call("bc_act_rows", m1, Bp * nq * Fm, 1, kind="relu", keep=m1)
            m2 = rec.empty(Bp * nq, C)
            rec.gemm(A=m1, W=hw[p + "mlp.lin2.weight"], M=Bp * nq, N=C, K=Fm, out=m2, bias=fw[p + "mlp.lin2.bias"], R=queries, ldr=C, kind="dec_mlp")
            queries = rec.layernorm(m2, Bp * nq, C, fw[p + "layer_norm3.weight"], fw[p + "layer_norm3.bias"], eps)
            qq = self._add(rec, queries, qpe, Bp * nq)
            if shared:
                # the residual is the one shared [T][C] block under Bp blocks of output rows: a GEMM epilogue reads R row for row, so the add
                # is its own launch here (one more fp16 rounding than the single-prompt plan's fused residual, in this layer only)
                k2 = self._attn_batch(rec, p + "cross_attn_image_to_token.", Bp, kk, T, True, qq, queries, nq, False)
                k2 = self._add(rec, k2, keys, Bp * T, T)
            else:
                k2 = self._attn_batch(rec, p + "cross_attn_image_to_token.", Bp, kk, T, False, qq, queries, nq, False, R=keys)
            keys, shared = rec.layernorm(k2, Bp * T, C, fw[p + "layer_norm4.weight"], fw[p + "layer_norm4.bias"], eps), False
        qq, kk = self._add(rec, queries, qpe, Bp * nq), self._add(rec, keys, kpe, Bp * T, T)
        queries = self._attn_batch(rec, "transformer.final_attn_token_to_image.", Bp, qq, nq, False, kk, keys, T, False, R=queries)
        queries = rec.layernorm(queries, Bp * nq, C, fw["transformer.layer_norm_final_attn.weight"], fw["transformer.layer_norm_final_attn.bias"], 1e-5)
        C1, C2 = C // 4, C // 8
        u1 = rec.empty(Bp * T, 4 * C1)
        rec.gemm(A=keys, W=hw["upscale_conv1.weight"], M=Bp * T, N=4 * C1, K=C, out=u1, bias=fw["upscale_conv1.bias"], kind="upscale")
        l1 = rec.layernorm(u1, 4 * Bp * T, C1, fw["upscale_layer_norm.weight"], fw["upscale_layer_norm.bias"], 1e-6)
        rec.call("bc_act_rows", l1, 4 * Bp * T * C1, 0, kind="gelu", keep=l1)
        u2 = rec.empty(4 * Bp * T, 4 * C2)
        rec.gemm(A=l1, W=hw["upscale_conv2.weight"], M=4 * Bp * T, N=4 * C2, K=C1, out=u2, bias=fw["upscale_conv2.bias"], act=_lib.ACT_GELU,
                 kind="upscale")
        ldh = pad8(C2)
        hyper = rec.zeros(Bp, ntok - 1, ldh)
        for t in range(ntok - 1):
            self._mlp3_batch(rec, f"output_hypernetworks_mlps.{t}.", Bp, queries, (1 + t) * C, nq * C, hyper, t * ldh, (ntok - 1) * ldh, C2)
        P.iou = rec.zeros(Bp, ntok - 1, dtype=torch.float32)
        self._mlp3_batch(rec, "iou_prediction_head.", Bp, queries, 0, nq * C, P.iou, 0, ntok - 1, ntok - 1, out_mode=_lib.OUT_F32)
        P.masks = rec.empty(Bp, ntok - 1, 4 * g_, 4 * g_, dtype=torch.float32)
        rec.call("bc_sam_masks", u2, C2, hyper, ldh, Bp, g_, g_, ntok - 1, P.masks, kind="sam_masks", keep=(u2, hyper, P.masks))
        self._plans[key] = P
        self.plans_recorded += 1
        return P

    @torch.no_grad()
    def decode_batch(self, points, labels, multimask_output=True):
        """Bp prompt sets at once on the image of the last `encode`: points [Bp][npts][2] (input frame), labels [Bp][npts] - device tensors or
        anything `torch.as_tensor` takes - -> (low-res logits [Bp][n][4 grid][4 grid], IoU scores [Bp][n]) fp32 on the device, n as in
        `decode`.  One graph replay per call; a plan per (Bp, npts) is recorded on first use and kept."""
        pts = torch.as_tensor(points, dtype=torch.float32) if not torch.is_tensor(points) else points.to(torch.float32)
        lab = torch.as_tensor(labels) if not torch.is_tensor(labels) else labels
        if pts.ndim != 3 or pts.shape[2] != 2 or pts.shape[0] == 0 or pts.shape[1] == 0 or tuple(lab.shape) != tuple(pts.shape[:2]):
            raise ValueError("decode_batch needs points [Bp][npts][2] and labels [Bp][npts] with Bp, npts >= 1")
        P = self._decoder_plan_batch(pts.shape[0], pts.shape[1])
        P.points.copy_(pts.to(self.device))
        P.labels.copy_(lab.to(self.device, torch.int32))
        run_graphed(P.seg, self.device)
        sel = slice(None) if multimask_output is None else slice(1, None) if multimask_output else slice(0, 1)
        return P.masks[:, sel].clone(), P.iou[:, sel].clone()

    @torch.no_grad()
    def mask_stats(self, logits, threshold=0.0, offset=1.0):
        """bc_mask_stats (include/blobctrl_sam.h): logits fp32 [n][H][W] on the device -> int32 [n][7] = count(v > t + o), count(v > t - o),
        count(v > t), and the inclusive box x0, y0, x1, y1 of v > t (zeros for an empty mask)."""
        self._need_gpu()
        lib = _lib.load()
        if logits.ndim != 3 or logits.shape[0] == 0:
            raise ValueError("mask_stats takes logits [n][H][W] with n >= 1")
        src = logits.to(self.device, torch.float32).contiguous()
        n, H, W = src.shape
        chunks = lib.bc_mask_stats_chunks(H, W)
        if chunks <= 0:
            raise ValueError(f"mask_stats: a mask of {H} x {W} is too large")
        partial = torch.empty(n, chunks, 7, dtype=torch.int32, device=self.device)
        out = torch.empty(n, 7, dtype=torch.int32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(lib.bc_mask_stats(src.data_ptr(), n, H, W, float(threshold), float(offset), partial.data_ptr(), out.data_ptr(), stream),
                   "bc_mask_stats")
        return out

    @torch.no_grad()
    def postprocess(self, low_res, input_size, original_size, return_logits=False, threshold=0.0):
        """low-res logits [n][h][w] -> the padded frame (bilinear) -> crop the unpadded region -> the original size; bool unless
        return_logits."""
        self._need_gpu()
        lib, S = _lib.load(), self.image_size
        n, h, w = low_res.shape
        src = low_res.to(self.device, torch.float32).contiguous()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        full = torch.empty(n, S, S, dtype=torch.float32, device=self.device)
        _lib.check(lib.bc_bilinear_resize_f32(src.data_ptr(), n, h, w, h, w, S, S, 0, 0.0, full.data_ptr(), stream), "bc_bilinear_resize_f32")
        out = torch.empty(n, original_size[0], original_size[1], dtype=torch.float32 if return_logits else torch.uint8, device=self.device)
        _lib.check(lib.bc_bilinear_resize_f32(full.data_ptr(), n, S, S, input_size[0], input_size[1], original_size[0], original_size[1],
                                              0 if return_logits else 1, float(threshold), out.data_ptr(), stream), "bc_bilinear_resize_f32")
        return out if return_logits else out.bool()


class ResizeLongestSide:
    """`segment_anything.utils.transforms.ResizeLongestSide` for coordinates: plain scaling by new / old of `preprocess_shape`."""

    def __init__(self, target_length: int):
        self.target_length = int(target_length)

    @staticmethod
    def get_preprocess_shape(oldh: int, oldw: int, long_side_length: int):
        return preprocess_shape(oldh, oldw, long_side_length)

    def apply_coords(self, coords, original_size) -> np.ndarray:
        """(x, y) in the original image [...][2] -> the resized frame, fp32 (the arithmetic of `scale_points`)."""
        c = np.asarray(coords)
        return scale_points(c, original_size, self.target_length).reshape(c.shape)

    def apply_coords_torch(self, coords: torch.Tensor, original_size) -> torch.Tensor:
        oh, ow = original_size
        nh, nw = preprocess_shape(oh, ow, self.target_length)
        scale = torch.tensor([nw / ow, nh / oh], dtype=torch.float64, device=coords.device)
        return (coords.to(torch.float64) * scale).to(torch.float32)


class SamPredictor:
    """The `segment_anything.SamPredictor` surface on a `SamModel`: `predict` (the call the reference app makes) and `predict_torch`."""

    def __init__(self, model: SamModel):
        self.model = model
        self.transform = ResizeLongestSide(model.image_size)
        self.reset_image()

    def reset_image(self):
        self.is_image_set = False
        self.features = None
        self.original_size = self.input_size = None

    def set_image(self, image, image_format: str = "RGB"):
        """image uint8 [H][W][3]: a numpy array, preprocessed on the host (`preprocess_image`), or a device tensor, preprocessed where it is
        (`resample.sam_pixel_values`: the same bytes, and the image never comes to the host)."""
        if torch.is_tensor(image) and image.is_cuda:
            from .resample import sam_pixel_values
            input_size, x = sam_pixel_values(image, self.model.image_size, image_format)
            original_size = tuple(int(v) for v in image.shape[:2])
        else:
            resized, x = preprocess_image(image, self.model.image_size, image_format)
            original_size, input_size = tuple(np.asarray(image).shape[:2]), tuple(resized.shape[:2])
        self.reset_image()
        self.original_size, self.input_size = original_size, input_size
        self.features = self.model.encode(x)
        self.model._emb_owner = id(self)
        self.is_image_set = True

    def get_image_embedding(self) -> torch.Tensor:
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) to generate an embedding.")
        return self.features

    def predict(self, point_coords=None, point_labels=None, box=None, mask_input=None, multimask_output=True, return_logits=False):
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        if box is not None:
            raise NotImplementedError("SamPredictor.predict: box prompts are not implemented (the app passes points only)")
        if mask_input is not None:
            raise NotImplementedError("SamPredictor.predict: mask_input prompts are not implemented (the app passes points only)")
        if point_coords is None or point_labels is None:
            raise ValueError("SamPredictor.predict needs point_coords and point_labels")
        if getattr(self.model, "_emb_owner", None) != id(self):
            raise RuntimeError("another SamPredictor has set an image on this model since: call set_image again")
        pts = scale_points(point_coords, self.original_size, self.model.image_size)
        low, iou = self.model.decode(pts, point_labels, multimask_output)
        masks = self.model.postprocess(low, self.input_size, self.original_size, return_logits=return_logits)
        return masks.cpu().numpy(), iou.cpu().numpy(), low.cpu().numpy()

    @torch.no_grad()
    def predict_torch(self, point_coords, point_labels, boxes=None, mask_input=None, multimask_output=True, return_logits=False):
        """B prompts at once, device tensors in and out: point_coords [B][N][2] ALREADY in the input frame (`transform.apply_coords_torch`),
        point_labels [B][N] -> (masks [B][C][H][W] bool - fp32 logits with return_logits -, IoU [B][C], low-res logits [B][C][4 g][4 g])."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        if boxes is not None:
            raise NotImplementedError("SamPredictor.predict_torch: box prompts are not implemented (points only)")
        if mask_input is not None:
            raise NotImplementedError("SamPredictor.predict_torch: mask_input prompts are not implemented (points only)")
        if point_coords is None or point_labels is None:
            raise ValueError("SamPredictor.predict_torch needs point_coords and point_labels")
        if getattr(self.model, "_emb_owner", None) != id(self):
            raise RuntimeError("another SamPredictor has set an image on this model since: call set_image again")
        return self._predict_batch(point_coords, point_labels, multimask_output, return_logits)

    def _predict_batch(self, point_coords, point_labels, multimask_output, return_logits, mark=None):
        """The device work of `predict_torch`; `mark()` is called between the decoder replay and the resizes (the generator's timing)."""
        low, iou = self.model.decode_batch(point_coords, point_labels, multimask_output)
        if mark is not None:
            mark()
        B, n = iou.shape
        masks = self.model.postprocess(low.flatten(0, 1), self.input_size, self.original_size, return_logits=return_logits)
        return masks.view(B, n, *masks.shape[1:]), iou, low


def box_nms(boxes_xyxy, scores, iou_threshold: float) -> np.ndarray:
    """torchvision.ops.nms on the host: indices of the kept boxes, by descending score (ties: the lower index first).  Area is
    (x2 - x1)(y2 - y1) without + 1; a box is suppressed when its IoU with a kept, better box is > iou_threshold; a NaN IoU (two boxes of zero
    area) suppresses nothing."""
    b = np.asarray(boxes_xyxy, dtype=np.float32).reshape(-1, 4)
    sc = np.asarray(scores, dtype=np.float32).reshape(-1)
    if len(b) != len(sc):
        raise ValueError("box_nms needs one score per box")
    order = np.argsort(-sc, kind="stable")
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = np.zeros(len(b), dtype=bool)
    keep = []
    for pos, i in enumerate(order):
        if dead[i]:
            continue
        keep.append(int(i))
        rest = order[pos + 1:]
        w = np.clip(np.minimum(b[i, 2], b[rest, 2]) - np.maximum(b[i, 0], b[rest, 0]), 0, None)
        h = np.clip(np.minimum(b[i, 3], b[rest, 3]) - np.maximum(b[i, 1], b[rest, 1]), 0, None)
        inter = w * h
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = inter / (area[i] + area[rest] - inter)
        dead[rest[iou > iou_threshold]] = True                      # (NaN > x is False)
    return np.asarray(keep, dtype=np.int64)


def build_point_grid(n_per_side: int) -> np.ndarray:
    """`segment_anything.utils.amg.build_point_grid`: n x n points in [0, 1]^2 at offset 1 / (2 n), x fastest, float64 [n * n][2]."""
    offset = 1 / (2 * n_per_side)
    side = np.linspace(offset, 1 - offset, n_per_side)
    return np.stack([np.tile(side[None, :], (n_per_side, 1)), np.tile(side[:, None], (1, n_per_side))], -1).reshape(-1, 2)


class SamAutomaticMaskGenerator:
    """`segment_anything.SamAutomaticMaskGenerator` on a `SamModel`, whole-image crop only: a grid of single-point prompts through the
    batched decoder, the predicted-IoU and stability filters from one bc_mask_stats pass over the full-size logits, box NMS on the host."""

    def __init__(self, model: SamModel, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.88, stability_score_thresh=0.95,
                 stability_score_offset=1.0, box_nms_thresh=0.7, crop_n_layers=0, crop_nms_thresh=0.7, crop_overlap_ratio=512 / 1500,
                 crop_n_points_downscale_factor=1, point_grids=None, min_mask_region_area=0, output_mode="binary_mask"):
        if (points_per_side is None) == (point_grids is None):
            raise ValueError("Exactly one of points_per_side or point_grid must be provided.")
        if crop_n_layers > 0:
            raise NotImplementedError("SamAutomaticMaskGenerator: crop_n_layers > 0 is not implemented (the whole-image crop only)")
        if min_mask_region_area > 0:
            raise NotImplementedError("SamAutomaticMaskGenerator: min_mask_region_area is a per-call argument here - generate(image, "
                                      "min_mask_region_area=N) - or the method postprocess_small_regions; the constructor takes 0 only")
        if output_mode != "binary_mask":
            raise NotImplementedError(f"SamAutomaticMaskGenerator: output_mode {output_mode!r} is not implemented ('binary_mask' only)")
        if points_per_batch < 1:
            raise ValueError("points_per_batch must be >= 1")
        self.point_grids = [build_point_grid(points_per_side)] if point_grids is None else [np.asarray(g_, dtype=np.float64) for g_ in point_grids]
        self.predictor = SamPredictor(model)
        self.points_per_batch = int(points_per_batch)
        self.pred_iou_thresh, self.stability_score_thresh = pred_iou_thresh, stability_score_thresh
        self.stability_score_offset, self.box_nms_thresh = stability_score_offset, box_nms_thresh
        self.mask_threshold = 0.0
        self.crop_n_layers, self.crop_nms_thresh, self.crop_overlap_ratio = crop_n_layers, crop_nms_thresh, crop_overlap_ratio
        self.crop_n_points_downscale_factor, self.min_mask_region_area, self.output_mode = crop_n_points_downscale_factor, min_mask_region_area, output_mode
        self.last_timing = {}

    @torch.no_grad()
    def generate(self, image, min_mask_region_area=0):
        """image uint8 [H][W][3] (a numpy array or a device tensor: it only goes to `set_image`) -> a list of dicts (segmentation, area, bbox XYWH, predicted_iou, point_coords, stability_score, crop_box) in NMS
        order, i.e. by descending predicted IoU.  A ragged last batch runs a decoder plan of its own size (recorded once, like the full one).
        `last_timing` holds HIP-event milliseconds of the call's phases (decode, resize, stats, regions) and the host time around them.
        `min_mask_region_area` > 0 is the package's post-processing of the kept masks, on the device before any mask crosses to the host
        (`_small_regions`): the order is then unchanged masks first, each group in its NMS order."""
        import time
        if min_mask_region_area < 0:
            raise ValueError("generate: min_mask_region_area must be >= 0")
        pred, model, dev = self.predictor, self.predictor.model, self.predictor.model.device
        t_start = time.perf_counter()
        pred.set_image(image)
        torch.cuda.synchronize(dev)
        t_set = time.perf_counter()
        H, W = pred.original_size
        grid = self.point_grids[0] * np.array([[W, H]], dtype=np.float64)               # (x, y) in the original image
        pts_in = torch.from_numpy(pred.transform.apply_coords(grid, pred.original_size)).to(dev)
        ev = lambda: torch.cuda.Event(enable_timing=True)
        marks, kept = [], []
        for lo in range(0, len(grid), self.points_per_batch):
            hi = min(len(grid), lo + self.points_per_batch)
            e = [ev() for _ in range(4)]
            e[0].record()
            logits, iou, _ = pred._predict_batch(pts_in[lo:hi, None, :], torch.ones(hi - lo, 1, dtype=torch.int32, device=dev), True, True,
                                                 mark=e[1].record)
            e[2].record()
            logits, iou = logits.flatten(0, 1), iou.flatten()
            # one pass over every mask of the batch (the statistics of a mask do not depend on the others), then both filters on the small
            # arrays: the same kept set as filtering by predicted IoU first, without gathering the logits in between
            stats = model.mask_stats(logits, self.mask_threshold, self.stability_score_offset)
            stability = stats[:, 0].to(torch.float32) / stats[:, 1].to(torch.float32)       # (0 / 0 is NaN and fails the test below)
            sel = torch.nonzero((iou > self.pred_iou_thresh) & (stability >= self.stability_score_thresh)).flatten()
            if sel.numel():
                point = torch.arange(lo, hi, device=dev).repeat_interleave(iou.numel() // (hi - lo))
                kept.append((logits[sel] > self.mask_threshold, iou[sel], point[sel], stats[sel], stability[sel]))
            e[3].record()
            marks.append(e)
        torch.cuda.synchronize(dev)
        out, regions_ms = [], 0.0
        if kept:
            # the NMS needs boxes and scores only: the masks stay on the device until it has chosen
            masks = torch.cat([k[0] for k in kept])
            iou, point, stats, stability = (torch.cat([k[j] for k in kept]).cpu().numpy() for j in range(1, 5))
            order = box_nms(stats[:, 3:7], iou, self.box_nms_thresh)
            masks = masks[torch.from_numpy(order).to(dev)]
            area_box = stats[order, 2:7]
            if min_mask_region_area > 0:
                masks, keep, area_box, regions_ms = self._small_regions(masks, min_mask_region_area, max(self.box_nms_thresh, self.crop_nms_thresh))
                order = order[keep]                    # (masks and area_box come back as the kept ones, already in that order)
            masks = masks.cpu().numpy()
            for m, i, ab in zip(masks, order, area_box):
                x0, y0, x1, y1 = (int(v) for v in ab[1:5])
                out.append({"segmentation": m, "area": int(ab[0]), "bbox": [x0, y0, x1 - x0, y1 - y0], "predicted_iou": float(iou[i]),
                            "point_coords": [[float(grid[point[i], 0]), float(grid[point[i], 1])]], "stability_score": float(stability[i]),
                            "crop_box": [0, 0, W, H]})
        t_end = time.perf_counter()
        gpu = [sum(e[j].elapsed_time(e[j + 1]) for e in marks) for j in range(3)]
        self.last_timing = {"set_image_ms": 1e3 * (t_set - t_start), "decode_ms": gpu[0], "resize_ms": gpu[1], "stats_ms": gpu[2],
                            "regions_ms": regions_ms, "host_ms": 1e3 * (t_end - t_set) - sum(gpu) - regions_ms,
                            "generate_ms": 1e3 * (t_end - t_start), "masks": len(out)}
        return out

    @staticmethod
    def _small_regions(masks, min_area, nms_thresh):
        """The package's `postprocess_small_regions` on device masks bool [n][H][W]: `masks.clean_masks` (holes, then islands), then box NMS
        over the NEW boxes with score 1 for an unchanged mask and 0 for a changed one, so that a cleaned mask which has become the duplicate
        of an untouched one is the one to go.  -> (cleaned masks of the kept ones on the device, kept indices in NMS order - unchanged first,
        each group in its previous order -, int32 [kept][5] = area, x0, y0, x1, y1, HIP-event ms of the device pass)."""
        from .masks import clean_masks
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cleaned, changed, stats = clean_masks(masks, min_area)
        e1.record()
        changed, stats = changed.cpu().numpy(), stats.cpu().numpy()                         # (synchronises: the events are complete)
        keep = box_nms(stats[:, 1:5], 1.0 - changed.astype(np.float32), nms_thresh)
        return cleaned[torch.from_numpy(keep).to(masks.device)], keep, stats[keep], e0.elapsed_time(e1)

    @torch.no_grad()
    def postprocess_small_regions(self, anns, min_area, nms_thresh):
        """The step `generate(image, min_mask_region_area=min_area)` applies, on a list of annotation dicts from anywhere (their
        `segmentation` arrays must share one shape): a NEW list in the package's order; a changed mask gets its new `segmentation`, `area`
        and `bbox`, every other key stays (`predicted_iou` and `stability_score` are those of the mask before, as in the package)."""
        if min_area < 0:
            raise ValueError("postprocess_small_regions: min_area must be >= 0")
        anns = list(anns)
        if not anns or min_area == 0:
            return [dict(a) for a in anns]
        self.predictor.model._need_gpu()
        dev = self.predictor.model.device
        masks = torch.from_numpy(np.stack([np.asarray(a["segmentation"]) != 0 for a in anns])).to(dev)
        cleaned, keep, area_box, _ = self._small_regions(masks, min_area, nms_thresh)
        out = []
        for m, i, ab in zip(cleaned.cpu().numpy(), keep, area_box):
            x0, y0, x1, y1 = (int(v) for v in ab[1:5])
            out.append(dict(anns[i], segmentation=m, area=int(ab[0]), bbox=[x0, y0, x1 - x0, y1 - y0]))
        return out
