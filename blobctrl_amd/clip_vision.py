"""CLIP vision tower with projection (ViT-H/14 for IP-Adapter's sd15 models, ViT-L/14 for others) on MI355X: replaces
`self.image_encoder(image, output_hidden_states=...)` of the reference's `encode_image` (arithmetic of transformers'
CLIPVisionModelWithProjection).  Runs once per edit, per image prompt.

Patch-embed (im2col + GEMM, no bias) -> [CLS] + position embeddings -> pre-LayerNorm -> L x { x + out_proj(attention(LN1 x)) ;
x + fc2(act(fc1(LN2 x))) } -> post-LayerNorm on token 0 -> visual_projection (no bias).  `hidden_act` is `gelu` (ViT-H) or `quick_gelu`
(ViT-L): both GEMM epilogues.  Every launch exists: the tower is recorded from Recorder.gemm / layernorm / attention with bc_patchify and
bc_add_cls_pos, in the style of Dinov2Model; one plan per (B, H, W), replayed as a graph.
`hidden_states[-2]` - what an IP-Adapter Plus reads - is the input of the last layer, without the post-LayerNorm.
"""
import torch

from . import _lib
from .launch import Recorder, run_graphed
from .weights import pad8

_ACTS = {"gelu": _lib.ACT_GELU, "quick_gelu": _lib.ACT_QUICK_GELU}


class CLIPVisionModelWithProjection:
    def __init__(self, state_dict, num_heads: int, patch_size: int = 14, image_size: int = 224, hidden_act: str = "quick_gelu",
                 eps: float = 1e-5, device="cuda:0"):
        self.device = torch.device(device)
        # (a host device is accepted for CONSTRUCTION only - loading / inspecting checkpoints; running refuses it: `_need_gpu`)
        _lib.load()
        # the `vision_model.` prefix is optional, as `text_model.` is for the text tower; `visual_projection` sits beside it
        sd = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v.detach().float().cpu() for k, v in state_dict.items()}
        if hidden_act not in _ACTS:
            raise ValueError(f"unsupported hidden_act {hidden_act!r} (gelu, quick_gelu)")
        self.sd = sd
        self.heads, self.patch, self.eps, self.act = num_heads, patch_size, eps, _ACTS[hidden_act]
        self.D = sd["embeddings.class_embedding"].shape[-1]
        self.P = sd["visual_projection.weight"].shape[0]
        if self.D % num_heads or (self.D // num_heads) not in (8, 16, 32, 40, 64, 80, 160):
            raise ValueError(f"unsupported head_dim {self.D}/{num_heads}")
        self.L = 0
        while f"encoder.layers.{self.L}.layer_norm1.weight" in sd:
            self.L += 1
        self.config = type("CLIPVisionConfig", (), dict(image_size=image_size, patch_size=patch_size, hidden_size=self.D, projection_dim=self.P,
                                                        num_hidden_layers=self.L, num_attention_heads=num_heads, hidden_act=hidden_act))()
        self.dtype = torch.float16
        dev = self.device
        h, f = {}, {}
        w = sd["embeddings.patch_embedding.weight"].flatten(1)               # the patch convolution has no bias
        self.Kpad = pad8(w.shape[1])
        wp = torch.zeros(w.shape[0], self.Kpad)
        wp[:, : w.shape[1]] = w
        h["patch.weight"] = wp.half().to(dev)
        f["cls"] = sd["embeddings.class_embedding"].reshape(-1).to(dev)
        f["pos"] = sd["embeddings.position_embedding.weight"].contiguous().to(dev)
        f["pre.weight"], f["pre.bias"] = sd["pre_layrnorm.weight"].to(dev), sd["pre_layrnorm.bias"].to(dev)   # (transformers' own spelling)
        for i in range(self.L):
            p = f"encoder.layers.{i}."
            a = p + "self_attn."
            h[p + "qk.weight"] = torch.cat([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"]], 0).half().to(dev)
            f[p + "qk.bias"] = torch.cat([sd[a + "q_proj.bias"], sd[a + "k_proj.bias"]], 0).to(dev)
            for src, dst in (("self_attn.v_proj", "v"), ("self_attn.out_proj", "o"), ("mlp.fc1", "fc1"), ("mlp.fc2", "fc2")):
                h[p + dst + ".weight"] = sd[p + src + ".weight"].half().to(dev)
                f[p + dst + ".bias"] = sd[p + src + ".bias"].to(dev)
            for nm in ("layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias"):
                f[p + nm] = sd[p + nm].to(dev)
        f["post.weight"], f["post.bias"] = sd["post_layernorm.weight"].to(dev), sd["post_layernorm.bias"].to(dev)
        h["proj.weight"] = sd["visual_projection.weight"].half().to(dev)     # no bias
        self.h, self.f = h, f
        self._plans = {}
        self.replays = 0                                                     # graph replays so far (a cached result costs none)

    @classmethod
    def from_pretrained(cls, path, subfolder=None, device="cuda:0", **_ignored):
        """`CLIPVisionModelWithProjection.from_pretrained(path, subfolder="image_encoder")`: a local config.json + model.safetensors."""
        import os
        from .checkpoint import _config, _model_file, read_safetensors
        d = os.path.join(path, subfolder) if subfolder else path
        cfg = _config(d)
        cfg = cfg.get("vision_config", cfg)
        return cls(read_safetensors(_model_file(d)), num_heads=cfg.get("num_attention_heads", 16), patch_size=cfg.get("patch_size", 14),
                   image_size=cfg.get("image_size", 224), hidden_act=cfg.get("hidden_act", "quick_gelu"),
                   eps=cfg.get("layer_norm_eps", 1e-5), device=device)

    def to(self, *a, **k):
        return self

    def parameters(self):
        """The device tensors, as far as `next(image_encoder.parameters()).dtype` of the reference's encode_image needs them."""
        return iter(list(self.h.values()) + list(self.f.values()))

    def _need_gpu(self):
        if self.device.type != "cuda":
            raise _lib.BlobCtrlHipError("blobctrl_amd.CLIPVisionModelWithProjection runs on MI355X only; there is no CPU fallback")

    def _plan(self, B, H, W):
        self._need_gpu()
        key = (B, H, W)
        if key in self._plans:
            return self._plans[key]
        D, heads = self.D, self.heads
        d = D // heads
        gh, gw = H // self.patch, W // self.patch
        T = gh * gw
        N = T + 1
        M = B * N
        hw, fw = self.h, self.f
        if fw["pos"].shape[0] != N:
            raise ValueError(f"a {H} x {W} input gives {N} tokens; the position embedding holds {fw['pos'].shape[0]} "
                             f"(image_size {self.config.image_size})")
        rec = Recorder(self.device)
        P = type("Plan", (), {})()
        P.rec = rec
        P.pixels = rec.zeros(B, 3, H, W, dtype=torch.float32)
        P.seg = rec.begin("clip_vision")
        cols = rec.empty(B * T, self.Kpad)
        rec.call("bc_patchify", P.pixels.data_ptr(), B, H, W, self.patch, self.Kpad, cols.data_ptr(), kind="patchify")
        pe = rec.empty(B * T, D)
        rec.gemm(A=cols, W=hw["patch.weight"], M=B * T, N=D, K=self.Kpad, out=pe, kind="patch_embed")
        x0 = rec.empty(M, D)
        rec.call("bc_add_cls_pos", pe.data_ptr(), fw["cls"].data_ptr(), fw["pos"].data_ptr(), B, T, D, x0.data_ptr(), kind="cls_pos")
        x = rec.layernorm(x0, M, D, fw["pre.weight"], fw["pre.bias"], self.eps)
        ldvt = (N + 63) // 64 * 64
        P.hidden = [x]
        for i in range(self.L):
            p = f"encoder.layers.{i}."
            ln = rec.layernorm(x, M, D, fw[p + "layer_norm1.weight"], fw[p + "layer_norm1.bias"], self.eps)
            qk = rec.empty(M, 2 * D)
            rec.gemm(A=ln, W=hw[p + "qk.weight"], M=M, N=2 * D, K=D, out=qk, bias=fw[p + "qk.bias"], kind="qkv")
            vt = rec.zeros(B, D, ldvt)
            rec.gemm(A=ln, W=hw[p + "v.weight"], M=M, N=D, K=D, out=vt, bias=fw[p + "v.bias"], out_mode=_lib.OUT_F16_T,
                     ldc=ldvt, rows_per_batch=N, kind="qkv")
            a = rec.empty(M, D)
            rec.attention(qk, qk, vt, a, B, heads, d, N, N, 2 * D, 2 * D, ldvt, D, N * 2 * D, N * 2 * D, D * ldvt, N * D,
                          d ** -0.5, q_off=0, k_off=D)
            x2 = rec.empty(M, D)
            rec.gemm(A=a, W=hw[p + "o.weight"], M=M, N=D, K=D, out=x2, bias=fw[p + "o.bias"], R=x, ldr=D, kind="attn_out")
            ln = rec.layernorm(x2, M, D, fw[p + "layer_norm2.weight"], fw[p + "layer_norm2.bias"], self.eps)
            F1 = hw[p + "fc1.weight"].shape[0]
            m1 = rec.empty(M, F1)
            rec.gemm(A=ln, W=hw[p + "fc1.weight"], M=M, N=F1, K=D, out=m1, bias=fw[p + "fc1.bias"], act=self.act, kind="ff")
            x = rec.empty(M, D)
            rec.gemm(A=m1, W=hw[p + "fc2.weight"], M=M, N=D, K=F1, out=x, bias=fw[p + "fc2.bias"], R=x2, ldr=D, kind="ff")
            P.hidden.append(x)
        # post-LayerNorm on token 0 of every image only (row stride N * D), then the projection
        pooled = rec.layernorm(x, B, D, fw["post.weight"], fw["post.bias"], self.eps, ldx=N * D, ldy=D)
        P.embeds = rec.empty(B, self.P)
        rec.gemm(A=pooled, W=hw["proj.weight"], M=B, N=self.P, K=D, out=P.embeds, kind="visual_projection")
        P.N = N
        self._plans[key] = P
        return P

    @torch.no_grad()
    def __call__(self, pixel_values: torch.Tensor, output_hidden_states: bool = False):
        """pixel_values [B][3][H][W] (H = W = config.image_size) -> an object with `.image_embeds` [B][projection_dim] fp16 and, when
        asked, `.hidden_states`: the L + 1 tensors [B][N][D] fp16 of transformers' output (the pre-LayerNorm's output, then every layer's)."""
        B, C, H, W = pixel_values.shape
        if C != 3 or H % self.patch or W % self.patch:
            raise ValueError("pixel_values must be [B,3,H,W] with H, W multiples of the patch size")
        P = self._plan(B, H, W)
        P.pixels.copy_(pixel_values.to(self.device, torch.float32))
        run_graphed(P.seg, self.device)
        self.replays += 1
        out = type("CLIPVisionModelOutput", (), {})()
        out.image_embeds = P.embeds.clone()
        out.hidden_states = tuple(h.view(B, P.N, self.D).clone() for h in P.hidden) if output_hidden_states else None
        return out
