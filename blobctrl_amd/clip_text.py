"""CLIP text encoder (SD-1.5: 12 layers, 768-d, 12 heads, 77 tokens) on MI355X: replaces
`self.text_encoder(text_input_ids)[0]` of blobctrl/pipelines/pipeline_blobnet.py:599-611 (arithmetic of transformers'
CLIPTextModel, pinned 4.49.0 upstream), including the clip_skip branch.  Runs once per edit.

Token + position embedding gather -> L x { x + out_proj(causal attention(LN1 x)) ; x + fc2(quick_gelu(fc1(LN2 x))) } -> final
LayerNorm.  Reuses the hot path's LayerNorm / MFMA GEMM / flash-attention kernels (causal-mask entry point); biases, quick_gelu
and the residual adds are GEMM epilogues.  Tokenisation stays on the host (callers pass `input_ids`).
"""
from collections import OrderedDict

import torch

from . import _lib
from .launch import Recorder, run_graphed
from .weights import LoraAdapters


class CLIPTextModel(LoraAdapters):
    """LoRA (load_lora_into_text_encoder of the reference): the fp32 state dict stays on the host with the adapter registry of the UNet
    shell (weights.LoraAdapters).  Adapters are merged in fp32 before the fp16 cast and the q|k concatenation; when the merged weights
    change, the device tensors are refilled IN PLACE, so every recorded plan keeps its addresses and gives the new result."""

    _LORA_TARGETS = (("self_attn.v_proj", "v"), ("self_attn.out_proj", "o"), ("mlp.fc1", "fc1"), ("mlp.fc2", "fc2"))

    def __init__(self, state_dict, num_heads: int = 12, eps: float = 1e-5, device="cuda:0"):
        self.device = torch.device(device)
        # (a host device is accepted for CONSTRUCTION only - loading / inspecting checkpoints; running refuses it: `_need_gpu`)
        _lib.load()
        # on-disk layout has a "text_model." prefix (transformers 4.x); 5.x dropped it
        sd = {(k[len("text_model."):] if k.startswith("text_model.") else k): v.detach().float().cpu()
              for k, v in state_dict.items()}
        self._sd = sd
        self._init_lora()
        dev = self.device
        self.heads, self.eps = num_heads, eps
        self.vocab, self.D = sd["embeddings.token_embedding.weight"].shape
        self.max_pos = sd["embeddings.position_embedding.weight"].shape[0]
        if self.D % num_heads or (self.D // num_heads) not in (8, 16, 32, 40, 64, 80, 160):
            raise ValueError(f"unsupported head_dim {self.D}/{num_heads}")
        self.L = 0
        while f"encoder.layers.{self.L}.layer_norm1.weight" in sd:
            self.L += 1
        h, f = {}, {}
        h["tok"] = sd["embeddings.token_embedding.weight"].half().to(dev)
        f["pos"] = sd["embeddings.position_embedding.weight"].to(dev)
        for i in range(self.L):
            p = f"encoder.layers.{i}."
            a = p + "self_attn."
            f[p + "qk.bias"] = torch.cat([sd[a + "q_proj.bias"], sd[a + "k_proj.bias"]], 0).to(dev)
            for src, dst in self._LORA_TARGETS:
                f[p + dst + ".bias"] = sd[p + src + ".bias"].to(dev)
            for nm in ("layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias"):
                f[p + nm] = sd[p + nm].to(dev)
        f["final.weight"] = sd["final_layer_norm.weight"].to(dev)
        f["final.bias"] = sd["final_layer_norm.bias"].to(dev)
        self.h, self.f = h, f
        self._plans = {}
        self._fill(1.0)

    # ---- the weights LoRA can target: q|k, v, out, fc1, fc2 of every layer, fp16 on the device
    def _fill(self, lora_scale: float):
        sd = self.effective_state_dict(lora_scale)
        for i in range(self.L):
            p = f"encoder.layers.{i}."
            new = {p + "qk.weight": torch.cat([sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.k_proj.weight"]], 0).half()}
            for src, dst in self._LORA_TARGETS:
                new[p + dst + ".weight"] = sd[p + src + ".weight"].half()
            for k, v in new.items():
                if k in self.h:
                    self.h[k].copy_(v)          # in place: the recorded plans hold this address
                else:
                    self.h[k] = v.to(self.device)
        self._filled = self._lora_state(lora_scale)

    def _lora_changed(self):
        """No work now: `__call__` refills the device tensors when the state they were filled for is not the one it is asked for."""
        self._filled = None

    def load_lora_adapter(self, lora, alphas, adapter_name="default", weight: float = 1.0):
        """`lora` / `alphas` as checkpoint.split_lora_state_dict returns them; module names with or without the `text_model.` prefix."""
        strip = lambda k: k[len("text_model."):] if k.startswith("text_model.") else k
        super().load_lora_adapter(OrderedDict((strip(k), v) for k, v in lora.items()), {strip(m): a for m, a in alphas.items()},
                                  adapter_name, weight)

    @classmethod
    def from_pretrained(cls, path, subfolder=None, device="cuda:0", **_ignored):
        """`CLIPTextModel.from_pretrained(sd15_path, subfolder="text_encoder")`: config.json + model.safetensors."""
        import os
        from .checkpoint import _config, _model_file, read_safetensors
        d = os.path.join(path, subfolder) if subfolder else path
        cfg = _config(d)
        return cls(read_safetensors(_model_file(d)), num_heads=cfg.get("num_attention_heads", 12),
                   eps=cfg.get("layer_norm_eps", 1e-5), device=device)

    def to(self, *a, **k):
        return self

    def _need_gpu(self):
        if self.device.type != "cuda":
            raise _lib.BlobCtrlHipError("blobctrl_amd.CLIPTextModel runs on MI355X only; there is no CPU fallback")

    def _plan(self, B, T):
        self._need_gpu()
        key = (B, T)
        if key in self._plans:
            return self._plans[key]
        rec = Recorder(self.device)
        P = type("Plan", (), {})()
        P.rec = rec
        D, heads = self.D, self.heads
        d = D // heads
        M = B * T
        hw, fw = self.h, self.f
        P.ids = torch.zeros(B, T, dtype=torch.int64, device=self.device)
        P.seg = rec.begin("clip_text")
        x = rec.empty(M, D)
        rec.call("bc_embed_tokens", P.ids.data_ptr(), hw["tok"].data_ptr(), fw["pos"].data_ptr(), B, T, D, self.vocab,
                 x.data_ptr(), kind="embed", keep=(P.ids, x))
        ldvt = (T + 63) // 64 * 64
        P.hidden = [x]
        for i in range(self.L):
            p = f"encoder.layers.{i}."
            ln = rec.layernorm(x, M, D, fw[p + "layer_norm1.weight"], fw[p + "layer_norm1.bias"], self.eps)
            qk = rec.empty(M, 2 * D)
            rec.gemm(A=ln, W=hw[p + "qk.weight"], M=M, N=2 * D, K=D, out=qk, bias=fw[p + "qk.bias"], kind="qkv")
            vt = rec.zeros(B, D, ldvt)
            rec.gemm(A=ln, W=hw[p + "v.weight"], M=M, N=D, K=D, out=vt, bias=fw[p + "v.bias"], out_mode=_lib.OUT_F16_T,
                     ldc=ldvt, rows_per_batch=T, kind="qkv")
            a = rec.empty(M, D)
            rec.attention(qk, qk, vt, a, B, heads, d, T, T, 2 * D, 2 * D, ldvt, D, T * 2 * D, T * 2 * D, D * ldvt, T * D,
                          d ** -0.5, q_off=0, k_off=D, causal=True)
            x2 = rec.empty(M, D)
            rec.gemm(A=a, W=hw[p + "o.weight"], M=M, N=D, K=D, out=x2, bias=fw[p + "o.bias"], R=x, ldr=D, kind="attn_out")
            ln = rec.layernorm(x2, M, D, fw[p + "layer_norm2.weight"], fw[p + "layer_norm2.bias"], self.eps)
            F1 = hw[p + "fc1.weight"].shape[0]
            m1 = rec.empty(M, F1)
            rec.gemm(A=ln, W=hw[p + "fc1.weight"], M=M, N=F1, K=D, out=m1, bias=fw[p + "fc1.bias"], act=_lib.ACT_QUICK_GELU,
                     kind="ff")
            x = rec.empty(M, D)
            rec.gemm(A=m1, W=hw[p + "fc2.weight"], M=M, N=D, K=F1, out=x, bias=fw[p + "fc2.bias"], R=x2, ldr=D, kind="ff")
            P.hidden.append(x)
        P.final = {}
        for skip, src in ((None, P.hidden[-1]),) + tuple((s, P.hidden[-(s + 1)]) for s in range(1, min(self.L, 4))):
            P.final[skip] = rec.layernorm(src, M, D, fw["final.weight"], fw["final.bias"], self.eps)
        self._plans[key] = P
        return P

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor, attention_mask=None, clip_skip=None, lora_scale: float = 1.0):
        """input_ids [B, T] int64 (T <= max_position_embeddings) -> (prompt_embeds [B, T, D] fp16,), as `text_encoder(ids)[0]`;
        `clip_skip=k` returns final_layer_norm(hidden_states[-(k+1)]) (pipe:604-611).  `lora_scale`: the per-call scale of the active
        adapters (encode_prompt's scale_lora_layers, pipe:551-558); the device weights stay at the last scale asked for."""
        if attention_mask is not None:
            raise NotImplementedError("SD-1.5's text encoder config has no use_attention_mask (pipe:593-596)")
        B, T = input_ids.shape
        if T > self.max_pos:
            raise ValueError(f"sequence length {T} exceeds max_position_embeddings {self.max_pos}")
        P = self._plan(B, T)
        if self._lora_state(lora_scale) != self._filled:
            torch.cuda.synchronize(self.device)             # (no replay may still be reading the weights)
            self._fill(lora_scale)
        if clip_skip not in P.final:
            raise ValueError(f"clip_skip={clip_skip} not supported (0 < clip_skip < min(layers, 4))")
        P.ids.copy_(input_ids.to(self.device, torch.int64))
        run_graphed(P.seg, self.device)
        return (P.final[clip_skip].view(B, T, self.D).clone(),)
