"""AutoencoderTiny (TAESD for SD-1.5) decoder on MI355X - the cheap look at the latents a `callback_on_step_end` receives.

Keeps the call surface of `diffusers.AutoencoderTiny` (D/models/autoencoders/autoencoder_tiny.py) that a preview uses:
    taesd = AutoencoderTiny.from_pretrained(folder)            # or AutoencoderTiny(state_dict)
    image = taesd.decode(latents).sample                       # fp32 NCHW in [-1, 1]; return_dict=False -> (image,)
    bytes = taesd.preview(latents)                             # uint8 [B][8h][8w][3] on the device (not in the reference)
Host mirror of DecoderTiny (D/models/autoencoders/vae.py:899-982) and AutoencoderTinyBlock (D/models/unets/unet_2d_blocks.py:552-586) on
csrc/tiny_vae.hip: one bc_tiny_latents_in (tanh(z / 3) * 3, fp16 NHWC) and 35 bc_tiny_conv3x3 launches - conv_in + ReLU, ten blocks of
conv+ReLU, conv+ReLU, conv + skip + ReLU, three bias-free convolutions that read their input through the nearest-2x upsample, and the
3-channel output convolution with the `2 y - 1` (or the quantising) epilogue.  Nothing but convolutions: no GroupNorm, no attention.
Only the default architecture (64 channels, decoder blocks (3, 3, 3, 1), ReLU, nearest, 4 latent channels) is accepted.
"""
from collections import OrderedDict

import torch

from . import _lib
from .launch import Recorder, run_graphed
from .weights import pack_conv3x3

DEFAULTS = OrderedDict([
    ("in_channels", 3), ("out_channels", 3), ("encoder_block_out_channels", (64, 64, 64, 64)), ("decoder_block_out_channels", (64, 64, 64, 64)),
    ("act_fn", "relu"), ("upsample_fn", "nearest"), ("latent_channels", 4), ("upsampling_scaling_factor", 2),
    ("num_encoder_blocks", (1, 3, 3, 3)), ("num_decoder_blocks", (3, 3, 3, 1)), ("latent_magnitude", 3), ("latent_shift", 0.5),
    ("force_upcast", False), ("scaling_factor", 1.0), ("shift_factor", 0.0),
])
# the fields the decoder's launch list depends on: any other value is refused
_FIXED = ("out_channels", "decoder_block_out_channels", "act_fn", "upsample_fn", "latent_channels", "upsampling_scaling_factor",
          "num_decoder_blocks")
CH = 64


def decoder_layers(num_blocks=(3, 3, 3, 1)):
    """The decoder as a list of convolutions in launch order: dict(name, form, stage) with `name` the state-dict prefix of the Conv2d
    (`decoder.layers.<i>` or `decoder.layers.<i>.conv.<j>`), `form` one of in / a / b / c / up / out and `stage` the resolution the
    convolution's OUTPUT has (0 = the latent's, each stage doubles it).  Indices follow DecoderTiny.__init__ (vae.py:931-957)."""
    out = [dict(name="decoder.layers.0", form="in", stage=0)]
    i = 2                                                              # (layers.1 is the ReLU)
    for s, n in enumerate(num_blocks):
        for _ in range(n):
            for j, form in ((0, "a"), (2, "b"), (4, "c")):
                out.append(dict(name=f"decoder.layers.{i}.conv.{j}", form=form, stage=s))
            i += 1
        last = s == len(num_blocks) - 1
        if not last:
            i += 1                                                     # (the Upsample)
        out.append(dict(name=f"decoder.layers.{i}", form="out" if last else "up", stage=s if last else s + 1))
        i += 1
    return out


class _Output:
    """`DecoderOutput` of the reference: `.sample`."""

    def __init__(self, sample):
        self.sample = sample


class AutoencoderTiny:
    def __init__(self, state_dict, device="cuda:0", config=None):
        self.device = torch.device(device)
        # (a host device is accepted for CONSTRUCTION only - loading / inspecting checkpoints, recording launch lists; running refuses it)
        self.lib = _lib.load()
        cfg = OrderedDict(DEFAULTS)
        for k, v in (config or {}).items():
            if k.startswith("_") or k == "block_out_channels":
                continue
            cfg[k] = tuple(v) if isinstance(v, list) else v
        for k in _FIXED:
            if cfg[k] != DEFAULTS[k]:
                raise ValueError(f"AutoencoderTiny: {k}={cfg[k]!r} is not supported, only the default architecture ({k}={DEFAULTS[k]!r})")
        cfg["block_out_channels"] = cfg["decoder_block_out_channels"]
        self.config = type("Config", (), dict(cfg))()
        self.latent_magnitude, self.latent_shift, self.scaling_factor = cfg["latent_magnitude"], cfg["latent_shift"], cfg["scaling_factor"]
        self.latent_channels = cfg["latent_channels"]
        self.layers = decoder_layers(cfg["num_decoder_blocks"])
        sd = {k: v.detach().float().cpu() for k, v in state_dict.items() if not k.startswith("encoder.")}
        self._check_schema(sd)
        self.h, self.f = {}, {}
        for L in self.layers:
            w = sd[L["name"] + ".weight"]
            if L["form"] == "out":                                     # Co 3 -> 8 with zero rows: padding of the weights only
                w = torch.cat([w, torch.zeros(8 - w.shape[0], *w.shape[1:])], 0)
            self.h[L["name"] + ".weight"] = pack_conv3x3(w).half().contiguous().to(self.device)      # (pack_conv3x3 pads Ci 4 -> 8 with zeros)
            if L["form"] != "up":
                self.f[L["name"] + ".bias"] = sd[L["name"] + ".bias"].contiguous().to(self.device)
        self.use_slicing = False
        self.use_tiling = False
        self._plans = {}
        self.input_read = None            # event behind the last decode / preview's read of its input (pipeline.preview orders the loop after it)

    def _check_schema(self, sd):
        from .synth import tiny_vae_param_shapes
        want = tiny_vae_param_shapes()
        conv_in = sd.get("decoder.layers.0.weight")
        if conv_in is None or conv_in.ndim != 4:
            raise ValueError("AutoencoderTiny: the state dict has no decoder (decoder.layers.0.weight)")
        if conv_in.shape[1] != 4:
            raise ValueError(f"AutoencoderTiny: latent_channels={conv_in.shape[1]} is not supported, only the default architecture (4)")
        if conv_in.shape[0] != CH:
            raise ValueError(f"AutoencoderTiny: decoder_block_out_channels={conv_in.shape[0]} is not supported, only the default (64, 64, 64, 64)")
        have = {k for k in sd if k.startswith("decoder.")}
        if have != set(want):
            odd = sorted(have ^ set(want))
            raise ValueError(f"AutoencoderTiny: num_decoder_blocks other than (3, 3, 3, 1) is not supported: the decoder's keys differ from the "
                             f"default architecture's at {odd[:4]}{' ...' if len(odd) > 4 else ''}")
        for k, shp in want.items():
            if tuple(sd[k].shape) != tuple(shp):
                field = "out_channels" if k.startswith("decoder.layers.18") else "decoder_block_out_channels"
                raise ValueError(f"AutoencoderTiny: {field}: {k} has shape {tuple(sd[k].shape)}, the default architecture has {tuple(shp)}")

    @classmethod
    def from_pretrained(cls, path, subfolder=None, device="cuda:0", **_ignored):
        """`AutoencoderTiny.from_pretrained("madebyollin/taesd" checked out locally)`: config.json + diffusion_pytorch_model.safetensors."""
        import os
        from .checkpoint import _config, _model_file, read_safetensors
        d = os.path.join(path, subfolder) if subfolder else path
        return cls(read_safetensors(_model_file(d)), device=device, config=_config(d))

    def to(self, *a, **k):
        return self

    # ------------------------------------------------------------------------------------------------ reference helpers
    def scale_latents(self, x: torch.Tensor) -> torch.Tensor:
        """raw latents -> [0, 1]  (autoencoder_tiny.py:161-163)"""
        return x.div(2 * self.latent_magnitude).add(self.latent_shift).clamp(0, 1)

    def unscale_latents(self, x: torch.Tensor) -> torch.Tensor:
        """[0, 1] -> raw latents  (autoencoder_tiny.py:165-167)"""
        return x.sub(self.latent_shift).mul(2 * self.latent_magnitude)

    def enable_slicing(self):
        """Decode a batch one image per plan (autoencoder_tiny.py:169-174).  Images are independent: the bits do not change."""
        self.use_slicing = True

    def disable_slicing(self):
        self.use_slicing = False

    def enable_tiling(self, use_tiling: bool = True):
        raise NotImplementedError("AutoencoderTiny.enable_tiling: a tiny decoder has no memory problem on this part (its largest activation "
                                  "at 512 x 512 is 33 MB), and the reference's tiled form blends differently from AutoencoderKL's")

    def disable_tiling(self):
        self.use_tiling = False

    def encode(self, *a, **k):
        raise NotImplementedError("AutoencoderTiny.encode: only the decoder is implemented - the pipeline cannot use a tiny encoder "
                                  "(it reads vae.encode(...).latent_dist), and a preview needs none")

    # ------------------------------------------------------------------------------------------------ plans
    def _need_gpu(self):
        if self.device.type != "cuda":
            raise _lib.BlobCtrlHipError("blobctrl_amd.AutoencoderTiny runs on MI355X only; there is no CPU fallback")

    def _conv(self, rec, L, x, B, H, W, skip=None, out=None, out_mode=_lib.TINY_OUT_F16):
        """Record one bc_tiny_conv3x3 with output size H x W; returns `out`."""
        form = L["form"]
        Ci, Co = (8 if form == "in" else CH), (3 if form == "out" else CH)
        w, bias = self.h[L["name"] + ".weight"], self.f.get(L["name"] + ".bias")
        up, relu = int(form == "up"), int(form in ("in", "a", "b", "c"))
        refs = (x, w, bias, skip, out)
        rec.keep.append(refs)
        for t in refs:
            rec.register(t)
        in_pix = B * H * W // (4 if up else 1)
        out_bytes = B * H * W * (128 if Co == CH else (12 if out_mode == _lib.TINY_OUT_IMAGE else 3))
        rec._op("bc_tiny_conv3x3_flat", (x, w, bias, skip, out, B, H, W, Ci, Co, up, relu, out_mode), "tiny_conv",
                flops=2 * B * H * W * 9 * Ci * (CH if Co == CH else 3), variant=f"tiny_conv3x3_kernel<{Ci},{2 if Co == CH else 1}>",
                shape=("tiny_" + form, B, H, W, Ci, Co), bytes_=2 * in_pix * Ci + w.numel() * 2 + out_bytes + (B * H * W * 128 if skip is not None else 0),
                rocprof=f"tiny_conv3x3_kernel<{Ci}, {2 if Co == CH else 1}>")
        return out

    def _plan(self, B, h, w):
        """The launch lists of a (B, h, w) latent, recorded once: segment `decode` (fp32 NCHW image) and segment `preview` (uint8 NHWC),
        1 + 35 launches each over the same buffers."""
        key = (B, h, w)
        if key in self._plans:
            return self._plans[key]
        rec = Recorder(self.device)
        P = type("Plan", (), {})()
        P.rec = rec
        P.zin = rec.zeros(B, 4, h, w, dtype=torch.float32)
        P.z8 = rec.zeros(B, h * w, 8)
        H, W = 8 * h, 8 * w
        P.img = rec.zeros(B, 3, H, W, dtype=torch.float32)
        P.u8 = rec.zeros(B, H, W, 3, dtype=torch.uint8)
        pools = [[rec.empty(B, (h << s) * (w << s), CH) for _ in range(3)] for s in range(4)]      # per stage: input / two scratch, rotating

        def record(name, final, mode):
            seg = rec.begin(name)
            rec.keep.append((P.zin, P.z8))
            rec._op("bc_tiny_latents_in", (P.zin, B, h, w, P.z8), "tiny_latents_in", variant="tiny_latents_in_kernel",
                    shape=("tiny_latents_in", B, h, w), bytes_=B * h * w * 32)
            x, block_in = P.z8, None
            for L in self.layers:
                s = L["stage"]
                Hs, Ws = h << s, w << s
                if L["form"] == "out":
                    self._conv(rec, L, x, B, Hs, Ws, out=final, out_mode=mode)
                    break
                if L["form"] == "a":
                    block_in = x
                dst = next(t for t in pools[s] if t is not x and t is not block_in)
                x = self._conv(rec, L, x, B, Hs, Ws, skip=block_in if L["form"] == "c" else None, out=dst)
                if L["form"] == "c":
                    block_in = None
            return seg

        P.decode = record("tiny_vae_decode", P.img, _lib.TINY_OUT_IMAGE)
        P.preview = record("tiny_vae_preview", P.u8, _lib.TINY_OUT_U8)
        self._plans[key] = P
        return P

    def _run(self, z, which):
        """Copy z into the plan of its shape, replay `which` ("decode" / "preview") as one graph, and return a fresh copy of the result - all
        enqueued on the caller's current stream (launch.run_graphed orders the replay behind it and the copy behind the replay)."""
        self._need_gpu()
        B, Cz, h, w = z.shape
        P = self._plan(B, h, w)
        P.zin.copy_(z, non_blocking=True)
        self.input_read = torch.cuda.current_stream(self.device).record_event()
        run_graphed(getattr(P, which), self.device)
        return (P.img if which == "decode" else P.u8).clone()

    def _apply(self, z, which):
        if z.ndim != 4 or z.shape[1] != self.latent_channels:
            raise ValueError(f"expected latents [B][{self.latent_channels}][h][w], got {tuple(z.shape)}")
        self._need_gpu()
        zz = z.to(self.device, torch.float32)
        if self.use_slicing and zz.shape[0] > 1:
            return torch.cat([self._run(zz[b:b + 1], which) for b in range(zz.shape[0])])
        return self._run(zz, which)

    # ------------------------------------------------------------------------------------------------ API
    @torch.no_grad()
    def decode(self, x: torch.Tensor, generator=None, return_dict: bool = True):
        """x [B, 4, h, w] -> object with `.sample` [B, 3, 8h, 8w] fp32 (return_dict=False: `(sample,)`), on the caller's current stream."""
        sample = self._apply(x, "decode")
        return _Output(sample) if return_dict else (sample,)

    @torch.no_grad()
    def preview(self, latents: torch.Tensor) -> torch.Tensor:
        """latents [B, 4, h, w] -> uint8 [B][8h][8w][3] on the device: round_half_even(clamp(sample / 2 + 0.5, 0, 1) * 255), quantised in the
        last convolution's epilogue."""
        return self._apply(latents, "preview")
