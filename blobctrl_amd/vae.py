"""SD-1.5 AutoencoderKL (encode / decode) on MI355X — the stages either side of the denoise loop.

Keeps the reference call surface used by the pipeline:
    vae.encode(image).latent_dist.sample(generator)          (pipeline_blobnet.py:300-309; the reference forgets to pass the
                                                              generator there - `sample()` here takes one)
    vae.decode(latents / vae.config.scaling_factor, return_dict=False)[0]      (pipeline_blobnet.py:1133)
Host mirror of D/models/autoencoders/autoencoder_kl.py:249-326 and D/models/autoencoders/vae.py:47-348 on the hot path's
kernels: convs / 1x1 / linears = bc_gemm (fused nearest-2x upsample, the encoder's pad-(0,1,0,1) stride-2 downsample via
`conv_nopad_lo`), GroupNorm(eps 1e-6)+SiLU with statistics from the producer epilogues, and the mid block's single-head,
head_dim-512 attention as GEMM (QK^T, scale folded) -> bc_softmax_rows -> GEMM (P V) per image (V produced transposed).
"""
from typing import Optional

import torch

from . import _lib
from .launch import Recorder, run_graphed
from .weights import pack_conv3x3, pack_matrix, pad8


class _Act:
    __slots__ = ("t", "C", "H", "W")

    def __init__(self, t, C, H, W):
        self.t, self.C, self.H, self.W = t, C, H, W


class _Dist:
    """`latent_dist` of the reference's AutoencoderKLOutput (vae.py:767-789)."""

    def __init__(self, vae, moments, B, h, w):
        self._vae, self._mom, self._B, self._h, self._w = vae, moments, B, h, w

    def sample(self, generator: Optional[torch.Generator] = None, scale: float = 1.0) -> torch.Tensor:
        v = self._vae
        Cz = v.latent_channels
        dev = v.device
        noise = torch.randn((self._B, Cz, self._h, self._w), generator=generator,
                            device=generator.device if generator is not None else "cpu", dtype=torch.float32).to(dev)
        out = torch.empty(self._B, Cz, self._h, self._w, dtype=torch.float32, device=dev)
        _lib.check(v.lib.bc_gaussian_sample(self._mom.data_ptr(), noise.data_ptr(), self._B, Cz, self._h * self._w, scale,
                                            out.data_ptr(), torch.cuda.current_stream().cuda_stream), "bc_gaussian_sample")
        return out

    def mode(self) -> torch.Tensor:
        m = self._mom.view(self._B, self._h, self._w, -1)[..., : self._vae.latent_channels]
        return m.permute(0, 3, 1, 2).float().contiguous()

    @property
    def parameters(self):
        return self._mom.view(self._B, self._h, self._w, -1).permute(0, 3, 1, 2).float().contiguous()


def tile_geometry(kind, H, W, tile_sample_min_size, tile_latent_min_size, tile_overlap_factor, scale):
    """Tile grid of a tiled decode (`kind` "decode": H x W is the latent, tiles grow by `scale`) or a tiled encode ("encode": H x W is the
    image, tiles shrink by `scale`), with the expressions of tiled_decode / tiled_encode (D/models/autoencoders/autoencoder_kl.py:359-361,
    409-411) evaluated as the same Python expressions, so their truncation is the reference's.  Pure host arithmetic: no GPU, no weights.

    Returns dict(overlap, extent, limit, rows, cols, out_h, out_w, tiles) with `tiles` in row-major order, each a dict:
        i, j            grid position
        y0, x0, in_h, in_w     the slice of the input the tile's plan runs on (clipped at the border)
        out_h, out_w    the size of what the plan returns for it
        ev, eh          blend extents against the tile above / to the left, clamped to min(neighbour size, own size, extent); 0 without one
        ch, cw          the cropped size `[:limit, :limit]` that goes into the result
        oy, ox          its origin there: the running sum of the cropped sizes before it (not index * limit)"""
    if kind not in ("decode", "encode"):
        raise ValueError(f"tile_geometry: kind {kind!r} (decode or encode)")
    f = tile_overlap_factor
    if kind == "decode":
        tile_in = tile_latent_min_size
        overlap = int(tile_latent_min_size * (1 - f))
        extent = int(tile_sample_min_size * f)
        limit = tile_sample_min_size - extent
    else:
        tile_in = tile_sample_min_size
        overlap = int(tile_sample_min_size * (1 - f))
        extent = int(tile_latent_min_size * f)
        limit = tile_latent_min_size - extent
    if overlap <= 0:
        raise ValueError(f"tile_overlap_factor {f} leaves a tile step of {overlap}: tiles would never advance")
    if limit <= 0 or extent < 0 or tile_in <= 0:
        raise ValueError(f"tile sizes {tile_sample_min_size} / {tile_latent_min_size} with tile_overlap_factor {f} keep nothing of a tile "
                         f"(blend extent {extent}, crop {limit})")
    ys, xs = list(range(0, H, overlap)), list(range(0, W, overlap))
    tiles, oy = [], 0
    for i, y0 in enumerate(ys):
        ox = 0
        for j, x0 in enumerate(xs):
            in_h, in_w = min(tile_in, H - y0), min(tile_in, W - x0)
            out_h, out_w = (in_h * scale, in_w * scale) if kind == "decode" else (in_h // scale, in_w // scale)
            t = dict(i=i, j=j, y0=y0, x0=x0, in_h=in_h, in_w=in_w, out_h=out_h, out_w=out_w, ev=0, eh=0,
                     ch=min(out_h, limit), cw=min(out_w, limit), oy=oy, ox=ox)
            if i > 0:
                t["ev"] = min(tiles[(i - 1) * len(xs) + j]["out_h"], out_h, extent)
            if j > 0:
                t["eh"] = min(tiles[-1]["out_w"], out_w, extent)
            tiles.append(t)
            ox += t["cw"]
        oy += tiles[-1]["ch"]
    return dict(overlap=overlap, extent=extent, limit=limit, rows=len(ys), cols=len(xs), out_h=oy, out_w=ox, tiles=tiles)


class AutoencoderKL:
    class _Cfg:
        scaling_factor = 0.18215
        sample_size = 512

    def __init__(self, state_dict, norm_num_groups: int = 32, layers_per_block: int = 2, device="cuda:0", sample_size: int = 512):
        self.device = torch.device(device)
        # (a host device is accepted for CONSTRUCTION only - loading / inspecting checkpoints; running refuses it: `_need_gpu`)
        self.lib = _lib.load()
        self.config = self._Cfg()
        self.G, self.lpb = norm_num_groups, layers_per_block
        self.config.block_out_channels = None       # (set below from the weights)
        sd = {k: v.detach().float().cpu() for k, v in state_dict.items()}
        self.latent_channels = sd["post_quant_conv.weight"].shape[0]
        self.h, self.f = {}, {}
        dev = self.device
        for k, v in sd.items():
            if v.ndim == 1:
                self.f[k] = v.to(dev)
            elif v.ndim == 4 and v.shape[-1] == 3:
                self.h[k] = pack_conv3x3(v).half().to(dev)
            else:
                self.h[k] = pack_matrix(v).half().to(dev)
        # q | k fused along N for the mid-block attention
        for side in ("encoder", "decoder"):
            a = f"{side}.mid_block.attentions.0."
            self.h[a + "to_qk.weight"] = torch.cat([sd[a + "to_q.weight"], sd[a + "to_k.weight"]], 0).half().to(dev)
            self.f[a + "to_qk.bias"] = torch.cat([sd[a + "to_q.bias"], sd[a + "to_k.bias"]], 0).to(dev)
        i = 0
        boc = []
        while f"encoder.down_blocks.{i}.resnets.0.conv1.weight" in sd:
            boc.append(sd[f"encoder.down_blocks.{i}.resnets.0.conv1.weight"].shape[0])
            i += 1
        self.config.block_out_channels = tuple(boc)
        self.config.sample_size = sample_size
        # tiling / slicing switches of the reference (autoencoder_kl.py:126-137): plain, settable attributes
        self.use_slicing = False
        self.use_tiling = False
        self.tile_sample_min_size = sample_size
        self.tile_latent_min_size = int(sample_size / (2 ** (len(boc) - 1)))
        self.tile_overlap_factor = 0.25
        self._plans = {}

    @classmethod
    def from_pretrained(cls, path, subfolder=None, device="cuda:0", **_ignored):
        """`AutoencoderKL.from_pretrained(sd15_path, subfolder="vae")`: config.json + diffusion_pytorch_model.safetensors."""
        import os
        from .checkpoint import _config, _model_file, read_safetensors
        d = os.path.join(path, subfolder) if subfolder else path
        cfg = _config(d)
        vae = cls(read_safetensors(_model_file(d)), norm_num_groups=cfg.get("norm_num_groups", 32),
                  layers_per_block=cfg.get("layers_per_block", 2), device=device, sample_size=cfg.get("sample_size", 512))
        vae.config.scaling_factor = cfg.get("scaling_factor", 0.18215)
        return vae

    # ------------------------------------------------------------------------------------------------ recorded blocks
    def _conv(self, rec, B, x: _Act, name, Cout, stride=1, up=False, nopad_lo=False, R=None, want_gn=True, out_f32=False):
        Hv, Wv = (2 * x.H, 2 * x.W) if up else (x.H, x.W)
        pads = 1 if nopad_lo else 2
        Ho, Wo = (Hv + pads - 3) // stride + 1, (Wv + pads - 3) // stride + 1
        out = rec.empty(B, Ho * Wo, Cout, dtype=torch.float32 if out_f32 else torch.float16)
        kw = {}
        if R is not None:
            kw.update(R=R.t, ldr=R.C)
        rec.gemm(A=x.t, W=self.h[name + ".weight"], M=B * Ho * Wo, N=Cout, K=9 * x.C, out=out,
                 out_mode=_lib.OUT_F32 if out_f32 else _lib.OUT_F16,
                 conv=dict(Cin=x.C, Hin=x.H, Win=x.W, Hv=Hv, Wv=Wv, Hout=Ho, Wout=Wo, stride=stride, nopad_lo=nopad_lo),
                 bias=self.f[name + ".bias"], rows_per_batch=Ho * Wo, want_gn=want_gn and not out_f32, kind="vae_conv", **kw)
        return _Act(out, Cout, Ho, Wo)

    def _dense(self, rec, x_t, M, K, wkey, bkey, N, rows_per_batch=0, **kw):
        out = kw.pop("out", None)
        if out is None:
            out = rec.empty(M, N)
        rec.gemm(A=x_t, W=self.h[wkey], M=M, N=N, K=K, out=out, bias=self.f[bkey] if bkey else None,
                 rows_per_batch=rows_per_batch, kind="vae_dense", **kw)
        return out

    def _gn(self, rec, B, x: _Act, name, silu=True):
        out = rec.groupnorm(x.t, x.C, None, 0, B, x.H * x.W, self.G, 1e-6, self.f[name + ".weight"], self.f[name + ".bias"], silu)
        return _Act(out, x.C, x.H, x.W)

    def _res(self, rec, B, p, x: _Act, Cout):
        h = self._gn(rec, B, x, p + "norm1")
        h = self._conv(rec, B, h, p + "conv1", Cout)
        h = self._gn(rec, B, h, p + "norm2")
        if (p + "conv_shortcut.weight") in self.h:
            M = B * x.H * x.W
            sc = _Act(self._dense(rec, x.t, M, x.C, p + "conv_shortcut.weight", p + "conv_shortcut.bias", Cout), Cout, x.H, x.W)
        else:
            sc = x
        return self._conv(rec, B, h, p + "conv2", Cout, R=sc)

    @staticmethod
    def _attend(rec, qk, vt, s, o, B, N, Cc):
        """The mid-block attention of B images over packed buffers: qk [B N][2 Cc] (q | k), vt [B Cc][pad8(N)] (V transposed, pad columns
        zero), s [N][pad8(N)] (the scores, then the probabilities, of ONE image), o [B N][Cc]."""
        Np = pad8(N)
        for b in range(B):                                 # heads = 1, head_dim = C: plain GEMMs per image
            rec.gemm(A=qk, a_offset=b * N * 2 * Cc, lda=2 * Cc, W=qk, w_offset=b * N * 2 * Cc + Cc, M=N, N=N, K=Cc, out=s,
                     ldc=Np, alpha=Cc ** -0.5, kind="vae_attn", ldw=2 * Cc)
            rec.call("bc_softmax_rows", s.data_ptr(), N, N, Np, kind="softmax", keep=(s,))
            rec.gemm(A=s, lda=Np, W=vt, w_offset=b * Cc * Np, M=N, N=Cc, K=Np, out=o, out_offset=b * N * Cc, kind="vae_attn",
                     ldw=Np)

    def _mid(self, rec, B, p, x: _Act):
        x = self._res(rec, B, p + "resnets.0.", x, x.C)
        a = p + "attentions.0."
        Cc, N = x.C, x.H * x.W
        if N % 8:
            raise ValueError("VAE attention needs a token count that is a multiple of 8")
        M = B * N
        n = self._gn(rec, B, x, a + "group_norm", silu=False)
        qk = self._dense(rec, n.t, M, Cc, a + "to_qk.weight", a + "to_qk.bias", 2 * Cc)
        vt = rec.zeros(B, Cc, pad8(N))
        self._dense(rec, n.t, M, Cc, a + "to_v.weight", a + "to_v.bias", Cc, rows_per_batch=N, out=vt,
                    out_mode=_lib.OUT_F16_T, ldc=pad8(N))
        o = rec.empty(M, Cc)
        Np = pad8(N)
        s = rec.zeros(N, Np)                               # scores of ONE image (images run back to back on the stream)
        self._attend(rec, qk, vt, s, o, B, N, Cc)
        out = self._dense(rec, o, M, Cc, a + "to_out.0.weight", a + "to_out.0.bias", Cc, rows_per_batch=N, R=x.t, ldr=Cc,
                          want_gn=True)
        return self._res(rec, B, p + "resnets.1.", _Act(out, Cc, x.H, x.W), Cc)

    # ------------------------------------------------------------------------------------------------ plans
    def to(self, *a, **k):
        return self

    def _need_gpu(self):
        if self.device.type != "cuda":
            raise _lib.BlobCtrlHipError("blobctrl_amd.AutoencoderKL runs on MI355X only; there is no CPU fallback")

    def _plan_decode(self, B, h, w):
        self._need_gpu()
        key = ("dec", B, h, w)
        if key in self._plans:
            return self._plans[key]
        rec = Recorder(self.device)
        P = type("Plan", (), {})()
        P.rec = rec
        Cz = self.latent_channels
        P.z = rec.zeros(B, h * w, 8)                                    # latent channels padded to 8
        P.seg = rec.begin("vae_decode")
        zp = rec.zeros(B, h * w, 8)                                     # post-quant output, again padded to 8 channels
        self._dense(rec, P.z, B * h * w, 8, "post_quant_conv.weight", "post_quant_conv.bias", Cz, out=zp, ldc=8)
        x = _Act(zp, 8, h, w)
        rev = [self.h[f"decoder.up_blocks.{i}.resnets.0.conv1.weight"].shape[0] for i in range(4)]
        x = self._conv(rec, B, x, "decoder.conv_in", rev[0])
        x = self._mid(rec, B, "decoder.mid_block.", x)
        i = 0
        while f"decoder.up_blocks.{i}.resnets.0.conv1.weight" in self.h:
            for j in range(self.lpb + 1):
                x = self._res(rec, B, f"decoder.up_blocks.{i}.resnets.{j}.", x, rev[i])
            if f"decoder.up_blocks.{i}.upsamplers.0.conv.weight" in self.h:
                x = self._conv(rec, B, x, f"decoder.up_blocks.{i}.upsamplers.0.conv", rev[i], up=True)
            i += 1
        x = self._gn(rec, B, x, "decoder.conv_norm_out")
        P.img = self._conv(rec, B, x, "decoder.conv_out", self.h["decoder.conv_out.weight"].shape[0], out_f32=True)
        self._plans[key] = P
        return P

    def _plan_encode(self, B, H, W):
        self._need_gpu()
        key = ("enc", B, H, W)
        if key in self._plans:
            return self._plans[key]
        rec = Recorder(self.device)
        P = type("Plan", (), {})()
        P.rec = rec
        P.x = rec.zeros(B, H * W, 8)                                    # RGB padded to 8 channels
        P.seg = rec.begin("vae_encode")
        x = _Act(P.x, 8, H, W)
        boc = [self.h[f"encoder.down_blocks.{i}.resnets.0.conv1.weight"].shape[0] for i in range(4)]
        x = self._conv(rec, B, x, "encoder.conv_in", boc[0])
        i = 0
        while f"encoder.down_blocks.{i}.resnets.0.conv1.weight" in self.h:
            for j in range(self.lpb):
                x = self._res(rec, B, f"encoder.down_blocks.{i}.resnets.{j}.", x, boc[i])
            if f"encoder.down_blocks.{i}.downsamplers.0.conv.weight" in self.h:
                x = self._conv(rec, B, x, f"encoder.down_blocks.{i}.downsamplers.0.conv", boc[i], stride=2, nopad_lo=True)
            i += 1
        x = self._mid(rec, B, "encoder.mid_block.", x)
        x = self._gn(rec, B, x, "encoder.conv_norm_out")
        Cm = 2 * self.latent_channels
        x = self._conv(rec, B, x, "encoder.conv_out", Cm, want_gn=False)
        P.moments = self._dense(rec, x.t, B * x.H * x.W, Cm, "quant_conv.weight", "quant_conv.bias", Cm)
        P.hw = (x.H, x.W)
        self._plans[key] = P
        return P

    # ------------------------------------------------------------------------------------------------ tiling / slicing
    def enable_tiling(self, use_tiling: bool = True):
        """Encode / decode inputs above the tile size as overlapping tiles blended together (autoencoder_kl.py:143-149).  The result
        differs from the plain one: every tile has its own GroupNorm statistics and its own mid-block attention."""
        self.use_tiling = use_tiling

    def disable_tiling(self):
        self.enable_tiling(False)

    def enable_slicing(self):
        """Encode / decode a batch one sample at a time (autoencoder_kl.py:158-163)."""
        self.use_slicing = True

    def disable_slicing(self):
        self.use_slicing = False

    def _tiles(self, kind, H, W):
        """The tile grid of an input, every tile checked against the mid-block attention's limit BEFORE anything is launched."""
        scale = 2 ** (len(self.config.block_out_channels) - 1)
        geo = tile_geometry(kind, H, W, self.tile_sample_min_size, self.tile_latent_min_size, self.tile_overlap_factor, scale)
        for t in geo["tiles"]:
            if kind == "encode" and (t["in_h"] % scale or t["in_w"] % scale):
                raise ValueError(f"tiled encode: tile {t['in_h']}x{t['in_w']} at ({t['y0']}, {t['x0']}) is not a multiple of {scale} pixels")
            lh, lw = (t["in_h"], t["in_w"]) if kind == "decode" else (t["out_h"], t["out_w"])
            if (lh * lw) % 8:
                raise ValueError(f"tiled {kind}: tile {t['in_h']}x{t['in_w']} at ({t['y0']}, {t['x0']}) has {lh}x{lw} = {lh * lw} latent "
                                 "tokens; VAE attention needs a token count that is a multiple of 8")
        return geo

    def _blend(self, src, keeps, t, out, mode, B, H, W):
        """One bc_vae_tile_blend launch on the caller's stream: tile `t` (plan output `src`) against its neighbours' keep-buffers."""
        above = keeps.get((t["i"] - 1, t["j"]))
        left = keeps.get((t["i"], t["j"] - 1))
        keep = torch.empty(B, t["out_h"], t["out_w"], 3 if mode == _lib.VAE_TILE_DECODE else 8, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.bc_vae_tile_blend(
            src.data_ptr(), above.data_ptr() if above is not None else None, left.data_ptr() if left is not None else None,
            keep.data_ptr(), out.data_ptr(), mode, B, t["out_h"], t["out_w"], above.shape[1] if above is not None else 0,
            left.shape[2] if left is not None else 0, t["ev"], t["eh"], t["oy"], t["ox"], t["ch"], t["cw"], H, W,
            torch.cuda.current_stream().cuda_stream), "bc_vae_tile_blend")
        keeps[(t["i"], t["j"])] = keep
        keeps.pop((t["i"] - 2, t["j"]), None)            # (two tile rows of keep-buffers are alive at a time)

    def _tiled_decode(self, z):
        B, Cz, h, w = z.shape
        geo = self._tiles("decode", h, w)
        if self.h["decoder.conv_out.weight"].shape[0] != 3:
            raise ValueError("tiled decode blends 3-channel images (bc_vae_tile_blend)")
        for t in geo["tiles"]:
            self._plan_decode(B, t["in_h"], t["in_w"])    # (every plan recorded before the first launch: a refusal launches nothing)
        s = torch.cuda.current_stream().cuda_stream
        H, W = geo["out_h"], geo["out_w"]
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=self.device)
        keeps = {}
        for t in geo["tiles"]:                             # row-major: above and left are blended before they are read
            P = self._plan_decode(B, t["in_h"], t["in_w"])
            zt = z[:, :, t["y0"]:t["y0"] + t["in_h"], t["x0"]:t["x0"] + t["in_w"]].contiguous()
            _lib.check(self.lib.bc_nchw_to_nhwc_f16(zt.data_ptr(), 1, B, Cz, t["in_h"] * t["in_w"], 8, P.z.data_ptr(), s),
                       "bc_nchw_to_nhwc_f16")
            run_graphed(P.seg, self.device)
            # the plan's image lives in its arena and the next tile of this shape overwrites it: the blend is enqueued on the caller's
            # stream now, and the next replay waits for that stream
            self._blend(P.img.t, keeps, t, out, _lib.VAE_TILE_DECODE, B, H, W)
        return out

    def _tiled_encode(self, x):
        B, _, Hi, Wi = x.shape
        geo = self._tiles("encode", Hi, Wi)
        if 2 * self.latent_channels != 8:
            raise ValueError("tiled encode blends 8 moment channels (bc_vae_tile_blend): latent_channels must be 4")
        for t in geo["tiles"]:
            self._plan_encode(B, t["in_h"], t["in_w"])
        s = torch.cuda.current_stream().cuda_stream
        h, w = geo["out_h"], geo["out_w"]
        mom = torch.empty(B, h * w, 2 * self.latent_channels, dtype=torch.float16, device=self.device)
        keeps = {}
        for t in geo["tiles"]:
            P = self._plan_encode(B, t["in_h"], t["in_w"])
            xt = x[:, :, t["y0"]:t["y0"] + t["in_h"], t["x0"]:t["x0"] + t["in_w"]].contiguous()
            _lib.check(self.lib.bc_nchw_to_nhwc_f16(xt.data_ptr(), 1, B, 3, t["in_h"] * t["in_w"], 8, P.x.data_ptr(), s),
                       "bc_nchw_to_nhwc_f16")
            run_graphed(P.seg, self.device)
            self._blend(P.moments, keeps, t, mom, _lib.VAE_TILE_ENCODE, B, h, w)
        return mom, h, w

    # ------------------------------------------------------------------------------------------------ API
    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = False, generator=None):
        """z [B, Cz, h, w] (already divided by the scaling factor) -> (image [B, 3, 8h, 8w] fp32,)."""
        B, Cz, h, w = z.shape
        if Cz != self.latent_channels:
            raise ValueError(f"expected {self.latent_channels} latent channels, got {Cz}")
        if self.use_slicing and B > 1:
            return (torch.cat([self._decode(z[b:b + 1]) for b in range(B)]),)
        return (self._decode(z),)

    def _decode(self, z):
        B, Cz, h, w = z.shape
        self._need_gpu()
        zz = z.to(self.device, torch.float32).contiguous()
        if self.use_tiling and (w > self.tile_latent_min_size or h > self.tile_latent_min_size):
            return self._tiled_decode(zz)
        P = self._plan_decode(B, h, w)
        s = torch.cuda.current_stream().cuda_stream
        _lib.check(self.lib.bc_nchw_to_nhwc_f16(zz.data_ptr(), 1, B, Cz, h * w, 8, P.z.data_ptr(), s), "bc_nchw_to_nhwc_f16")
        run_graphed(P.seg, self.device)
        img = P.img
        return img.t.view(B, img.H, img.W, img.C).permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def encode(self, x: torch.Tensor):
        """x [B, 3, H, W] in [-1, 1] -> object with `.latent_dist` (sample(generator) / mode() / parameters)."""
        B, C, H, W = x.shape
        if C != 3 or H % 8 or W % 8:
            raise ValueError("image must be [B,3,H,W] with H, W multiples of 8")
        self._need_gpu()
        xx = x.to(self.device, torch.float32).contiguous()
        out = type("AutoencoderKLOutput", (), {})()
        if self.use_tiling and (W > self.tile_sample_min_size or H > self.tile_sample_min_size):
            mom, h, w = self._tiled_encode(xx)                         # (the tiling test comes first, as in the reference)
        elif self.use_slicing and B > 1:
            parts = []
            for b in range(B):                                         # (one batch-1 plan: its moments are copied out before the next replay)
                m, (h, w) = self._encode_moments(xx[b:b + 1])
                parts.append(m.clone())
            mom = torch.cat(parts)
        else:
            mom, (h, w) = self._encode_moments(xx)
        out.latent_dist = _Dist(self, mom, B, h, w)
        return out

    def _encode_moments(self, xx):
        """The encode plan of xx's shape replayed on it: (moments [B * h * w, 8] fp16 in the plan's arena, (h, w))."""
        B, _, H, W = xx.shape
        P = self._plan_encode(B, H, W)
        s = torch.cuda.current_stream().cuda_stream
        _lib.check(self.lib.bc_nchw_to_nhwc_f16(xx.data_ptr(), 1, B, 3, H * W, 8, P.x.data_ptr(), s), "bc_nchw_to_nhwc_f16")
        run_graphed(P.seg, self.device)
        return P.moments, P.hw
