"""Host-side image pre/post-processing either side of the pipeline (no arithmetic worth a kernel: a few MB per edit on the host).

  * VaeImageProcessor      - D/image_processor.py:469-600 (preprocess) and :602-680 (postprocess) for the inputs the pipeline accepts:
                             PIL images (lanczos resize to (height, width) rounded down to a multiple of the VAE scale factor, THEN
                             RGB conversion, [0,1] -> [-1,1]), numpy arrays, tensors; outputs "latent" | "pt" | "np" | "pil".
                             Also the four functions of a zoomed edit - blur, get_crop_region, resize(resize_mode) and apply_overlay
                             (:184-407, :651-684) - for PIL images on the host and for uint8 device tensors through blobctrl_amd.overlay.
  * Dinov2ImageProcessor   - what `AutoImageProcessor.from_pretrained(dinov2_path)` resolves to for facebook/dinov2-* (transformers'
                             BitImageProcessor, called at pipeline_blobnet.py:696): RGB, bicubic resize of the SHORTEST edge to 256,
                             centre crop 224 x 224, 1/255, ImageNet mean / std.  Pinned against the installed BitImageProcessor
                             (tests/golden/image_processors.npz).
"""
from typing import List, Optional, Union

import numpy as np
import torch


def _pil():
    from PIL import Image
    return Image


class VaeImageProcessor:
    def __init__(self, vae_scale_factor: int = 8, do_resize: bool = True, resample: str = "lanczos", do_normalize: bool = True,
                 do_convert_rgb: bool = False, vae_latent_channels: int = 4):
        self.config = type("Config", (), dict(vae_scale_factor=vae_scale_factor, do_resize=do_resize, resample=resample,
                                              do_normalize=do_normalize, do_convert_rgb=do_convert_rgb))()
        self.vae_latent_channels = vae_latent_channels

    # ---- D/image_processor.py:426-467
    def get_default_height_width(self, image, height=None, width=None):
        Image = _pil()
        if height is None:
            height = image.height if isinstance(image, Image.Image) else (image.shape[2] if torch.is_tensor(image) else image.shape[1])
        if width is None:
            width = image.width if isinstance(image, Image.Image) else (image.shape[3] if torch.is_tensor(image) else image.shape[2])
        f = self.config.vae_scale_factor
        return height - height % f, width - width % f

    # ---- zoomed ("only masked") edits: D/image_processor.py:184-190, :193-280, :282-407 and :651-684.  A PIL image takes the host route,
    #      which is Pillow's own calls (blobctrl_amd.overlay's numpy restatement is the tests' yardstick, not a route); a uint8 device tensor
    #      takes that module's device half - the same bytes, on the GPU; a CPU tensor raises BlobCtrlHipError
    @staticmethod
    def blur(image, blur_factor: int = 4):
        if torch.is_tensor(image):
            from . import overlay
            return overlay.blur(image, blur_factor)
        from PIL import ImageFilter
        return image.filter(ImageFilter.GaussianBlur(blur_factor))

    @staticmethod
    def get_crop_region(mask_image, width: int, height: int, pad=0):
        from . import overlay
        if torch.is_tensor(mask_image):
            return overlay.crop_region(mask_image, width, height, pad)
        box = mask_image.convert("L").getbbox()                   # (left, top, right, bottom) of the non-zero pixels, None without any
        bounds = (-1, -1, -1, -1) if box is None else (box[0], box[2] - 1, box[1], box[3] - 1)
        return overlay.crop_region_from_bounds(bounds, mask_image.width, mask_image.height, width, height, pad)

    @staticmethod
    def _fit(image, width: int, height: int, crop: bool):
        """resize_mode "crop" (cover the frame, cut the excess) or "fill" (fit inside it, fill the bands from the image's edge lines)."""
        from . import overlay
        Image = _pil()
        src_w, src_h, ox, oy, band = overlay.fill_geometry(image.width, image.height, width, height)
        if crop:
            src_w, src_h = overlay._fit_sizes(image.width, image.height, width, height, True)
            ox, oy, band = width // 2 - src_w // 2, height // 2 - src_h // 2, None
        resized = image.resize((src_w, src_h), resample=Image.LANCZOS)
        res = Image.new("RGB", (width, height))
        res.paste(resized, box=(ox, oy))
        # a band is Image.resize of a box of zero extent on the edge it continues (overlay.band_tables says what Pillow makes of that)
        if band == "rows":
            for edge, y in ((0, 0), (src_h, oy + src_h)):
                res.paste(resized.resize((width, oy), box=(0, edge, width, edge)), box=(0, y))
        elif band == "cols":
            for edge, x in ((0, 0), (src_w, ox + src_w)):
                res.paste(resized.resize((ox, height), box=(edge, 0, edge, height)), box=(x, 0))
        return res

    def resize(self, image, height: int, width: int, resize_mode: str = "default"):
        """PIL images and uint8 device images [n][H][W][3] / [H][W][3]; resize_mode "default" | "fill" | "crop".  (The float tensor and
        numpy modes of the reference's `resize` are `preprocess`'s business here and are not taken.)"""
        if resize_mode not in ("default", "fill", "crop"):
            raise ValueError(f"resize_mode {resize_mode} is not supported")
        if torch.is_tensor(image):
            from . import overlay, resample
            if resize_mode == "default":
                if image.device.type != "cuda":
                    raise overlay._no_cpu("resize")
                return resample.resize_images(image, (height, width), self.config.resample)
            return (overlay.resize_fill if resize_mode == "fill" else overlay.resize_fit)(image, width, height)
        Image = _pil()
        if not isinstance(image, Image.Image):
            raise ValueError(f"Only PIL images and uint8 device tensors are supported for resize_mode {resize_mode}")
        if resize_mode == "default":
            rs = {"lanczos": Image.LANCZOS, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "nearest": Image.NEAREST}
            return image.resize((width, height), resample=rs[self.config.resample])
        return self._fit(image, width, height, resize_mode == "crop")

    def apply_overlay(self, mask, init_image, image, crop_coords=None):
        """The edit's output laid over the original through the mask: the original where the mask is 0, Pillow's blend elsewhere.  The
        frame is the image's; init and mask are resized to it."""
        if torch.is_tensor(image):
            from . import overlay
            return overlay.apply_overlay(mask, init_image, image, crop_coords)
        from PIL import Image, ImageOps
        size = image.size
        keep = ImageOps.invert(self.resize(mask, size[1], size[0]).convert("L"))            # alpha of the original: 255 where the mask is 0
        original = Image.new("RGBa", size)                                                  # premultiplied, transparent black
        original.paste(self.resize(init_image, size[1], size[0]).convert("RGBA").convert("RGBa"), mask=keep)
        if crop_coords is not None:
            x1, y1, x2, y2 = crop_coords
            canvas = Image.new("RGBA", size)
            canvas.paste(self.resize(image, y2 - y1, x2 - x1, resize_mode="crop"), (x1, y1))
            image = canvas.convert("RGB")                                                   # black outside the box
        out = image.convert("RGBA")
        out.alpha_composite(original.convert("RGBA"))
        return out.convert("RGB")

    def preprocess(self, image, height: Optional[int] = None, width: Optional[int] = None) -> torch.Tensor:
        Image = _pil()
        if not isinstance(image, list):
            image = [image]
        if not all(isinstance(i, (Image.Image, np.ndarray, torch.Tensor)) for i in image) or not image:
            raise ValueError("Input is in incorrect format. Currently, we only support PIL.Image.Image, np.ndarray, torch.Tensor")
        if isinstance(image[0], Image.Image):
            if self.config.do_resize:
                height, width = self.get_default_height_width(image[0], height, width)
                rs = {"lanczos": Image.LANCZOS, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "nearest": Image.NEAREST}
                image = [i.resize((width, height), resample=rs[self.config.resample]) for i in image]
            if self.config.do_convert_rgb:
                image = [i.convert("RGB") for i in image]
            arr = np.stack([np.array(i).astype(np.float32) / 255.0 for i in image], axis=0)
            if arr.ndim == 3:
                arr = arr[..., None]
            x = torch.from_numpy(arr.transpose(0, 3, 1, 2))
        elif isinstance(image[0], np.ndarray):
            arr = np.concatenate(image, axis=0) if image[0].ndim == 4 else np.stack(image, axis=0)
            if arr.ndim == 3:
                arr = arr[..., None]
            x = torch.from_numpy(arr.transpose(0, 3, 1, 2))
            height, width = self.get_default_height_width(x, height, width)
            if self.config.do_resize:
                x = torch.nn.functional.interpolate(x, size=(height, width))
        else:
            x = torch.cat(image, dim=0) if image[0].ndim == 4 else torch.stack(image, dim=0)
            if x.shape[1] == self.vae_latent_channels:            # already latents
                return x
            height, width = self.get_default_height_width(x, height, width)
            if self.config.do_resize:
                x = torch.nn.functional.interpolate(x, size=(height, width))
        if self.config.do_normalize and not (x.min() < 0):         # tensors already in [-1, 1] are passed through (:580-587)
            x = 2.0 * x - 1.0
        return x

    def postprocess(self, image: torch.Tensor, output_type: str = "pil", do_denormalize: Optional[List[bool]] = None):
        if output_type not in ("latent", "pt", "np", "pil"):
            output_type = "np"                                       # (:640-646: deprecation fallback)
        if output_type == "latent":
            return image
        if do_denormalize is None:
            do_denormalize = [self.config.do_normalize] * image.shape[0]
        image = torch.stack([(image[i] / 2 + 0.5).clamp(0, 1) if do_denormalize[i] else image[i] for i in range(image.shape[0])])
        if output_type == "pt":
            return image
        arr = image.cpu().permute(0, 2, 3, 1).float().numpy()
        if output_type == "np":
            return arr
        Image = _pil()
        u8 = (arr * 255).round().astype("uint8")
        if u8.shape[-1] == 1:
            return [Image.fromarray(a.squeeze(), mode="L") for a in u8]
        return [Image.fromarray(a) for a in u8]


class IPAdapterMaskProcessor(VaeImageProcessor):
    """D/image_processor.py:928-1029: the masks of `cross_attention_kwargs={"ip_adapter_masks": ...}`.  `preprocess(mask, height, width)`:
    lanczos resize to the call's height and width rounded down to multiples of `vae_scale_factor`, grayscale, binarised at 0.5, no
    normalisation -> [n][1][H][W] with values 0 and 1; the caller stacks an adapter's masks to [1][images][H][W]
    (`masks.reshape(1, masks.shape[0], masks.shape[2], masks.shape[3])`, as the reference's documentation does).
    The host route takes PIL images and uint8 numpy arrays ([H][W] or [H][W][C]; taken as the PIL image `Image.fromarray` makes of them)
    through Pillow and returns fp32 on the host.  The device route takes a uint8 device mask [H][W] or [n][H][W] (0 / 255, as
    `edit_inputs.ellipse_masks` leaves them) through blobctrl_amd.resample - Pillow's bytes - and returns uint8 on the device.  Both give
    the same values.  The downsampling to an attention level is no method here: blobctrl_amd.ip_masks does it into buffers a plan owns."""

    def __init__(self, do_resize: bool = True, vae_scale_factor: int = 8, resample: str = "lanczos", do_normalize: bool = False,
                 do_binarize: bool = True, do_convert_grayscale: bool = True):
        super().__init__(vae_scale_factor=vae_scale_factor, do_resize=do_resize, resample=resample, do_normalize=do_normalize)
        self.config.do_binarize, self.config.do_convert_grayscale = do_binarize, do_convert_grayscale

    def preprocess(self, image, height: Optional[int] = None, width: Optional[int] = None) -> torch.Tensor:
        Image = _pil()
        if torch.is_tensor(image) or (isinstance(image, list) and image and torch.is_tensor(image[0])):
            return self._preprocess_device(torch.stack(list(image)) if isinstance(image, list) else image, height, width)
        images = image if isinstance(image, list) else [image]
        if not images or not all(isinstance(i, (Image.Image, np.ndarray)) for i in images):
            raise ValueError("Input is in incorrect format. Currently, we only support PIL.Image.Image, np.ndarray, torch.Tensor")
        pil = []
        for i in images:
            if isinstance(i, np.ndarray):
                if i.dtype != np.uint8 or i.ndim not in (2, 3):
                    raise ValueError(f"a numpy mask is uint8 [H][W] or [H][W][C], not {i.dtype} {i.shape}")
                i = Image.fromarray(i[..., 0] if i.ndim == 3 and i.shape[-1] == 1 else i)
            pil.append(i)
        if self.config.do_resize:
            height, width = self.get_default_height_width(pil[0], height, width)
            pil = [self.resize(i, height, width) for i in pil]
        if self.config.do_convert_grayscale:
            pil = [i.convert("L") for i in pil]
        arr = np.stack([np.array(i).astype(np.float32) / 255.0 for i in pil], axis=0)
        x = torch.from_numpy(arr[..., None].transpose(0, 3, 1, 2) if arr.ndim == 3 else arr.transpose(0, 3, 1, 2))
        if self.config.do_binarize:
            x[x < 0.5] = 0
            x[x >= 0.5] = 1
        return x

    def _preprocess_device(self, mask, height, width):
        from . import resample
        if mask.device.type != "cuda":
            raise resample._no_cpu("IPAdapterMaskProcessor.preprocess")
        if mask.dtype != torch.uint8 or mask.ndim not in (2, 3):
            raise ValueError(f"a device mask is uint8 [H][W] or [n][H][W], not {mask.dtype} {tuple(mask.shape)}")
        m = mask[None] if mask.ndim == 2 else mask
        H, W = (m.shape[1] if height is None else height), (m.shape[2] if width is None else width)
        f = self.config.vae_scale_factor
        H, W = H - H % f, W - W % f
        if self.config.do_resize and (H, W) != tuple(m.shape[1:]):
            # a grayscale image resizes as each band of an RGB image does: the mask three times over, one band back
            m = resample.resize_images(m[..., None].expand(-1, -1, -1, 3), (H, W), self.config.resample)[..., 0]
        if self.config.do_binarize:
            m = (m >= 128).to(torch.uint8)                        # v / 255 >= 0.5
        else:
            m = m.to(torch.float32) / 255.0
        return m[:, None].contiguous()


class Dinov2ImageProcessor:
    """`dinov2_processor.preprocess(images=..., do_resize=True, return_tensors="pt", do_convert_rgb=True)` (pipe:696) for the
    facebook/dinov2 preprocessor_config.json values; returns an object with `.pixel_values` that is also a mapping (`**inputs`)."""

    def __init__(self, shortest_edge: int = 256, crop_size: int = 224, image_mean=(0.485, 0.456, 0.406),
                 image_std=(0.229, 0.224, 0.225), rescale_factor: float = 1 / 255):
        self.shortest_edge, self.crop_size = shortest_edge, crop_size
        self.image_mean, self.image_std, self.rescale_factor = tuple(image_mean), tuple(image_std), rescale_factor

    @classmethod
    def from_pretrained(cls, path, **_ignored):
        import json
        import os
        with open(os.path.join(path, "preprocessor_config.json")) as f:
            c = json.load(f)
        size = c.get("size", {"shortest_edge": 256})
        crop = c.get("crop_size", {"height": 224, "width": 224})
        return cls(size["shortest_edge"] if isinstance(size, dict) else int(size), crop["height"] if isinstance(crop, dict) else int(crop),
                   c.get("image_mean", (0.485, 0.456, 0.406)), c.get("image_std", (0.229, 0.224, 0.225)), c.get("rescale_factor", 1 / 255))

    def _one(self, img) -> np.ndarray:
        Image = _pil()
        if isinstance(img, np.ndarray):
            img = Image.fromarray(img)
        img = img.convert("RGB")
        w, h = img.size
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = self.shortest_edge, int(self.shortest_edge * long / short)
        nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
        img = img.resize((nw, nh), resample=Image.BICUBIC)
        top, left = (nh - self.crop_size) // 2, (nw - self.crop_size) // 2
        arr = np.array(img)[top:top + self.crop_size, left:left + self.crop_size].astype(np.float32) * np.float32(self.rescale_factor)
        arr = (arr - np.array(self.image_mean, np.float32)) / np.array(self.image_std, np.float32)
        return arr.transpose(2, 0, 1)

    def preprocess(self, images, do_resize=True, return_tensors="pt", do_convert_rgb=True, **_ignored):
        if not isinstance(images, (list, tuple)):
            images = [images]
        px = torch.from_numpy(np.stack([self._one(i) for i in images], 0))
        return _BatchFeature(pixel_values=px)

    __call__ = preprocess


CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


class CLIPImageProcessor(Dinov2ImageProcessor):
    """transformers' `CLIPImageProcessor(images=..., return_tensors="pt").pixel_values` with its Pillow backend, for an IP-Adapter's image
    encoder: RGB, bicubic resize of the shortest edge to `size` (the long edge truncated by int(...)), centre crop, 1 / 255, CLIP mean /
    std.  The geometry is Dinov2ImageProcessor's; the arithmetic differs in one rounding: the rescale multiplies in float64 and rounds
    to float32 once (transformers' `rescale`), then (x - mean) / std in float32."""

    def __init__(self, size=224, crop_size=224, image_mean=CLIP_MEAN, image_std=CLIP_STD, rescale_factor: float = 1 / 255):
        super().__init__(self._edge(size, "shortest_edge"), self._edge(crop_size, "height"), image_mean, image_std, rescale_factor)

    @staticmethod
    def _edge(v, key):
        """`size` / `crop_size` as a preprocessor_config.json spells them: a bare int or {"shortest_edge": n} / {"height": n, "width": n}."""
        if isinstance(v, dict):
            if key not in v or (key == "height" and v.get("width", v[key]) != v[key]):
                raise ValueError(f"CLIPImageProcessor takes {{'{key}': n}} (a square crop), got {v}")
            return int(v[key])
        return int(v)

    @property
    def size(self):
        return {"shortest_edge": self.shortest_edge}

    @classmethod
    def from_pretrained(cls, path, **_ignored):
        import json
        import os
        with open(os.path.join(path, "preprocessor_config.json")) as f:
            c = json.load(f)
        return cls(c.get("size", 224), c.get("crop_size", 224), c.get("image_mean", CLIP_MEAN), c.get("image_std", CLIP_STD),
                   c.get("rescale_factor", 1 / 255))

    def normalise(self, arr_u8: np.ndarray) -> np.ndarray:
        """uint8 [...][3] -> float32, channel last: the expression every pixel goes through after the crop (and resample.clip_lut's)."""
        arr = (arr_u8.astype(np.float64) * self.rescale_factor).astype(np.float32)
        return (arr - np.array(self.image_mean, np.float32)) / np.array(self.image_std, np.float32)

    def _one(self, img) -> np.ndarray:
        from .resample import dinov2_geometry
        Image = _pil()
        if isinstance(img, np.ndarray):
            img = Image.fromarray(img)
        img = img.convert("RGB")
        (nh, nw), (top, left, ch, cw) = dinov2_geometry(img.size[1], img.size[0], self.shortest_edge, self.crop_size)
        img = img.resize((nw, nh), resample=Image.BICUBIC)
        return self.normalise(np.array(img)[top:top + ch, left:left + cw]).transpose(2, 0, 1)


class _BatchFeature(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def to(self, device=None, dtype=None):
        return _BatchFeature({k: (v.to(device=device, dtype=dtype) if torch.is_tensor(v) and v.is_floating_point() else
                                  (v.to(device) if torch.is_tensor(v) else v)) for k, v in self.items()})
