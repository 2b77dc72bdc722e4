"""Pillow's 8-bit resize on the GPU (blobctrl_amd/resample.py, csrc/image_resample.hip) against Pillow and the host processors it stands
for.  Everything is integer arithmetic and a lookup, so every comparison is `torch.equal` / `np.array_equal`: no tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from blobctrl_amd import resample, sam  # noqa: E402
from blobctrl_amd.image_processor import Dinov2ImageProcessor  # noqa: E402
from tests import image_resample_common as rc  # noqa: E402

DEV = "cuda:0"
SENTINEL = 0xA5
PAD = 67                                              # bytes of sentinel before and after a view (odd: the views end up unaligned)


class Fenced:
    """A uint8 tensor `shape` inside a sentinel-filled buffer; `check()` asserts that the buffer outside it is untouched."""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.view = self.buf[PAD:PAD + self.n].view(*shape)

    def check(self):
        assert bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.n:] == SENTINEL).all()), "wrote outside its view"
        return self.view


def up(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                               # (a copy: the shared images are read-only)


@pytest.mark.parametrize("name", rc.FILTERS)
def test_resize_images_is_pillow(name):
    for H, W, oh, ow in rc.CASES:
        batch = up(np.stack([rc.image(H, W, 0), rc.image(H, W, 1)]))
        want = up(np.stack([rc.pillow(H, W, oh, ow, name, 0), rc.pillow(H, W, oh, ow, name, 1)]))
        assert not torch.equal(batch[0], batch[1])
        out = Fenced((2, oh, ow, 3))
        shape = resample.temp_shape(H, W, (oh, ow), name)
        assert (shape is None) == (oh == H or ow == W)
        tmp = Fenced((2,) + shape) if shape else None
        got = resample.resize_images(batch, (oh, ow), name, out=out.view, tmp=tmp.view if tmp else None)
        assert got is out.view and torch.equal(out.check(), want), (H, W, oh, ow, name)
        if tmp:
            tmp.check()
        one = resample.resize_images(batch[1], (oh, ow), name)                             # one image, memory of its own
        assert one.shape == (oh, ow, 3) and torch.equal(one, want[1]), (H, W, oh, ow, name)


@pytest.mark.parametrize("H,W,oh,ow", [(37, 53, 80, 91), (257, 130, 32, 41), (40, 40, 40, 17), (33, 1024, 8, 256), (64, 64, 64, 64),
                                       (13, 200, 40, 200)])
def test_windows_are_slices_of_the_full_result(H, W, oh, ow):
    src = up(np.stack([rc.image(H, W, 0), rc.image(H, W, 1)]))
    for name in rc.FILTERS:
        full = resample.resize_images(src, (oh, ow), name)
        assert torch.equal(full[0], up(resample.resize_reference(rc.image(H, W, 0), (oh, ow), name)))
        windows = [(oh // 3, ow // 3, max(1, oh // 2), max(1, ow // 2)),                    # interior
                   (0, ow // 4, max(1, oh // 3), max(1, ow // 2)), (oh - max(1, oh // 3), 0, max(1, oh // 3), max(1, ow // 2)),  # top, bottom + left
                   (oh // 4, ow - max(1, ow // 3), max(1, oh // 2), max(1, ow // 3)),          # right
                   (oh // 2, ow // 2, 1, 1), (0, 0, 1, 1), (oh - 1, ow - 1, 1, 1)]             # single pixels
        for y0, x0, h, w in windows:
            out = Fenced((2, h, w, 3))
            resample.resize_images(src, (oh, ow), name, window=(y0, x0, h, w), out=out.view)
            assert torch.equal(out.check(), full[:, y0:y0 + h, x0:x0 + w]), (name, y0, x0, h, w)
    for bad in [(0, 0, oh + 1, 1), (-1, 0, 1, 1), (0, ow, 1, 1), (0, 0, 0, 1)]:
        with pytest.raises(ValueError, match="leaves the resized frame"):
            resample.resize_images(src, (oh, ow), "bicubic", window=bad)


def test_dinov2_pixel_values_are_the_host_processors():
    small = Dinov2ImageProcessor(shortest_edge=32, crop_size=28)
    for proc, (H, W) in [(small, (40, 56)), (small, (56, 40)), (small, (64, 64)), (small, (20, 24)), (Dinov2ImageProcessor(), (300, 260))]:
        imgs = [rc.all_bytes_image(H, W, 0), rc.all_bytes_image(H, W, 1)]
        want = proc.preprocess(imgs)["pixel_values"]
        got = resample.dinov2_pixel_values(up(np.stack(imgs)), proc)
        assert got.dtype == torch.float32 and got.shape == want.shape == (2, 3, proc.crop_size, proc.crop_size)
        assert torch.equal(got.cpu(), want), (H, W)
        assert torch.equal(resample.dinov2_pixel_values(up(imgs[1]), proc).cpu(), want[1:]), (H, W)


@pytest.mark.parametrize("H,W,fmt", [(200, 150, "RGB"), (200, 150, "BGR"), (150, 200, "RGB"), (256, 256, "RGB"), (64, 256, "BGR")])
def test_sam_input_is_preprocess_image(H, W, fmt):
    image = rc.all_bytes_image(H, W)
    resized, x = sam.preprocess_image(image, 256, fmt)
    got_resized, got_x = resample.sam_input(up(image), 256, fmt)
    assert got_resized.dtype == torch.uint8 and torch.equal(got_resized.cpu(), torch.from_numpy(resized.copy()))
    assert got_x.dtype == torch.float32 and got_x.shape == x.shape == (1, 3, 256, 256) and torch.equal(got_x.cpu(), x)
    size, only_x = resample.sam_pixel_values(up(image), 256, fmt)                           # what set_image uses: no uint8 frame in between
    assert size == resized.shape[:2] and torch.equal(only_x.cpu(), x)
    if (H, W) == (200, 150):
        assert bool((got_x[0, :, :, 192:] == 0).all()) and not bool((got_x[0, :, :, :192] == 0).any())   # SAM's padding, and nothing else, is zero


def test_set_image_takes_a_device_tensor():
    from tests.test_sam_gpu import gold, model_of
    model, cfg = model_of("a")
    img = gold()["predictor_pre_image"]
    assert img.dtype == np.uint8 and img.shape == (200, 150, 3)
    host, dev = sam.SamPredictor(model), sam.SamPredictor(model)
    host.set_image(img)
    emb_host = host.get_image_embedding().clone()
    dev.set_image(up(img))
    assert dev.original_size == host.original_size == (200, 150) and dev.input_size == host.input_size == (256, 192)
    assert all(type(v) is int for v in dev.original_size + dev.input_size)
    assert torch.equal(dev.get_image_embedding(), emb_host)                                 # the same encoder on the same bytes
    masks, iou, low = dev.predict(np.array([[75.0, 100.0]]), np.array([1]), multimask_output=False)
    assert masks.shape == (1, 200, 150) and iou.shape == (1,) and low.shape == (1, 64, 64)
    dev.set_image(up(img[..., ::-1]), "BGR")
    assert torch.equal(dev.get_image_embedding(), emb_host)


def test_the_pipeline_embeds_a_device_image_without_the_host(monkeypatch):
    from PIL import Image
    from tests.test_edit_inputs_gpu import tiny_pipeline
    fg = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_call.npz"))["fg"]
    assert fg.dtype == np.uint8 and fg.ndim == 3
    pipe = tiny_pipeline("ddim")
    host = pipe.encode_image_dinov2(Image.fromarray(fg))
    assert torch.isfinite(host).all() and torch.equal(pipe.encode_image_dinov2(up(fg)), host)

    def crossed(*a, **k):
        raise AssertionError("the device image went to the host processor")

    monkeypatch.setattr(pipe.dinov2_processor, "preprocess", crossed)
    assert torch.equal(pipe.encode_image_dinov2(up(fg)), host)

    class Other(Dinov2ImageProcessor):                                                    # any other processor object keeps the host route
        calls = 0

        def preprocess(self, *a, **k):
            Other.calls += 1
            return Dinov2ImageProcessor.preprocess(self, *a, **k)

    pipe.dinov2_processor = Other()
    assert torch.equal(pipe.encode_image_dinov2(up(fg)), host) and Other.calls == 1


def test_offsets_past_two_to_the_31():
    """683 frames of 1024 x 1024 x 3 are 2^31 + 2^20 bytes.  As a source (every pass reads past 2^31: horizontal alone, vertical straight from
    the source, both through the intermediate), as a uint8 result, and as an fp32 result of as many bytes.  All frames but the last are
    the same, so the host computes two references and the device compares the rest among themselves."""
    n, S = 683, 1024
    A, B = rc.image(S, S, 0), rc.image(S, S, 1)
    src = torch.empty((n, S, S, 3), dtype=torch.uint8, device=DEV)
    src[:] = up(A)
    src[-1] = up(B)
    assert src.numel() > 2 ** 31
    for (oh, ow), name in (((S, 48), "bicubic"), ((40, S), "lanczos"), ((40, 48), "bilinear")):
        got = resample.resize_images(src, (oh, ow), name)
        assert torch.equal(got[0], up(rc.pillow(S, S, oh, ow, name, 0))) and torch.equal(got[-1], up(rc.pillow(S, S, oh, ow, name, 1)))
        assert bool((got[1:-1] == got[:1]).all()) and not torch.equal(got[0], got[-1])
    del src, got
    a, b = rc.image(16, 16, 0), rc.image(16, 16, 1)
    small = up(np.stack([a] * (n - 1) + [b]))
    big = resample.resize_images(small, (S, S), "bicubic")
    assert big.numel() > 2 ** 31
    assert torch.equal(big[0], up(rc.pillow(16, 16, S, S, "bicubic", 0))) and torch.equal(big[-1], up(rc.pillow(16, 16, S, S, "bicubic", 1)))
    assert bool((big[1:-1] == big[:1]).all()) and not torch.equal(big[0], big[-1])
    del big
    proc = Dinov2ImageProcessor(shortest_edge=512, crop_size=512)
    px = resample.dinov2_pixel_values(small, proc)                                          # 683 x 3 x 512 x 512 floats: 2^31 + 2^20 bytes
    assert px.numel() * 4 > 2 ** 31
    want = proc.preprocess([a, b])["pixel_values"]
    assert torch.equal(px[0].cpu(), want[0]) and torch.equal(px[-1].cpu(), want[1]) and bool((px[1:-1] == px[:1]).all())
