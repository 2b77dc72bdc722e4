"""Zoomed edits on the GPU against Pillow and the host restatement of blobctrl_amd/overlay.py (which tests/test_overlay_cpu.py holds to
Pillow and to the reference processor): equality, no tolerance.  The raw launches run in buffers fenced with 0xA5 that must survive."""
import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter

pytestmark = pytest.mark.gpu

from blobctrl_amd import _lib, blob_edit, overlay  # noqa: E402
from blobctrl_amd.image_processor import VaeImageProcessor  # noqa: E402
from tests import overlay_common as oc  # noqa: E402

DEV = "cuda:0"
SENTINEL = 0xA5
GUARD = 64


class Fenced:
    """A tensor `shape` of `dtype` inside a buffer filled with 0xA5, at least 64 guard bytes on both sides (`lead` of them in front: an odd
    lead makes the view's base unaligned); `check()` asserts that the buffer outside the view is untouched."""

    def __init__(self, shape, dtype=torch.uint8, lead=GUARD):
        self.bytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.lead = lead
        self.buf = torch.full((lead + self.bytes + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.view = self.buf[lead:lead + self.bytes].view(dtype).view(*shape)

    def fill(self, array):
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(array)))
        return self

    def check(self):
        assert bool((self.buf[:self.lead] == SENTINEL).all()) and bool((self.buf[self.lead + self.bytes:] == SENTINEL).all()), "wrote outside its view"
        return self.view.cpu().numpy()


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def up(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


# the issue's frames (3 x 70 both ways), and one row wider than two of a workgroup's stretches of 1024 pixels
BLUR_FRAMES_GPU = ((1, 1), (3, 70), (70, 3), (37, 53), (130, 129), (2, 2100))
BLUR_FACTORS_GPU = oc.BLUR_FACTORS + (64,)           # 32 and 64: a halo of 96 and 192 lines, beyond the 64 rows of a column tile


@pytest.mark.parametrize("H,W", BLUR_FRAMES_GPU)
def test_blur_launches_are_the_host_passes_and_stay_in_their_views(H, W):
    lib = _lib.load()
    for n in (1, 3):
        src_np = np.stack([oc.blob_mask(H, W, 70 + i, hard=i == 1) for i in range(n)])
        src = Fenced((n, H, W), lead=GUARD + 3).fill(src_np)                              # an unaligned base
        for factor in BLUR_FACTORS_GPU:
            R, ww, fw = overlay.blur_params(factor)
            rows_want = src_np
            for _ in range(3):
                rows_want = overlay.box_blur_lines(rows_want, R, ww, fw)
            want = overlay.gaussian_blur_reference(src_np, factor)
            tmp, out = Fenced((n, H, W), lead=GUARD + 1), Fenced((n, H, W))
            assert lib.bc_box_blur3_rows(src.view.data_ptr(), n, H, W, R, ww, fw, tmp.view.data_ptr(), stream()) == 0, lib.bc_last_error()
            assert lib.bc_box_blur3_cols(tmp.view.data_ptr(), n, H, W, R, ww, fw, out.view.data_ptr(), stream()) == 0, lib.bc_last_error()
            assert np.array_equal(tmp.check(), rows_want), (n, factor, "rows")
            assert np.array_equal(out.check(), want), (n, factor, "cols")
        assert np.array_equal(src.check(), src_np)


def test_blur_is_pillows_gaussian_blur():
    batch = np.stack([oc.blob_mask(130, 129, 5), oc.blob_mask(130, 129, 6, hard=True)])
    for factor in (1, 4, 32):
        got = overlay.blur(up(batch), factor).cpu().numpy()
        for a, g in zip(batch, got):
            assert np.array_equal(np.array(Image.fromarray(a).filter(ImageFilter.GaussianBlur(factor))), g), factor
    one = VaeImageProcessor.blur(up(batch[0]))                                            # the reference's default factor, 4
    assert one.shape == (130, 129) and np.array_equal(one.cpu().numpy(), overlay.gaussian_blur_reference(batch[0], 4))
    assert torch.equal(overlay.blur(up(batch[0]), 0), up(batch[0]))
    g = oc.golden()
    for name, ((H, W), factor, seed) in oc.BLUR_GOLDEN.items():
        got = overlay.blur(up(oc.blob_mask(H, W, seed, hard="hard" in name)), factor)
        assert np.array_equal(got.cpu().numpy(), g[f"blur_{name}"]), name


def bounds_masks(H, W):
    masks = {"empty": np.zeros((H, W), np.uint8), "full": np.full((H, W), 7, np.uint8)}
    for name, (y, x) in {"tl": (0, 0), "tr": (0, W - 1), "bl": (H - 1, 0), "br": (H - 1, W - 1)}.items():
        masks[name] = np.zeros((H, W), np.uint8)
        masks[name][y, x] = 1
    masks["blob"] = np.where(oc.blob_mask(H, W, 9) > 250, 255, 0).astype(np.uint8)
    masks["blob"][:, :1] = 0
    return masks


@pytest.mark.parametrize("H,W", [(37, 53), (300, 1), (1, 1), (5, 1100)])
def test_mask_bounds(H, W):
    lib = _lib.load()
    masks = bounds_masks(H, W)
    batch = np.stack(list(masks.values()))
    n = len(batch)
    src = Fenced((n, H, W), lead=GUARD + 1).fill(batch)
    ext, out = Fenced((n, H, 2), torch.int32), Fenced((n, 4), torch.int32)
    assert lib.bc_mask_bounds(src.view.data_ptr(), n, H, W, ext.view.data_ptr(), out.view.data_ptr(), stream()) == 0, lib.bc_last_error()
    want = [overlay.bounds_reference(m) for m in batch]
    ext.check()
    assert out.check().tolist() == [list(w) for w in want]
    assert want[0] == (-1, -1, -1, -1) and want[1] == (0, W - 1, 0, H - 1)
    assert overlay.mask_bounds(up(batch)).cpu().tolist() == [list(w) for w in want]
    assert overlay.mask_bounds(up(batch[1])).cpu().tolist() == list(want[1])


def composite_want(mask, init, patches, x, y):
    H, W = mask.shape
    res = []
    for p in patches:
        d = np.zeros((H, W, 3), np.uint8)
        d[y:y + p.shape[0], x:x + p.shape[1]] = p
        res.append(overlay.overlay_pixels(init, mask[:, :, None], d))
    return np.stack(res)


@pytest.mark.parametrize("h,w,x,y", [(37, 53, 0, 0), (10, 17, 0, 0), (10, 17, 36, 27), (1, 1, 20, 11), (36, 1, 52, 1)])
def test_the_composite_launch(h, w, x, y):
    """37 x 53 with all 256 mask values: the whole frame (no crop), a patch at (0, 0), one flush with the far corner, 1 x 1; n = 2."""
    lib = _lib.load()
    H, W = 37, 53
    mask, init_np, _ = oc.overlay_frame_inputs(H, W, 21)
    patches = np.stack([oc.rgb_image(h, w, 300), oc.rgb_image(h, w, 301)])
    m, init, pt = Fenced((H, W), lead=GUARD + 1).fill(mask), Fenced((H, W, 3), lead=GUARD + 2).fill(init_np), Fenced((2, h, w, 3), lead=GUARD + 3).fill(patches)
    want = composite_want(mask, init_np, patches, x, y)
    for lead in (GUARD, GUARD + 1):                                                        # the 32-bit and the byte stores
        out = Fenced((2, H, W, 3), lead=lead)
        assert lib.bc_overlay_composite(init.view.data_ptr(), m.view.data_ptr(), pt.view.data_ptr(), 2, H, W, h, w, x, y, out.view.data_ptr(),
                                        stream()) == 0, lib.bc_last_error()
        assert np.array_equal(out.check(), want), lead
    m.check(), init.check(), pt.check()


def test_apply_overlay_is_the_reference_processors():
    g = oc.golden()
    proc = VaeImageProcessor()
    for name in oc.OVERLAY_CASES:
        mask, init, image, crop = oc.overlay_inputs(name)
        got = overlay.apply_overlay(up(mask), up(init), up(image), crop)
        assert got.shape == image.shape and np.array_equal(got.cpu().numpy(), g[f"overlay_{name}"]), name
        assert torch.equal(proc.apply_overlay(up(mask), up(init), up(image), crop), got)
        two = overlay.apply_overlay(up(mask), up(init), up(np.stack([image, init])), crop)   # num_images_per_prompt = 2
        assert torch.equal(two[0], got) and np.array_equal(two[1].cpu().numpy(), overlay.apply_overlay_reference(mask, init, init, crop)), name
    mask, init, image = oc.overlay_resized_inputs()
    assert np.array_equal(overlay.apply_overlay(up(mask), up(init), up(image)).cpu().numpy(), g["overlay_resized"])


def test_crop_and_resize_and_the_resize_modes_are_the_reference_processors():
    g = oc.golden()
    proc = VaeImageProcessor()
    for name, ((H, W), (width, height), seed) in oc.RESIZE_CASES.items():
        img = oc.rgb_image(H, W, seed)
        whole = overlay.crop_and_resize(up(img), (0, 0, W, H), (height, width))
        assert np.array_equal(whole.cpu().numpy(), g[f"fill_{name}"]), name
        assert torch.equal(proc.resize(up(img), height, width, resize_mode="fill"), whole)
        assert np.array_equal(proc.resize(up(img), height, width, resize_mode="crop").cpu().numpy(), g[f"fit_{name}"]), name
        box = (W // 5, H // 4, W - 1, H - 2)
        part = overlay.crop_and_resize(up(np.stack([img, img[::-1]])), box, (height, width))
        for got, src in zip(part, (img, img[::-1])):
            want = overlay.resize_and_fill_reference(src[box[1]:box[3], box[0]:box[2]], width, height)
            assert np.array_equal(got.cpu().numpy(), want), name
    with pytest.raises(ValueError, match="leaves"):
        overlay.crop_and_resize(up(oc.rgb_image(8, 8, 1)), (0, 0, 9, 8), (16, 16))


def test_crop_region_is_the_reference_processors():
    g = oc.golden()
    for name, ((H, W), box, (width, height), pad) in oc.CROP_CASES.items():
        want = tuple(int(v) for v in g[f"crop_{name}"])
        assert overlay.crop_region(up(oc.box_mask(H, W, *box)), width, height, pad) == want, name
    (H, W), box, (width, height), pad = oc.CROP_CASES["wider"]
    both = up(np.stack([oc.box_mask(H, W, *box), oc.box_mask(H, W, *oc.CROP_CASES["taller"][1])]))
    assert VaeImageProcessor.get_crop_region(both, width, height, pad) == [tuple(int(v) for v in g["crop_wider"]), tuple(int(v) for v in g["crop_taller"])]
    with pytest.raises(ValueError, match="empty"):
        overlay.crop_region(up(np.zeros((4, 5), np.uint8)), 512, 512)


def test_to_uint8_is_postprocess_pil():
    x = torch.from_numpy(oc.rng(8).uniform(-1.2, 1.2, (2, 3, 9, 11)).astype(np.float32))
    x[0, :, 0, :4] = torch.tensor([-1.0, 1.0, 0.0, (2 * 100.5 / 255) - 1])
    want = np.stack([np.array(i) for i in VaeImageProcessor().postprocess(x, "pil")])
    assert np.array_equal(overlay.to_uint8(x.to(DEV)).cpu().numpy(), want)
    assert np.array_equal(overlay.to_uint8(x.to(DEV).half()).cpu().numpy(),
                          np.stack([np.array(i) for i in VaeImageProcessor().postprocess(x.to(DEV).half(), "pil")]))


START, TARGET = ((30.5, 40.25), (24.0, 14.0), 20.0), ((52.0, 36.0), (18.0, 26.0), -35.0)


def test_zoom_edit_maps_the_ellipses_by_the_closed_form():
    H, W, height, width, pad = 80, 96, 64, 96, 5
    image = oc.rgb_image(H, W, 77)
    crop, zoomed, mask, s_e, t_e = overlay.zoom_edit(up(image), START, TARGET, height=height, width=width, pad=pad)
    union = np.maximum(blob_edit.ellipse_mask(START, H, W), blob_edit.ellipse_mask(TARGET, H, W))
    assert np.array_equal(mask.cpu().numpy(), union)
    assert crop == overlay.crop_region_reference(union, width, height, pad)
    x1, y1, x2, y2 = crop
    assert np.array_equal(zoomed.cpu().numpy(), overlay.resize_and_fill_reference(image[y1:y2, x1:x2], width, height))
    cw, ch = x2 - x1, y2 - y1
    src_w = width if width / height < cw / ch else cw * height // ch
    src_h = height if width / height >= cw / ch else ch * width // cw
    s, ox, oy = src_w / cw, width // 2 - src_w // 2, height // 2 - src_h // 2
    for got, e in ((s_e, START), (t_e, TARGET)):
        assert got == (((e[0][0] - x1 + 0.5) * s - 0.5 + ox, (e[0][1] - y1 + 0.5) * s - 0.5 + oy), (e[1][0] * s, e[1][1] * s), e[2])
    # the mapped ellipse covers in the zoomed frame what the original covers in the crop, up to the resampling of its outline
    inner = blob_edit.ellipse_mask(s_e, height, width)[oy:oy + src_h, ox:ox + src_w] > 0
    assert abs(int(inner.sum()) - int((blob_edit.ellipse_mask(START, H, W)[y1:y2, x1:x2] > 0).sum()) * s * s) < 0.1 * inner.sum()


def test_a_round_trip_keeps_the_original_where_the_blurred_mask_is_zero():
    H, W = 80, 96                                                                       # a 96 x 80 frame edited at its own size
    image = oc.rgb_image(H, W, 78)
    crop, zoomed, mask, _, _ = overlay.zoom_edit(up(image), START, TARGET, height=H, width=W, pad=8)
    result = (255 - zoomed).permute(2, 0, 1)[None].float() / 127.5 - 1.0                  # a fake "result" in [-1, 1]: the negative
    fake = overlay.to_uint8(result)[0]
    assert (fake.int() - (255 - zoomed).int()).abs().max() <= 1
    soft = overlay.blur(mask, 2)
    out = overlay.apply_overlay(soft, up(image), fake, crop).cpu().numpy()
    soft, fake, (x1, y1, x2, y2) = soft.cpu().numpy(), fake.cpu().numpy(), crop
    assert 0 < (soft == 0).sum() < H * W and (soft == 255).any() and ((soft > 0) & (soft < 255)).any()
    assert not soft[:y1].any() and not soft[y2:].any() and not soft[:, :x1].any() and not soft[:, x2:].any()      # the pad holds the blur
    assert np.array_equal(out[soft == 0], image[soft == 0])
    pasted = np.zeros_like(image)
    pasted[y1:y2, x1:x2] = overlay.resize_and_crop_reference(fake, x2 - x1, y2 - y1)
    assert np.array_equal(out[soft == 255], pasted[soft == 255]) and not np.array_equal(out, image)
    assert np.array_equal(out, overlay.apply_overlay_reference(soft, image, fake, crop))
