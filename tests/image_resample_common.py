"""Shared by tests/test_image_resample_cpu.py and tests/test_image_resample_gpu.py: the shape cases, the seeded images and Pillow's results
(computed once per process and handed out read-only)."""
import functools

import numpy as np

# (H, W, out_h, out_w): 1 x 1 sources, a reduction to one pixel, big up-scales, no change, one axis unchanged, odd sizes, rows wider than a
# workgroup's span
CASES = [(1, 1, 5, 9), (300, 301, 1, 1), (2, 3, 67, 129), (64, 64, 64, 64), (64, 48, 33, 29), (37, 53, 80, 91), (40, 40, 40, 17),
         (13, 200, 13, 7), (5, 7, 3, 2), (257, 130, 32, 41), (200, 150, 256, 192), (33, 1024, 8, 256)]
FILTERS = ("bilinear", "bicubic", "lanczos")
# the cases that enlarge an image of more than a few pixels in both axes: where bicubic and lanczos overshoot next to a 0 / 255 edge
UPSCALING = [(37, 53, 80, 91), (200, 150, 256, 192)]
BLOCK = 4


def pil_filter(name):
    from PIL import Image
    return {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]


@functools.lru_cache(maxsize=None)
def image(H, W, seed=0):
    """Seeded random bytes [H][W][3]; one half (the right one, or the lower one of a narrow image) is 0 / 255 blocks of BLOCK pixels a side,
    so that the negative lobes of bicubic and lanczos overshoot and the clamp fires at both ends."""
    rng = np.random.default_rng(1000 * H + W + 7919 * seed)
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    by, bx = (H + BLOCK - 1) // BLOCK, (W + BLOCK - 1) // BLOCK
    blocks = (rng.integers(0, 2, (by, bx, 1), dtype=np.uint8) * 255).repeat(BLOCK, 0).repeat(BLOCK, 1)[:H, :W]
    if W >= 2 * BLOCK:
        a[:, W // 2:] = blocks[:, W // 2:]
    elif H >= 2 * BLOCK:
        a[H // 2:] = blocks[H // 2:]
    a.setflags(write=False)
    return a


def all_bytes_image(H, W, seed=0):
    """`image` with every byte value 0 .. 255 present in every channel (needs H * W >= 256)."""
    a = image(H, W, seed).copy()
    assert H * W >= 256
    rng = np.random.default_rng(seed + 5)
    for c in range(3):
        a.reshape(-1, 3)[rng.permutation(H * W)[:256], c] = np.arange(256, dtype=np.uint8)
    assert all(len(np.unique(a[..., c])) == 256 for c in range(3))
    return a


@functools.lru_cache(maxsize=None)
def pillow(H, W, oh, ow, resample, seed=0):
    """`Image.resize` of `image(H, W, seed)`: the reference of both test files."""
    from PIL import Image
    r = np.array(Image.fromarray(image(H, W, seed)).resize((ow, oh), pil_filter(resample)))
    r.setflags(write=False)
    return r
