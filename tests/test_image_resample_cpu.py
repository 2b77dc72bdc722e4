"""Pillow's 8-bit resize, without a GPU: the numpy restatement of the algorithm (`resample.resize_reference`, from the tables the device
uses) against `Image.resize` on every pixel, the int32 accumulator bound of every table, the binding table of include/blobctrl_resample.h,
and what the entry points and the Python layer refuse before anything reaches the device."""
import os

import numpy as np
import pytest
import torch

from blobctrl_amd import _lib, resample
from tests import image_resample_common as rc

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("bc_resample_horizontal", "bc_resample_vertical")


@pytest.mark.parametrize("resample_name", rc.FILTERS)
def test_the_reference_is_pillow_on_every_pixel(resample_name):
    for H, W, oh, ow in rc.CASES:
        got = resample.resize_reference(rc.image(H, W), (oh, ow), resample_name)
        want = rc.pillow(H, W, oh, ow, resample_name)
        assert got.dtype == np.uint8 and got.shape == want.shape == (oh, ow, 3) and got.flags.c_contiguous
        assert np.array_equal(got, want), (H, W, oh, ow, resample_name, int((got != want).sum()))
    same = rc.image(64, 64)
    assert resample.resize_reference(same, (64, 64), resample_name) is not same         # both passes skipped: a copy


def test_the_images_overshoot_and_clamp_at_both_ends():
    for H, W, oh, ow in rc.UPSCALING:
        assert oh > H and ow > W and (H, W, oh, ow) in rc.CASES
        for name in rc.FILTERS:
            out = rc.pillow(H, W, oh, ow, name)
            assert out.min() == 0 and out.max() == 255, (H, W, name)
        # ... and for the two filters with negative lobes the clamp really fires: the unclamped value of some output leaves [0, 255]
        for name in ("bicubic", "lanczos"):
            bx, cx, _ = resample.resample_tables(W, ow, name)
            row = rc.image(H, W).astype(np.int64)
            acc = np.stack([(row[:, lo:lo + n] * cx[i, :n, None]).sum(1) for i, (lo, n) in enumerate(bx.tolist())], 1) + (1 << 21)
            assert (acc >> 22).min() < 0 and (acc >> 22).max() > 255, (H, W, name)


def test_tables_follow_pillow_and_keep_the_accumulator_in_int32():
    worst = 0
    sides = sorted({(i, o) for H, W, oh, ow in rc.CASES for i, o in ((H, oh), (W, ow))} | {(512, 256), (1024, 512), (768, 512), (2048, 1024),
                                                                                           (1365, 683), (16384, 1), (1, 4096), (4096, 4095)})
    for i, o in sides:
        for name in rc.FILTERS:
            bounds, coeffs, ksize = resample.resample_tables(i, o, name)
            assert bounds.dtype == coeffs.dtype == np.int32 and bounds.shape == (o, 2) and coeffs.shape == (o, ksize)
            support = resample.FILTER_SUPPORT[name] * max(i / o, 1.0)
            assert ksize == int(np.ceil(support)) * 2 + 1
            assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= ksize).all() and (bounds.sum(1) <= i).all()
            assert all((coeffs[r, n:] == 0).all() for r, n in enumerate(bounds[:, 1].tolist()))
            assert abs(int(coeffs.astype(np.int64).sum(1).max()) - (1 << 22)) <= ksize      # the weights of a row sum to 1.0, each rounded
            worst = max(worst, resample.accumulator_bound(coeffs))
            assert resample.accumulator_bound(coeffs) < 2 ** 31, (i, o, name)
    assert 2 ** 30 < worst < 2 ** 31                                                        # (lanczos: about 1.7e9)
    b, c, k = resample.identity_tables(5)
    assert k == 1 and b.tolist() == [[j, 1] for j in range(5)] and (c == 1 << 22).all()
    px = np.arange(256, dtype=np.uint8).reshape(1, 256)
    assert np.array_equal(resample.apply_tables(px, *resample.identity_tables(1)[:2]), px)
    with pytest.raises(ValueError, match="resample must be"):
        resample.resample_tables(4, 5, "nearest")
    with pytest.raises(ValueError, match="outside 1"):
        resample.resample_tables(0, 5, "bicubic")


def test_a_tap_outside_the_input_contributes_nothing():
    """What the kernels do with a table the Python layer never builds (they cannot inspect device memory), stated on the CPU restatement."""
    a = rc.image(5, 7)
    bounds = np.array([[-2, 4], [3, 9], [7, 2]], dtype=np.int32)                            # rows -2 .. 1, 3 .. 11, 7 .. 8 of 5
    coeffs = np.full((3, 9), (1 << 22) // 2, dtype=np.int32)
    got = resample.apply_tables(a, bounds, coeffs)
    half = lambda rows: np.clip(((1 << 21) + (1 << 21) * a[rows].astype(np.int64).sum(0)) >> 22, 0, 255)
    assert np.array_equal(got[0], half([0, 1])) and np.array_equal(got[1], half([3, 4])) and (got[2] == 0).all()


def test_binding_table_of_the_resample_entry_points():
    lib = _lib.load()
    header = open(os.path.join(HERE, "..", "include", "blobctrl_resample.h")).read()
    assert set(_lib.RESAMPLE_SIGNATURES) == set(NAMES)
    entry = open(os.path.join(HERE, "..", "__graft_entry__.py")).read()
    assert '"blobctrl_resample.h"' in entry and '"image_resample.hip"' in entry
    kinds = {"const unsigned char*": _lib.C.c_void_p, "unsigned char*": _lib.C.c_void_p, "const int*": _lib.C.c_void_p, "float*": _lib.C.c_void_p,
             "const float*": _lib.C.c_void_p, "bc_stream": _lib.C.c_void_p, "int": _lib.C.c_int}
    for name in NAMES:
        assert getattr(lib, name) is not None and f"int {name}(" in header
        res, args = _lib.RESAMPLE_SIGNATURES[name]
        assert getattr(lib, name).argtypes == args and res is _lib.C.c_int
        proto = header.split(f"int {name}(")[1].split(");")[0]                              # the header's prototype, argument by argument
        assert [kinds[" ".join(a.split()[:-1])] for a in proto.replace("\n", " ").split(",")] == args
        for table in (_lib.OPS, _lib.REQUEST_OPS, _lib.SAM_OPS, _lib.SAM_BATCH_OPS, _lib.EXPORTED_SYMBOLS, _lib.VAE_SIGNATURES,
                      _lib.REQUEST_SIGNATURES, _lib.SAM_SIGNATURES, _lib.SAM_BATCH_SIGNATURES, _lib.SAM_HOST_SIGNATURES, _lib.MASK_SIGNATURES,
                      _lib.EDIT_SIGNATURES):
            assert name not in table
        with pytest.raises(KeyError):
            _lib.op_code(name)
    assert len(header.split("\nint bc_")) - 1 == len(NAMES)                                 # ... and the header declares nothing else


def refused(fn, args, word):
    lib = _lib.load()
    assert fn(*args, None) == 1, args
    msg = lib.bc_last_error()
    assert word in msg, (args, msg)
    return msg


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Dummy addresses: every call below must return before a kernel could touch them."""
    lib = _lib.load()
    p, big = 4096, _lib.EDIT_MAX_DIM + 1

    def put(good, at, v):
        return good[:at] + [v] + good[at + 1:]

    # src n H W r0 rows bounds coeffs ksize ow x0 cw tmp
    hz, h_good, hw = lib.bc_resample_horizontal, [p, 2, 8, 9, 1, 6, p, p, 5, 12, 2, 7, p], b"bc_resample_horizontal"
    # in n IH IW r0 xin0 bounds coeffs ksize oh y0 ch cw out_u8 out_f32 lut PH PW
    vt, vw = lib.bc_resample_vertical, b"bc_resample_vertical"
    v_u8, v_f32 = [p, 2, 8, 9, 1, 2, p, p, 5, 12, 3, 6, 7, p, None, None, 0, 0], [p, 2, 8, 9, 1, 2, p, p, 5, 12, 3, 6, 7, None, p, p, 16, 16]
    for at in (0, 6, 7, 12):
        assert b"null pointer" in refused(hz, put(h_good, at, None), hw)
    for good in (v_u8, v_f32):
        for at in (0, 6, 7):
            assert b"null pointer" in refused(vt, put(good, at, None), vw)
    assert b"null pointer" in refused(vt, put(v_u8, 13, None), vw)                          # no output at all
    assert b"null pointer" in refused(vt, put(v_f32, 15, None), vw)                         # fp32 output without its table
    assert b"one epilogue" in refused(vt, put(v_f32, 13, p), vw)
    assert b"lut goes with out_f32" in refused(vt, put(v_u8, 15, p), vw)
    for bad in (0, -1):
        for at in (1, 2, 3, 9):                                                             # n, H, W, ow / n, IH, IW, oh
            assert b"<= 0" in refused(hz, put(h_good, at, bad), hw)
            for good in (v_u8, v_f32):
                assert b"<= 0" in refused(vt, put(good, at, bad), vw)
        assert b"ksize = " in refused(hz, put(h_good, 8, bad), hw)
        assert b"ksize = " in refused(vt, put(v_u8, 8, bad), vw)
        assert b"rows [" in refused(hz, put(h_good, 5, bad), hw)
        assert b"window columns" in refused(hz, put(h_good, 11, bad), hw)
        assert b"window rows" in refused(vt, put(v_u8, 11, bad), vw)
        assert b"window columns" in refused(vt, put(v_f32, 12, bad), vw)
    assert b"ksize = " in refused(hz, put(h_good, 8, 6 * _lib.EDIT_MAX_DIM + 2), hw)
    for at in (2, 3, 9):                                                                    # oversize sides
        assert b"limit" in refused(hz, put(h_good, at, big), hw)
        assert b"limit" in refused(vt, put(v_f32, at, big), vw)
    # the window inside the resized frame, the rows inside the source
    assert b"rows [" in refused(hz, put(h_good, 4, -1), hw) and b"rows [" in refused(hz, put(h_good, 4, 3), hw)        # 3 + 6 > 8
    assert b"window columns" in refused(hz, put(h_good, 10, -1), hw) and b"window columns" in refused(hz, put(h_good, 10, 6), hw)   # 6 + 7 > 12
    assert b"r0 = " in refused(vt, put(v_u8, 4, -1), vw)
    assert b"window rows" in refused(vt, put(v_u8, 10, -1), vw) and b"window rows" in refused(vt, put(v_u8, 10, 7), vw)   # 7 + 6 > 12
    assert b"window columns" in refused(vt, put(v_u8, 5, -1), vw) and b"window columns" in refused(vt, put(v_u8, 5, 3), vw)   # 3 + 7 > 9
    for at, v in ((16, 5), (17, 6), (16, big), (17, big)):                                  # the padded frame must hold the window
        assert b"must hold the window" in refused(vt, put(v_f32, at, v), vw)
    # alignment of the int32 and float tables
    for at in (6, 7):
        assert b"aligned" in refused(hz, put(h_good, at, p + 2), hw) and b"aligned" in refused(vt, put(v_u8, at, p + 1), vw)
    for at in (14, 15):
        assert b"aligned" in refused(vt, put(v_f32, at, p + 2), vw)
    # counts that would not fit the grid
    assert b"grid" in refused(hz, [p, 1 << 20, 4096, 4096, 0, 4096, p, p, 5, 4096, 0, 4096, p], hw)
    assert b"grid" in refused(vt, [p, 1 << 20, 4096, 4096, 0, 0, p, p, 5, 4096, 0, 4096, 4096, p, None, None, 0, 0], vw)
    assert b"grid" in refused(vt, [p, 1 << 20, 8, 8, 0, 0, p, p, 5, 8, 0, 8, 8, None, p, p, 4096, 4096], vw)


def test_the_python_surface_refuses_without_a_gpu():
    from blobctrl_amd.image_processor import Dinov2ImageProcessor
    img = torch.zeros(6, 7, 3, dtype=torch.uint8)
    for call in (lambda: resample.resize_images(img, (3, 4)),
                 lambda: resample.resize_images(img[None], (3, 4), "bicubic", window=(0, 0, 1, 1)),
                 lambda: resample.dinov2_pixel_values(img, Dinov2ImageProcessor()),
                 lambda: resample.sam_input(img, 16),
                 lambda: resample.sam_input(img, 16, "BGR"),
                 lambda: resample.sam_pixel_values(img, 16)):
        with pytest.raises(_lib.BlobCtrlHipError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        resample.resize_images(np.zeros((6, 7, 3), np.uint8), (3, 4))


def test_geometry_and_lookup_tables_are_the_host_processors():
    from blobctrl_amd.image_processor import Dinov2ImageProcessor
    from blobctrl_amd.sam import preprocess_image
    assert resample.dinov2_geometry(300, 260, 256, 224) == ((295, 256), (35, 16, 224, 224))
    assert resample.dinov2_geometry(40, 56, 32, 28) == ((32, 44), (2, 8, 28, 28))
    with pytest.raises(ValueError, match="does not fit"):
        resample.dinov2_geometry(40, 56, 16, 28)
    # every byte value of every channel through the processors themselves, one pixel wide: no resize, no crop - the normalisation alone
    col = np.repeat(np.arange(256, dtype=np.uint8).reshape(256, 1, 1), 3, axis=2)
    proc = Dinov2ImageProcessor(shortest_edge=1, crop_size=1)
    want = np.stack([proc.preprocess(np.ascontiguousarray(col[v:v + 1]))["pixel_values"].numpy()[0, :, 0, 0] for v in range(256)], 1)
    lut = resample.dinov2_lut(proc)
    assert lut.dtype == np.float32 and lut.shape == (3, 256) and np.array_equal(lut, want)
    _, x = preprocess_image(np.ascontiguousarray(col.transpose(1, 0, 2)), 256)               # [1][256][3]: long side 256 already
    assert torch.equal(resample.sam_lut(), x[0, :, 0, :])
    # the rows the horizontal pass must produce are those the vertical tables name, and no more
    for H, oh, name, y0, ch in ((257, 32, "lanczos", 5, 9), (37, 80, "bicubic", 0, 80), (300, 1, "bilinear", 0, 1)):
        b = resample.resample_tables(H, oh, name)[0][y0:y0 + ch]
        r0, rows = resample.source_rows(H, oh, name, y0, ch)
        assert r0 == b[:, 0].min() and r0 + rows == (b[:, 0] + b[:, 1]).max() and 0 <= r0 and r0 + rows <= H
    assert resample.source_rows(40, 40, "bicubic", 3, 4) == (3, 4)
    assert resample.temp_shape(64, 48, (33, 29), "bicubic") == (64, 29, 3) and resample.temp_shape(40, 40, (40, 17), "bicubic") is None


def test_the_pipeline_keeps_the_host_route_for_pixels_that_are_not_on_the_device():
    """`encode_image_dinov2` on a stand-in pipeline: a uint8 tensor in host memory goes through the processor, as it always did."""
    from types import SimpleNamespace
    from blobctrl_amd.image_processor import Dinov2ImageProcessor
    from blobctrl_amd.pipeline import StableDiffusionBlobNetPipeline
    proc, seen = Dinov2ImageProcessor(shortest_edge=32, crop_size=28), {}

    def dinov2(pixel_values):
        seen["px"] = pixel_values
        return SimpleNamespace(pooler_output=torch.zeros(1, 4))

    me = SimpleNamespace(dinov2=dinov2, dinov2_processor=proc, device="cpu")
    img = rc.image(40, 56)
    out = StableDiffusionBlobNetPipeline.encode_image_dinov2(me, torch.from_numpy(img.copy()))
    assert out.shape == (1, 1, 4) and torch.equal(seen["px"], proc.preprocess(img)["pixel_values"])


def test_set_image_still_takes_ndarrays(monkeypatch):
    """The host route of `SamPredictor.set_image` is what it was: an ndarray goes through `preprocess_image`, never through `resample`."""
    from blobctrl_amd import sam

    class Model:
        image_size = 32

        def encode(self, x):
            self.x = x
            return "features"

    def no_device_route(*a, **k):
        raise AssertionError("an ndarray must not take the device route")

    monkeypatch.setattr(resample, "sam_pixel_values", no_device_route)
    image = rc.image(20, 24)
    pred = sam.SamPredictor(Model())
    pred.set_image(image, "BGR")
    resized, x = sam.preprocess_image(image, 32, "BGR")
    assert pred.original_size == (20, 24) and pred.input_size == resized.shape[:2] == (27, 32) and pred.is_image_set
    assert pred.features == "features" and torch.equal(pred.model.x, x)
    with pytest.raises(ValueError, match="uint8 image"):
        pred.set_image(image.astype(np.float32))
