"""VAE tiling / slicing, host side: the tile geometry against what the reference recorded (tests/golden/vae_tiled.npz), the defaults and
switches on the VAE and the pipeline, the refusals that come before any launch, and the ABI placement of the blend kernel (a header and
a signature table of its own: the plan ABI's symbol list and op table are what they were)."""
import numpy as np
import pytest
import torch

from blobctrl_amd import synth
from tests.vae_tiling_common import TILE_LATENT, TILE_SAMPLE, TILED_CASES, load_tiled

TINY_BOC = (32, 32, 64, 64)


@pytest.fixture(scope="module")
def tiny_cpu_vae():
    from blobctrl_amd.vae import AutoencoderKL
    return AutoencoderKL(synth.synth_state_dict(synth.vae_param_shapes(TINY_BOC, 2, 4), 21), norm_num_groups=8, device="cpu", sample_size=32)


# ------------------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("tag", TILED_CASES)
def test_geometry_reproduces_the_tiles_the_reference_cut(golden_dir, tag):
    from blobctrl_amd.vae import tile_geometry
    z, meta = load_tiled(golden_dir)
    m = meta[tag]
    h, w = m["latent"]
    for kind, H, W, key, shape in (("decode", h, w, "decode_tiles", m["decoded_shape"]), ("encode", 8 * h, 8 * w, "encode_tiles", m["moments_shape"])):
        geo = tile_geometry(kind, H, W, TILE_SAMPLE, TILE_LATENT, m["f"], 8)
        got = [[t["in_h"], t["in_w"], t["out_h"], t["out_w"], t["oy"], t["ox"]] for t in geo["tiles"]]
        assert got == z[f"{tag}_{key}"].tolist(), (tag, kind)
        assert [geo["rows"], geo["cols"]] == m["grid"] and [geo["out_h"], geo["out_w"]] == shape[2:]
        assert [(t["i"], t["j"]) for t in geo["tiles"]] == [(i, j) for i in range(geo["rows"]) for j in range(geo["cols"])]     # row-major
        for t in geo["tiles"]:                                              # crops tile the result exactly; extents fit both tiles
            assert t["ch"] == min(t["out_h"], geo["limit"]) and t["cw"] == min(t["out_w"], geo["limit"])
            assert (t["ev"] > 0) == (t["i"] > 0) and (t["eh"] > 0) == (t["j"] > 0)
            assert t["ev"] <= min(t["out_h"], geo["extent"]) and t["eh"] <= min(t["out_w"], geo["extent"])
        cover = np.zeros((geo["out_h"], geo["out_w"]), np.int32)
        for t in geo["tiles"]:
            cover[t["oy"]:t["oy"] + t["ch"], t["ox"]:t["ox"] + t["cw"]] += 1
        assert (cover == 1).all()


def test_geometry_cases_are_the_ones_the_fixture_names(golden_dir):
    from blobctrl_amd.vae import tile_geometry
    z, meta = load_tiled(golden_dir)
    shapes = lambda tag: sorted({(r[0], r[1]) for r in z[f"{tag}_decode_tiles"].tolist()}, reverse=True)
    assert shapes("A") == [(8, 8), (8, 6), (4, 8), (4, 6)] and meta["A"]["grid"] == [3, 2] and meta["A"]["batch"] == 2
    assert [r[0] for r in z["B_decode_tiles"].tolist()[::2]] == [8, 6, 2]                        # the last row: 16 px, below the 32 px extent
    geo = tile_geometry("decode", 10, 8, TILE_SAMPLE, TILE_LATENT, 0.5, 8)
    assert geo["extent"] == 32 and [t["ev"] for t in geo["tiles"][::2]] == [0, 32, 16]           # the clamp
    assert meta["C"]["grid"] == [1, 2] and meta["Cp"]["grid"] == [2, 1]
    # D: enabled, not triggered - one tile would be the whole input, and the dispatch test (h > tile or w > tile) is false
    assert meta["D"]["tiled"] is False and meta["D"]["latent"] == [8, 8] and meta["D"]["decoded_shape"] == [1, 3, 64, 64]
    # the origin is the running sum of the cropped sizes, not index * limit: they part when a caller sets inconsistent sizes
    geo = tile_geometry("decode", 12, 4, 40, TILE_LATENT, 0.25, 8)                               # 64-px tiles, limit 30 < step 48
    assert [(t["oy"], t["ch"]) for t in geo["tiles"]] == [(0, 30), (30, 30)] and geo["out_h"] == 60
    geo = tile_geometry("decode", 14, 4, 96, TILE_LATENT, 0.25, 8)                               # limit 72 > tile 64: the crop is the tile
    assert [(t["oy"], t["ch"]) for t in geo["tiles"]] == [(0, 64), (64, 64), (128, 16)] and geo["out_h"] == 144


def test_zero_step_and_bad_token_counts_raise_before_any_launch(tiny_cpu_vae):
    from blobctrl_amd.vae import tile_geometry
    with pytest.raises(ValueError, match="tile_overlap_factor 1.0"):
        tile_geometry("decode", 16, 12, 64, 8, 1.0, 8)
    vae = tiny_cpu_vae
    vae.tile_sample_min_size, vae.tile_latent_min_size = TILE_SAMPLE, TILE_LATENT
    try:
        vae.tile_overlap_factor = 1.0
        with pytest.raises(ValueError, match="tile_overlap_factor 1.0"):
            vae._tiles("decode", 16, 12)
        vae.tile_overlap_factor = 0.25
        assert len(vae._tiles("decode", 16, 12)["tiles"]) == 6
        with pytest.raises(ValueError, match=r"tile 3x7 at \(6, 0\) has 3x7 = 21 latent tokens.*multiple of 8"):
            vae._tiles("decode", 9, 7)                                      # tiles 8x7 (56 tokens: fine) and 3x7
        with pytest.raises(ValueError, match=r"tile 24x56 at \(48, 0\) has 3x7 = 21 latent tokens"):
            vae._tiles("encode", 72, 56)
        assert not vae._plans                                               # nothing was recorded, let alone launched
    finally:
        vae.tile_sample_min_size, vae.tile_latent_min_size, vae.tile_overlap_factor = 32, 4, 0.25


# ------------------------------------------------------------------------------------------------------------ public surface
def test_defaults_and_switches(tiny_cpu_vae):
    from blobctrl_amd.vae import AutoencoderKL
    zeros = {k: torch.zeros(1).expand(*v) if len(v) else torch.zeros(()) for k, v in synth.vae_param_shapes().items()}
    full = AutoencoderKL(zeros, device="cpu")                               # the SD-1.5 schema
    assert (full.config.sample_size, full.tile_sample_min_size, full.tile_latent_min_size, full.tile_overlap_factor) == (512, 512, 64, 0.25)
    assert full.use_tiling is False and full.use_slicing is False
    vae = tiny_cpu_vae
    assert (vae.config.sample_size, vae.tile_sample_min_size, vae.tile_latent_min_size, vae.tile_overlap_factor) == (32, 32, 4, 0.25)
    vae.enable_tiling()
    assert vae.use_tiling is True
    vae.enable_tiling(False)
    assert vae.use_tiling is False
    vae.enable_tiling(True)
    vae.disable_tiling()
    assert vae.use_tiling is False
    vae.enable_slicing()
    assert vae.use_slicing is True and vae.use_tiling is False
    vae.disable_slicing()
    assert vae.use_slicing is False
    vae.tile_sample_min_size, vae.tile_latent_min_size, vae.tile_overlap_factor = 64, 8, 0.5          # plain, settable attributes
    assert (vae.tile_sample_min_size, vae.tile_latent_min_size, vae.tile_overlap_factor) == (64, 8, 0.5)
    vae.tile_sample_min_size, vae.tile_latent_min_size, vae.tile_overlap_factor = 32, 4, 0.25


def test_pipeline_and_engine_switches_reach_the_vae(tiny_cpu_vae):
    from blobctrl_amd.pipeline import BlobCtrlEngine, StableDiffusionBlobNetPipeline
    vae = tiny_cpu_vae
    for cls in (StableDiffusionBlobNetPipeline, BlobCtrlEngine):
        pipe = cls.__new__(cls)
        pipe.vae = vae
        pipe.enable_vae_tiling()
        assert vae.use_tiling is True and vae.use_slicing is False
        pipe.enable_vae_slicing()
        assert vae.use_slicing is True
        pipe.disable_vae_tiling()
        assert vae.use_tiling is False and vae.use_slicing is True
        pipe.disable_vae_slicing()
        assert vae.use_slicing is False
    eng = BlobCtrlEngine.__new__(BlobCtrlEngine)
    eng.vae = None
    with pytest.raises(ValueError, match="without a VAE"):
        eng.enable_vae_tiling()


# ------------------------------------------------------------------------------------------------------------ ABI placement
def test_blend_entry_point_resolves_outside_the_plan_abi():
    import os
    import re
    from blobctrl_amd import _lib
    from tests.test_freeu_cpu import OLD_OPS, OP_FREEU
    lib = _lib.load()                                                       # (raises when a declared symbol does not resolve)
    assert list(_lib.VAE_SIGNATURES) == ["bc_vae_tile_blend"] and lib.bc_vae_tile_blend.argtypes is not None
    assert len(_lib.VAE_SIGNATURES["bc_vae_tile_blend"][1]) == 20
    assert len(_lib.EXPORTED_SYMBOLS) == 92 and "bc_vae_tile_blend" not in _lib.EXPORTED_SYMBOLS
    assert _lib.OPS == dict(OLD_OPS, bc_freeu=OP_FREEU)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(repo, "include", "blobctrl_vae.h")).read()
    assert re.findall(r"\b(bc_[a-z0-9_]+)\s*\(", header) == ["bc_last_error", "bc_vae_tile_blend"]       # (the first: named in a comment)
    assert "bc_vae" not in open(os.path.join(repo, "include", "blobctrl_hip.h")).read()


def test_blend_argument_checks_refuse_before_launching():
    from blobctrl_amd import _lib
    lib = _lib.load()
    p = 1 << 20                                                             # (non-null, aligned, far apart: the checks fail first)
    base = dict(src=p, above=2 * p, left=3 * p, keep=4 * p, out=5 * p, mode=0, B=1, th=8, tw=8, ha=8, wl=8, ev=4, eh=4, oy=0, ox=0, ch=6,
                cw=6, H=16, W=16)
    cases = [(dict(src=None), b"null pointer"), (dict(keep=None), b"null pointer"), (dict(out=None), b"null pointer"),
             (dict(mode=2), b"mode 2"), (dict(B=0), b"bad shape"), (dict(tw=0), b"bad shape"),
             (dict(ev=9), b"vertical extent 9 larger than a tile"), (dict(ev=5, ha=4), b"vertical extent 5 larger than a tile"),
             (dict(eh=9), b"horizontal extent 9 larger than a tile"), (dict(eh=-1), b"horizontal extent -1"),
             (dict(ch=9), b"crop 9x6"), (dict(oy=11), b"leaves the tile"), (dict(ox=12, cw=6, W=16), b"leaves the tile"),
             (dict(src=p + 8), b"alignment"), (dict(left=3 * p + 4), b"alignment"), (dict(out=5 * p + 2), b"alignment"),
             (dict(keep=p), b"buffers of their own"), (dict(keep=2 * p + 64), b"buffers of their own"),
             (dict(out=3 * p + 128), b"buffers of their own"), (dict(out=4 * p + 256), b"buffers of their own"),
             (dict(mode=1, out=p + 512), b"buffers of their own")]
    for kw, word in cases:
        a = dict(base, **kw)
        assert lib.bc_vae_tile_blend(*a.values(), None) == 1, kw
        assert word in lib.bc_last_error(), (kw, lib.bc_last_error())
