"""VAE tiling / slicing on the HIP path: the blend kernel alone against a torch restatement of the two ramps, tiled decode / encode
against the reference-generated fixture (tests/golden/vae_tiled.npz: a plain result misses it by half the tensor scale), slicing, tiled
decode at the SD-1.5 widths against the CPU oracle under the same tile loop, and the switches through the pipeline.
Bars: the kernel alone max-abs <= 1e-6 of max|input| (a few fp32 roundings; an indexing error is O(1)), its fp16 result within one fp16
ulp of the rounded expectation; everything through the VAE: the project's VAE bar (max-abs <= 1e-2 of scale, PSNR >= 40 dB)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from blobctrl_amd import synth  # noqa: E402
from tests.common import g  # noqa: E402
from tests.vae_tiling_common import (TILE_LATENT, TILE_SAMPLE, TILED_CASES, blend_grid, load_tiled, tiled_apply, vae_close,  # noqa: E402
                                     vae_differs, vae_error)


@pytest.fixture(scope="module")
def tiny_vae():
    from blobctrl_amd.vae import AutoencoderKL
    sd = synth.synth_state_dict(synth.vae_param_shapes((32, 32, 64, 64), 2, 4), 21)
    vae = AutoencoderKL(sd, norm_num_groups=8, sample_size=32)
    vae.tile_sample_min_size, vae.tile_latent_min_size = TILE_SAMPLE, TILE_LATENT
    return vae


@pytest.fixture(scope="module")
def tiled(golden_dir):
    return load_tiled(golden_dir)


def _set(vae, tiling, f=0.25, slicing=False):
    vae.enable_tiling(tiling)
    vae.tile_overlap_factor = f
    vae.use_slicing = slicing


# ------------------------------------------------------------------------------------------------------------ the kernel alone
def _run_blend(mode, heights, widths, extent, limit, B, seed):
    """Random, distinct tiles of a len(heights) x len(widths) grid through bc_vae_tile_blend in row-major order; returns
    (tiles as NCHW fp32 on the CPU, the stitched result as NCHW fp32, the keep-buffers as NCHW fp32, max|input|)."""
    from blobctrl_amd import _lib
    lib = _lib.load()
    Cc = 3 if mode == _lib.VAE_TILE_DECODE else 8
    tiles, k = [], 0
    for h in heights:
        row = []
        for w in widths:
            t = g(seed + k, B, Cc, h, w) * 3 + k                     # (distinct: a tile read in place of another is an O(1) error)
            row.append(t.half().float() if mode == _lib.VAE_TILE_ENCODE else t)
            k += 1
        tiles.append(row)
    H, W = sum(min(h, limit) for h in heights), sum(min(w, limit) for w in widths)
    out = torch.full((B, Cc, H, W) if mode == _lib.VAE_TILE_DECODE else (B, H * W, Cc), float("nan"),
                     dtype=torch.float32 if mode == _lib.VAE_TILE_DECODE else torch.float16, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keeps, oy = {}, 0
    for i, h in enumerate(heights):
        ox = 0
        for j, w in enumerate(widths):
            src = tiles[i][j].permute(0, 2, 3, 1).contiguous().to("cuda", torch.float32 if mode == _lib.VAE_TILE_DECODE else torch.float16)
            above, left = keeps.get((i - 1, j)), keeps.get((i, j - 1))
            keep = torch.full((B, h, w, Cc), float("nan"), dtype=torch.float32, device="cuda")
            ev = min(heights[i - 1], h, extent) if i else 0
            eh = min(widths[j - 1], w, extent) if j else 0
            rc = lib.bc_vae_tile_blend(src.data_ptr(), above.data_ptr() if i else None, left.data_ptr() if j else None, keep.data_ptr(),
                                       out.data_ptr(), mode, B, h, w, heights[i - 1] if i else 0, widths[j - 1] if j else 0, ev, eh, oy, ox,
                                       min(h, limit), min(w, limit), H, W, s)
            assert rc == 0, lib.bc_last_error()
            keeps[(i, j)] = keep
            ox += min(w, limit)
        oy += min(h, limit)
    torch.cuda.synchronize()
    res = out.cpu() if mode == _lib.VAE_TILE_DECODE else out.cpu().view(B, H, W, Cc).permute(0, 3, 1, 2)
    scale = max(t.abs().max().item() for row in tiles for t in row)
    return tiles, res, {k_: v.cpu().permute(0, 3, 1, 2) for k_, v in keeps.items()}, scale


# (heights, widths, extent, limit): a 3 x 2 grid on the 16-byte paths; the same with ragged edge tiles (a 7-wide column: the scalar
# path; a crop that ends inside a 4-pixel run); extents above the last row and column (the clamp); one row; one column
BLEND_GRIDS = {"aligned": ((12, 12, 8), (16, 12), 4, 8), "ragged": ((12, 12, 5), (16, 7), 3, 9), "clamp": ((12, 6, 2), (8, 2), 4, 6),
               "row": ((6,), (8, 8, 4), 2, 6), "column": ((8, 8, 3), (5,), 3, 5)}


@pytest.mark.parametrize("name", list(BLEND_GRIDS))
@pytest.mark.parametrize("mode", [0, 1], ids=["decode_nchw_f32", "encode_nhwc_f16"])
def test_blend_kernel_against_the_two_ramps(name, mode):
    heights, widths, extent, limit = BLEND_GRIDS[name]
    tiles, res, keeps, scale = _run_blend(mode, heights, widths, extent, limit, B=2, seed=900)
    want, blended = blend_grid(tiles, extent, limit)
    assert res.shape == want.shape
    for (i, j), k in keeps.items():                                   # the fp32 path: what later neighbours read
        err = (k - blended[i][j]).abs().max().item()
        print(f"{name} mode {mode} tile ({i}, {j}): keep max-abs {err:.3e} (scale {scale:.2f})")
        assert err <= 1e-6 * scale, (name, i, j, err)
    if mode == 0:
        err = (res - want).abs().max().item()
        print(f"{name}: result max-abs {err:.3e}")
        assert err <= 1e-6 * scale
    else:
        w16 = want.half()
        ulp = torch.maximum(torch.floor(torch.log2(w16.float().abs().clamp(min=2.0 ** -14))), torch.tensor(-14.0))
        ulp = torch.pow(2.0, ulp - 10)
        err = (res.float() - w16.float()).abs()
        print(f"{name}: fp16 result worst error {float((err / ulp).max()):.2f} ulp")
        assert not torch.isnan(res).any() and bool((err <= ulp).all())
    if name == "clamp":
        assert min(heights[1], heights[2], extent) == 2 < extent and min(widths) == 2 < extent


# ------------------------------------------------------------------------------------------------------------ the reference fixture
@pytest.mark.parametrize("tag", TILED_CASES)
def test_tiled_decode_and_encode_match_the_reference_fixture(tiny_vae, tiled, tag):
    z, meta = tiled
    m = meta[tag]
    lat, img = torch.from_numpy(z[f"{tag}_z"]).cuda(), torch.from_numpy(z[f"{tag}_img"]).cuda()
    _set(tiny_vae, True, m["f"])
    try:
        dec = tiny_vae.decode(lat, return_dict=False)[0]
        dist = tiny_vae.encode(img).latent_dist
        mom = dist.parameters
        assert list(dec.shape) == m["decoded_shape"] and dec.dtype == torch.float32 and list(mom.shape) == m["moments_shape"]
        print(f"{tag}: tiled decode (max-abs/scale, PSNR) {vae_error(dec.cpu().numpy(), z[f'{tag}_decoded'])}, "
              f"moments {vae_error(mom.cpu().numpy(), z[f'{tag}_moments'])}")
        vae_close(dec.cpu().numpy(), z[f"{tag}_decoded"])
        vae_close(mom.cpu().numpy(), z[f"{tag}_moments"])
        vae_close(dist.mode().cpu().numpy(), z[f"{tag}_moments"][:, :4])
        assert torch.equal(tiny_vae.decode(lat)[0], dec)                 # cached plans, same bits
        # the blended moments feed the same posterior sample
        noise = torch.randn(mom[:, :4].shape, generator=torch.Generator().manual_seed(5))
        ref = torch.from_numpy(z[f"{tag}_moments"])
        want = ref[:, :4] + torch.exp(0.5 * ref[:, 4:].clamp(-30, 20)) * noise
        vae_close(dist.sample(torch.Generator().manual_seed(5)).cpu().numpy(), want.numpy())
        # the same calls with tiling disabled miss the bar: the test can see the difference
        _set(tiny_vae, False)
        plain = tiny_vae.decode(lat)[0].cpu().numpy()
        plain_mom = tiny_vae.encode(img).latent_dist.parameters.cpu().numpy()
        print(f"{tag}: plain decode vs tiled fixture {vae_error(plain, z[f'{tag}_decoded'])}, moments {vae_error(plain_mom, z[f'{tag}_moments'])}")
        assert vae_differs(plain, z[f"{tag}_decoded"]) and vae_differs(plain_mom, z[f"{tag}_moments"])
    finally:
        _set(tiny_vae, False)


def test_tiling_enabled_but_not_triggered_is_bit_identical(tiny_vae, tiled):
    z, meta = tiled
    lat, img = torch.from_numpy(z["D_z"]).cuda(), torch.from_numpy(z["D_img"]).cuda()
    try:
        _set(tiny_vae, False)
        dec0, mom0 = tiny_vae.decode(lat)[0], tiny_vae.encode(img).latent_dist.parameters
        _set(tiny_vae, True)
        dec1, mom1 = tiny_vae.decode(lat)[0], tiny_vae.encode(img).latent_dist.parameters
        assert torch.equal(dec0, dec1) and torch.equal(mom0, mom1)
        vae_close(dec1.cpu().numpy(), z["D_decoded"])
        vae_close(mom1.cpu().numpy(), z["D_moments"])
    finally:
        _set(tiny_vae, False)


# ------------------------------------------------------------------------------------------------------------ slicing
def test_sliced_decode_and_encode(tiny_vae, tiled, golden_dir):
    import os
    v = np.load(os.path.join(golden_dir, "vae_tiny.npz"))
    z, meta = tiled
    try:
        _set(tiny_vae, False, slicing=True)
        dec = tiny_vae.decode(torch.from_numpy(v["z"]).cuda())[0]
        dist = tiny_vae.encode(torch.from_numpy(v["img"]).cuda()).latent_dist
        assert v["z"].shape[0] == 2 and dec.shape == v["decoded"].shape
        assert ("dec", 1, 4, 6) in tiny_vae._plans and ("enc", 1, 32, 48) in tiny_vae._plans         # one sample at a time
        vae_close(dec.cpu().numpy(), v["decoded"])
        vae_close(dist.parameters.cpu().numpy(), v["moments"])
        vae_close(dist.sample(torch.Generator().manual_seed(5)).cpu().numpy(), v["sample"])
        assert not torch.equal(dec[0], dec[1])                                                       # (the second sample is its own)
        # slicing with tiling on case A: tiling alone, within the bar (and the fixture's)
        lat, img = torch.from_numpy(z["A_z"]).cuda(), torch.from_numpy(z["A_img"]).cuda()
        _set(tiny_vae, True, meta["A"]["f"], slicing=False)
        dec_t, mom_t = tiny_vae.decode(lat)[0].cpu().numpy(), tiny_vae.encode(img).latent_dist.parameters.cpu().numpy()
        _set(tiny_vae, True, meta["A"]["f"], slicing=True)
        dec_st, mom_st = tiny_vae.decode(lat)[0].cpu().numpy(), tiny_vae.encode(img).latent_dist.parameters.cpu().numpy()
        vae_close(dec_st, dec_t)
        vae_close(mom_st, mom_t)
        vae_close(dec_st, z["A_decoded"])
        vae_close(mom_st, z["A_moments"])
    finally:
        _set(tiny_vae, False)


# ------------------------------------------------------------------------------------------------------------ SD-1.5 widths
def test_full_width_tiled_decode_vs_oracle_under_the_same_tile_loop():
    """The SD-1.5 VAE schema with 256 / 32 tiles on a 40 x 32 latent: tiles (32, 32), (32, 8), (16, 32), (16, 8), each decoded by the
    CPU oracle and blended by the restatement (less oracle work than the full-size test's 64 x 64 decode)."""
    import os
    from blobctrl_amd.vae import AutoencoderKL
    from oracle import vae as o_vae
    torch.set_num_threads(min(32, len(os.sched_getaffinity(0))))
    sd = synth.synth_state_dict(synth.vae_param_shapes(), 33)
    vae = AutoencoderKL(sd)
    vae.tile_sample_min_size, vae.tile_latent_min_size = 256, 32
    vae.enable_tiling()
    zl = g(63, 1, 4, 40, 32)
    shapes = []

    def dec(t):
        shapes.append(tuple(t.shape[2:]))
        return o_vae.decode(sd, t)
    ref = tiled_apply(dec, zl, 32, int(32 * (1 - 0.25)), int(256 * 0.25), 256 - int(256 * 0.25)).numpy()
    assert shapes == [(32, 32), (32, 8), (16, 32), (16, 8)] and ref.shape == (1, 3, 320, 256)
    img = vae.decode(zl.cuda())[0].cpu().numpy()
    assert img.shape == ref.shape
    print(f"full-width tiled decode (max-abs/scale, PSNR): {vae_error(img, ref)}")
    vae_close(img, ref)


# ------------------------------------------------------------------------------------------------------------ pipeline
def test_pipeline_picks_up_the_switches(tiny_vae):
    """fg_image / bg_image in, output_type="pt" out at 128 x 96 with tiling on == encode_latents -> latent call -> decode_latents composed
    by hand, bit for bit; with tiling off the image is another one."""
    from tests.common import TINY, tiny_weights
    from tests.gpu_common import make_pipeline
    usd, bsd = tiny_weights()
    pipe = make_pipeline(usd, bsd, scheduler="ddim")
    pipe.vae = tiny_vae
    _set(tiny_vae, False)
    fg, bg = g(71, 1, 3, 128, 96).clamp(-1, 1), g(72, 1, 3, 128, 96).clamp(-1, 1)
    prompt, score = g(73, 2, 5, TINY["ctx"]), g(74, 1, 2, 16, 12).abs().clamp(max=1)
    dino, lat0 = g(75, 1, 1, TINY["feat"]), g(76, 1, 4, 16, 12)
    try:
        pipe.enable_vae_tiling()
        assert tiny_vae.use_tiling
        torch.manual_seed(11)
        img = pipe(prompt, None, None, score, dino, num_inference_steps=2, latents=lat0, fg_image=fg, bg_image=bg, output_type="pt")
        assert img.shape == (1, 3, 128, 96)
        assert ("dec", 1, 8, 8) in tiny_vae._plans and ("dec", 1, 4, 6) in tiny_vae._plans and ("enc", 1, 32, 48) in tiny_vae._plans
        torch.manual_seed(11)
        fl, bl = pipe.encode_latents(fg), pipe.encode_latents(bg)
        lat = pipe(prompt, fl, bl, score, dino, num_inference_steps=2, latents=lat0)
        assert torch.equal(pipe.decode_latents(lat, "pt"), img)
        pipe.disable_vae_tiling()
        assert not tiny_vae.use_tiling
        torch.manual_seed(11)
        plain = pipe(prompt, None, None, score, dino, num_inference_steps=2, latents=lat0, fg_image=fg, bg_image=bg, output_type="pt")
        assert plain.shape == img.shape and not torch.equal(plain, img)
        assert vae_differs(plain.cpu().numpy(), img.cpu().numpy())
    finally:
        _set(tiny_vae, False)
