"""Helpers of the tiled-VAE tests: a torch restatement of the two blend ramps and of the tile loop (what `enable_tiling()` means in the
reference: D/models/autoencoders/autoencoder_kl.py:328-442), the VAE bar of tests/test_vae_gpu.py, and the fixture loader.  Nothing
here touches the GPU or the package under test."""
import json
import os

import numpy as np
import torch

from tests.common import psnr

TILE_SAMPLE, TILE_LATENT = 64, 8                       # the tile sizes of tests/golden/vae_tiled.npz
TILED_CASES = ("A", "B", "C", "Cp")


def load_tiled(golden_dir):
    z = np.load(os.path.join(golden_dir, "vae_tiled.npz"))
    return z, json.loads(str(z["meta"]))


def vae_error(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6)), float(psnr(a, b))


def vae_close(a, b, tol=1e-2, db=40.0):
    """The project's VAE bar (`_close` of tests/test_vae_gpu.py): max-abs <= 1e-2 of the reference's scale and PSNR >= 40 dB."""
    err, p = vae_error(a, b)
    assert err < tol and p > db, f"max-abs/scale {err:.3e}, PSNR {p:.1f} dB"
    return err


def vae_differs(a, b, tol=1e-2, db=40.0):
    """True when `a` MISSES the VAE bar against `b` (what a plain result must do against a tiled fixture)."""
    err, p = vae_error(a, b)
    return not (err < tol and p > db)


def _ramp(n):
    """fp32 weights of an n-wide ramp: (1 - i / n, i / n) formed as Python floats (doubles) and rounded once."""
    own = torch.tensor([i / n for i in range(n)], dtype=torch.float64)
    return (1 - own).to(torch.float32), own.to(torch.float32)


def blend_grid(tiles, extent, limit):
    """tiles[i][j]: fp32 [B, C, h_i, w_j].  Blends every tile with the tile above, then with the tile to its left, in row-major order
    and in place (so a neighbour is already blended when it is read), extents clamped to min(neighbour, own, extent); returns
    (the `[:limit, :limit]` crops concatenated, the blended tiles)."""
    tiles = [[t.clone() for t in row] for row in tiles]
    out_rows = []
    for i, row in enumerate(tiles):
        for j, t in enumerate(row):
            if i > 0:
                a = tiles[i - 1][j]
                e = min(a.shape[2], t.shape[2], extent)
                if e:
                    wa, wt = (w.view(1, 1, e, 1) for w in _ramp(e))
                    t[:, :, :e, :] = a[:, :, a.shape[2] - e:, :] * wa + t[:, :, :e, :] * wt
            if j > 0:
                a = row[j - 1]
                e = min(a.shape[3], t.shape[3], extent)
                if e:
                    wa, wt = (w.view(1, 1, 1, e) for w in _ramp(e))
                    t[:, :, :, :e] = a[:, :, :, a.shape[3] - e:] * wa + t[:, :, :, :e] * wt
        out_rows.append(torch.cat([t[:, :, :limit, :limit] for t in row], dim=3))
    return torch.cat(out_rows, dim=2), tiles


def tiled_apply(fn, x, tile_in, step, extent, limit):
    """`fn` on every `tile_in`-sized tile of x [B, C, H, W] cut every `step` (clipped at the border), blended by `blend_grid`."""
    H, W = x.shape[2:]
    tiles = [[fn(x[:, :, i:i + tile_in, j:j + tile_in]) for j in range(0, W, step)] for i in range(0, H, step)]
    return blend_grid(tiles, extent, limit)[0]
