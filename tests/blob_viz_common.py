"""Shared by tests/test_blob_viz_cpu.py and tests/test_blob_viz_gpu.py: the fixture loader and a plain numpy restatement of the
reference lines the blob-visualisation kernels replace (blobctrl/utils/utils.py = `ut:`): alpha compositing ut:179-181, the feature
splat ut:57-77, bilinear resizing as F.interpolate(mode="bilinear", align_corners=False) does it, pyramid_resize ut:280-294."""
import json
import os

import numpy as np


def load_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "blob_viz.npz"))
    return z, json.loads(str(z["meta"]))


def viz_boost(s):
    """The non-identity viz_score_fn of the fixture (tools/make_golden.py::viz_boost): `s * 1.5` (ut:109), clamped at 1."""
    return s.mul(1.5).clamp(max=1)


def composite(raw):
    """ut:179-181: raw [..., K] -> d_i = raw_i * prod_{j>i}(1 - raw_j), d_{K-1} = raw_{K-1}."""
    K = raw.shape[-1]
    d = np.empty_like(raw)
    d[..., K - 1] = raw[..., K - 1]
    p = 1.0 - raw[..., K - 1]
    for i in range(K - 2, -1, -1):
        d[..., i] = p * raw[..., i]
        p = p * (1.0 - raw[..., i])
    return d


def _taps(n_in, n_out):
    src = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = np.clip(src - i0, 0.0, 1.0)
    return i0, i1, 1.0 - w1, w1


def bilinear(img, h2, w2):
    """img [..., H, W] -> [..., h2, w2] in float64: src = (dst + 0.5) * in / out - 0.5 clamped at 0, upper neighbour clamped."""
    img = np.asarray(img, dtype=np.float64)
    y0, y1, wy0, wy1 = _taps(img.shape[-2], h2)
    x0, x1, wx0, wx1 = _taps(img.shape[-1], w2)
    r0 = img[..., y0, :][..., x0] * wx0 + img[..., y0, :][..., x1] * wx1
    r1 = img[..., y1, :][..., x0] * wx0 + img[..., y1, :][..., x1] * wx1
    return r0 * wy0[:, None] + r1 * wy1[:, None]


def from_scores(scores, features, size, channels_last=True):
    """ut:57-77 in float64, with the reference's `size and not (scores.shape[2] == size)` test."""
    s = np.asarray(scores, dtype=np.float64)
    if channels_last:
        shape2 = s.shape[2]
        s = s.transpose(0, 3, 1, 2)
    else:
        shape2 = s.shape[2]
    if size and not (shape2 == size):
        h2, w2 = (size, size) if isinstance(size, int) else size
        s = bilinear(s, h2, w2)
    return np.einsum("nmhw,nmc->nchw", s, np.asarray(features, dtype=np.float64))


def pyramid(img, cutoff):
    """ut:280-294: halve with an int size, so every level below the first is square."""
    out = [np.asarray(img, dtype=np.float64)]
    while out[-1].shape[-1] > cutoff:
        half = out[-1].shape[-1] // 2
        out.append(bilinear(out[-1], half, half))
    return {o.shape[-1]: o for o in out}


def raw_scores(ellipse, W, H, h, w, size=1.0):
    """The raw channels-last scores [1, h, w, 2] = (1, s) of one ellipse (ut:175-176), s from the oracle's rasteriser."""
    from oracle import blob_splat
    s = blob_splat.splat_scores_from_ellipse(ellipse, W, H, h, w, size)[0, 1]
    return np.stack([np.ones_like(s), s], -1)[None]


def blob_kwargs(ellipse, W, H, size=1.0):
    """The reference's blob dictionary (scripts/blobctrl_inference.py:100-109) for `splat_features(**blob, ...)`."""
    import torch
    from blobctrl_amd.splat import blob_dict_from_ellipse
    blob = blob_dict_from_ellipse(ellipse, W, H)
    blob["sizes"] = torch.tensor([[size]])
    return blob
