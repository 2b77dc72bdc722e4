"""Gaussian-blob splat rasteriser on MI355X: drop-in for `blobctrl.utils.utils.splat_features(...)`.

Keeps the reference call signature (blobctrl/utils/utils.py:80-241, `ut:` below) for every call the reference's scripts and app make:
    splat_features(xs, ys, covs, sizes, score_size=(h, w), return_d_score=True) -> Tensor[N, M+1, h, w]  (float64)
        the pipeline's branch (scripts/blobctrl_inference.py:112-117, scripts/blobctrl_app.py:653-658): ONE kernel, bc_splat_scores;
    splat_features(..., viz_size=(H, W), is_viz=True, viz_colors=..., only_vis=True)["feature_img"]
        the app's blob image (scripts/blobctrl_app.py:637-650): bc_splat_maps, bc_alpha_composite, bc_splat_from_scores;
    splat_features(..., score_size=(h, w), interp_size=k, features=...) -> dict
        the dictionary return (ut:226-241): scores_pyramid (bc_resize_bilinear), feature_grid, the layout entries;
with N = M = 1 as hard-coded by the tuple branches (ut:132-133, 157-158), all in fp64 like the reference.  Also public:
`splat_features_from_scores` (ut:57-77, general in N, M, C) and `pyramid_resize` (ut:280-294), and the ellipse -> normalised
Gaussian helpers of scripts/blobctrl_inference.py:23-109.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def ellipse_to_gaussian(ellipse):
    """((xc,yc),(d1,d2),angle_deg) -> (mean[2], cov[2,2]); scripts/blobctrl_inference.py:23-86."""
    (xc, yc), (d1, d2), angle = ellipse
    theta = np.radians((((180 - angle) % 180) + 90) % 180)
    a, b = d1 / 2.0, d2 / 2.0
    cov = np.array([[b ** 2, 0.0], [0.0, a ** 2]])
    R = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    cov = R @ cov @ R.T
    cov[0, 1] *= -1
    cov[1, 0] *= -1
    return np.array([xc, yc], dtype=np.float64), cov


def normalize_gs(mean, cov, width, height):
    """scripts/blobctrl_inference.py:88-98."""
    return mean / np.array([width, height]), cov / (np.sqrt(width ** 2 + height ** 2) ** 2)


def blob_dict_from_ellipse(ellipse, width, height):
    """scripts/blobctrl_inference.py:78-109 chained: returns the kwargs `splat_features(**blob, ...)` expects."""
    mean, cov = ellipse_to_gaussian(ellipse)
    nm = mean / np.array([width, height])
    nc = cov / (np.sqrt(width ** 2 + height ** 2) ** 2)
    return {"xs": torch.tensor(nm[0]).unsqueeze(0), "ys": torch.tensor(nm[1]).unsqueeze(0),
            "covs": torch.tensor(nc).unsqueeze(0).unsqueeze(0), "sizes": torch.tensor([1.0]).unsqueeze(0)}


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.BlobCtrlHipError("splat_features runs on MI355X only; there is no CPU fallback")
    return dev


def _require_gpu(t: torch.Tensor, what: str):
    if t.device.type != "cuda":
        raise _lib.BlobCtrlHipError(f"{what} runs on MI355X only; there is no CPU fallback")


def splat_features(xs, ys, covs, sizes, score_size=None, interp_size=None, features=None, viz_size=None, is_viz=False,
                   ret_layout=True, viz_score_fn=None, return_d_score=False, only_vis=False, only_splatting_fg=False,
                   only_splatting_bg=False, device="cuda:0", **kwargs):
    """HIP replacement of utils.splat_features (ut:80-241) with the reference's branch order.  The grid is `viz_size` when that is a
    tuple (then `score_size` is ignored, ut:120-135), else the tuple `score_size` (ut:145-160); an int `score_size` (ut:137-144) has no
    caller in the reference and is not provided."""
    if isinstance(viz_size, (tuple, list)):
        h, w = int(viz_size[0]), int(viz_size[1])
    elif isinstance(score_size, (tuple, list)):
        h, w = int(score_size[0]), int(score_size[1])
    else:
        raise NotImplementedError("only the tuple-grid branches are provided: score_size=(h, w) or viz_size=(H, W)")
    in_xs, in_ys, in_covs, in_sizes = xs, ys, covs, sizes
    xs = torch.as_tensor(xs, dtype=torch.float64).reshape(-1)
    ys = torch.as_tensor(ys, dtype=torch.float64).reshape(-1)
    covs = torch.as_tensor(covs, dtype=torch.float64).reshape(-1, 2, 2)
    sizes = torch.as_tensor(sizes, dtype=torch.float64).reshape(-1)
    n = xs.numel()
    if not (ys.numel() == n and covs.shape[0] == n and sizes.numel() == n):
        raise ValueError("xs, ys, covs, sizes must describe the same number of blobs")
    if n != 1:
        raise ValueError("the reference branch hard-codes batch = 1, n_gaussians = 1 (utils.py:157-158)")
    viz_colors = kwargs.get("viz_colors", None)
    if is_viz and not return_d_score and viz_colors is None:
        raise NotImplementedError("is_viz=True with viz_colors=None draws random colours from the global RNG (ut:249-265); "
                                  "pass viz_colors [K, 3] or [N, K, 3]")
    dev = _device(device)
    prm = torch.zeros(n, 8, dtype=torch.float64)
    prm[:, 0], prm[:, 1] = xs.cpu(), ys.cpu()
    prm[:, 2:6] = covs.reshape(n, 4).cpu()
    prm[:, 6] = sizes.cpu()
    from . import ops  # noqa: F401  (registers torch.ops.blobctrl.*)
    index = dev.index if dev.index is not None else 0
    if return_d_score and not only_splatting_bg and not only_splatting_fg:
        return torch.ops.blobctrl.splat_scores(prm, h, w, index)                       # ut:193-194, already channels-first
    scores, d_all = torch.ops.blobctrl.splat_maps(prm, h, w, index)                    # [N, H, W, M+1] each
    if only_splatting_bg:                                                              # ut:183-191
        d_scores = d_all[..., 0].unsqueeze(-1)
    elif only_splatting_fg:
        d_scores = d_all[..., 1:]
    else:
        d_scores = d_all
    if return_d_score:
        return d_scores.permute(0, 3, 1, 2)                                            # 'n h w m -> n m h w' view, ut:194
    ret = {}
    if is_viz:                                                                         # ut:198-214
        if viz_score_fn is not None:
            viz_posterior = viz_score_fn(scores)
            if not (isinstance(viz_posterior, torch.Tensor) and viz_posterior.shape == scores.shape):
                raise ValueError("viz_score_fn must map the raw scores [N, H, W, M+1] to a tensor of the same shape")
            scores_viz = torch.ops.blobctrl.alpha_composite(viz_posterior.to(torch.float64).contiguous())
        else:
            scores_viz = d_scores
        colors = torch.as_tensor(viz_colors).to(dev)                                   # ut:250-256
        if colors.ndim == 2:
            colors = colors[:n + 1][None].expand(scores_viz.shape[0], -1, -1)
        elif colors.ndim == 3:
            colors = colors[:, :n + 1]
        else:
            raise NotImplementedError("viz_colors must be [K, 3] or [N, K, 3] (other ranks draw random colours, ut:257-258)")
        ret["feature_img"] = splat_features_from_scores(scores_viz, colors, viz_size)
    if only_vis:
        return ret
    score_img = d_scores.permute(0, 3, 1, 2)                                           # ut:226
    ret["scores_pyramid"] = pyramid_resize(score_img, cutoff=interp_size)
    if features is None:
        raise TypeError("the dictionary return needs features [N, M+1, C] (ut:230-233)")
    feature_grid = splat_features_from_scores(ret["scores_pyramid"][interp_size], features, interp_size, channels_last=False)
    ret.update({"feature_grid": feature_grid, "feature_img": None, "entropy_img": None})
    if ret_layout:
        if torch.is_tensor(in_sizes) and in_sizes.ndim == 3:
            in_sizes = in_sizes.squeeze(-1)                                            # ut:165-166
        ret.update({"xs": in_xs, "ys": in_ys, "covs": in_covs, "raw_scores": scores, "sizes": in_sizes,
                    "composed_scores": d_scores, "features": features})
    return ret


def splat_features_from_scores(scores, features, size, channels_last=True):
    """ut:57-77 (= pipeline_blobnet.py:706-721) in ONE bc_splat_from_scores launch: scores [N, H, W, M] (or [N, M, H, W] when not
    channels_last) x features [N, M, C] -> [N, C, H', W'], with the bilinear resize to `size` (int: square; tuple) folded into the read.
    Like the reference, `size` resizes unless it equals scores.shape[2] (a falsy `size` never does)."""
    if not isinstance(scores, torch.Tensor) or scores.dtype not in (torch.float64, torch.float32):
        raise TypeError("splat_features_from_scores: scores must be a float64 or float32 tensor")
    if scores.ndim != 4:
        raise ValueError("splat_features_from_scores: scores must be [N, H, W, M] or [N, M, H, W]")
    _require_gpu(scores, "splat_features_from_scores")
    features = torch.as_tensor(features).to(dtype=scores.dtype, device=scores.device)          # ut:69
    H, W = (scores.shape[1], scores.shape[2]) if channels_last else (scores.shape[2], scores.shape[3])
    if size and not (scores.shape[2] == size):                                                 # ut:70
        out_h, out_w = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    else:
        out_h, out_w = H, W
    from . import ops  # noqa: F401
    return torch.ops.blobctrl.splat_from_scores(scores, features, out_h, out_w, bool(channels_last))


def pyramid_resize(img, cutoff):
    """ut:280-294: {last-dimension size: level}; every level below the first is the SQUARE bilinear resize to half the last dimension."""
    from . import ops  # noqa: F401
    out = [img]
    while img.shape[-1] > cutoff:
        half = img.shape[-1] // 2
        img = torch.ops.blobctrl.resize_bilinear(img, half, half)
        out.append(img)
    return {i.size(-1): i for i in out}


def _params_array(params: torch.Tensor):
    p = params.detach().to("cpu", torch.float64).contiguous()
    return (C.c_double * (8 * p.shape[0]))(*p.reshape(-1).tolist()), p.shape[0]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _splat_scores_impl(params: torch.Tensor, h: int, w: int, dev: torch.device) -> torch.Tensor:
    """Body of torch.ops.blobctrl.splat_scores: one bc_splat_scores launch (fp64) on `dev`."""
    lib = _lib.load()
    prm, n = _params_array(params)
    out = torch.empty(n, 2, h, w, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.bc_splat_scores(prm, n, h, w, out.data_ptr(), _stream()), "bc_splat_scores")
    return out


def _splat_maps_impl(params: torch.Tensor, h: int, w: int, dev: torch.device):
    """Body of torch.ops.blobctrl.splat_maps: one bc_splat_maps launch -> (raw, composed), each [n][h][w][2] fp64."""
    lib = _lib.load()
    prm, n = _params_array(params)
    raw = torch.empty(n, h, w, 2, dtype=torch.float64, device=dev)
    composed = torch.empty_like(raw)
    with torch.cuda.device(dev):
        _lib.check(lib.bc_splat_maps(prm, n, h, w, raw.data_ptr(), composed.data_ptr(), _stream()), "bc_splat_maps")
    return [raw, composed]


def _alpha_composite_impl(raw: torch.Tensor) -> torch.Tensor:
    _require_gpu(raw, "blobctrl::alpha_composite")
    if raw.dtype != torch.float64 or raw.ndim < 1:
        raise TypeError("blobctrl::alpha_composite: raw scores must be float64 [..., K]")
    lib = _lib.load()
    raw = raw.contiguous()
    out = torch.empty_like(raw)
    K = raw.shape[-1]
    with torch.cuda.device(raw.device):
        _lib.check(lib.bc_alpha_composite(raw.data_ptr(), raw.numel() // K, K, out.data_ptr(), _stream()), "bc_alpha_composite")
    return out


def _splat_from_scores_impl(scores: torch.Tensor, features: torch.Tensor, out_h: int, out_w: int, channels_last: bool) -> torch.Tensor:
    _require_gpu(scores, "blobctrl::splat_from_scores")
    if scores.dtype not in (torch.float64, torch.float32) or features.dtype != scores.dtype or features.device != scores.device:
        raise TypeError("blobctrl::splat_from_scores: scores and features must share float64 or float32 and the device")
    lib = _lib.load()
    sn, s1, s2, s3 = scores.stride()
    if channels_last:
        (N, H, W, M), (sy, sx, sm) = scores.shape, (s1, s2, s3)
    else:
        (N, M, H, W), (sm, sy, sx) = scores.shape, (s1, s2, s3)
    if features.ndim != 3 or features.shape[0] != N or features.shape[1] != M:
        raise ValueError(f"blobctrl::splat_from_scores: features must be [{N}, {M}, C], got {tuple(features.shape)}")
    features = features.contiguous()
    Cf = features.shape[2]
    out = torch.empty(N, Cf, out_h, out_w, dtype=scores.dtype, device=scores.device)
    with torch.cuda.device(scores.device):
        _lib.check(lib.bc_splat_from_scores(scores.data_ptr(), features.data_ptr(), N, M, Cf, H, W, sn, sm, sy, sx, out_h, out_w,
                                            int(scores.dtype == torch.float32), out.data_ptr(), _stream()), "bc_splat_from_scores")
    return out


def _resize_bilinear_impl(img: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    _require_gpu(img, "blobctrl::resize_bilinear")
    if img.dtype not in (torch.float64, torch.float32) or img.ndim != 4:
        raise TypeError("blobctrl::resize_bilinear: img must be a float64 or float32 [N, K, H, W] tensor")
    lib = _lib.load()
    img = img.contiguous()
    N, K, H, W = img.shape
    out = torch.empty(N, K, out_h, out_w, dtype=img.dtype, device=img.device)
    with torch.cuda.device(img.device):
        _lib.check(lib.bc_resize_bilinear(img.data_ptr(), N * K, H, W, out_h, out_w, int(img.dtype == torch.float32), out.data_ptr(),
                                          _stream()), "bc_resize_bilinear")
    return out


def _pack_rgb8_impl(img: torch.Tensor) -> torch.Tensor:
    _require_gpu(img, "blobctrl::pack_rgb8")
    if img.dtype != torch.float64 or img.ndim != 4 or img.shape[0] != 1 or img.shape[1] != 3:
        raise TypeError("blobctrl::pack_rgb8: img must be a float64 [1, 3, H, W] tensor")
    lib = _lib.load()
    img = img.contiguous()
    H, W = img.shape[2], img.shape[3]
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=img.device)
    with torch.cuda.device(img.device):
        _lib.check(lib.bc_pack_rgb8(img.data_ptr(), H, W, out.data_ptr(), _stream()), "bc_pack_rgb8")
    return out
