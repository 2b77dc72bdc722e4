#!/usr/bin/env python3
"""HIP-event time of `blob_edit.blob_overlay` (the app's blob image, scripts/blobctrl_app.py:611-650) at 512 x 512: median of N calls
after warm-up, with the copy of the uint8 image to the host and without it, beside the reference's CPU time recorded in
tests/golden/blob_viz.npz.  Usage: python tools/blob_overlay_probe.py [N=50]"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    from blobctrl_amd import ops  # noqa: F401
    from blobctrl_amd.blob_edit import blob_overlay
    from blobctrl_amd.splat import blob_dict_from_ellipse, splat_features
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    z = np.load(os.path.join(REPO, "tests", "golden", "blob_viz.npz"))
    meta = json.loads(str(z["meta"]))["full"]
    colors = torch.from_numpy(z["viz_colors"]).to("cuda:0")
    ell, H, W = meta["ellipse"], meta["H"], meta["W"]

    def device_only():
        img = splat_features(**blob_dict_from_ellipse(ell, W, H), interp_size=64, viz_size=(H, W), is_viz=True, score_size=64,
                             viz_score_fn=lambda s: s, viz_colors=colors, only_vis=True)["feature_img"]
        return torch.ops.blobctrl.pack_rgb8(img)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(np.min(ms))

    with_copy = timed(lambda: blob_overlay(ell, H, W, colors))
    without = timed(device_only)
    print(json.dumps({"blob_overlay_512_ms_median": with_copy[0], "blob_overlay_512_ms_min": with_copy[1],
                      "device_only_ms_median": without[0], "device_only_ms_min": without[1], "calls": n,
                      "reference_cpu_ms": meta["reference_cpu_ms_median_of_5"], "reference_threads": meta["threads"]}))


if __name__ == "__main__":
    main()
