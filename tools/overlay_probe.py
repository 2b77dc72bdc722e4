#!/usr/bin/env python3
"""What the finishing step of a zoomed edit costs on the device (blobctrl_amd/overlay.py, include/blobctrl_overlay.h) and on the host route
it stands beside, at 512 x 512, 2048 x 2048 and 3000 x 4000 (rows x columns):
  * HIP-event time of each launch - bc_box_blur3_rows, bc_box_blur3_cols (blur factors 4 and 32), bc_mask_bounds (both its launches),
    bc_overlay_composite (no crop: the patch is the frame) - as the median over windows of INNER back-to-back launches, with GB/s against
    the bytes it must read plus the bytes it writes (halo reads, which the caches mostly serve, are not counted);
  * wall time of the device route (`blur`, `crop_region`, `apply_overlay` with a crop) from device tensors to a device result, and of the
    host route for the same pixels in the same run: the copies down, Pillow (the PIL branch of VaeImageProcessor, which is Pillow's own
    calls), the copy up.  The two alternate, every wall time ends in a device synchronise, and their results are compared once (they must be equal).
Nothing is gated: the numbers are written down.  Prints one JSON line; --markdown FILE also writes the tables."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
INNER = 20
FRAMES = [(512, 512), (2048, 2048), (3000, 4000)]
FACTORS = (4, 32)


def event_ms(fn, inner=INNER):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def inputs(H, W):
    """(image, mask with a filled ellipse of a sixth of the frame, a "result" image) on the device"""
    from blobctrl_amd import edit_inputs
    g = torch.Generator(device="cuda").manual_seed(H)
    image = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    result = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    mask = edit_inputs.ellipse_masks([((0.55 * W, 0.45 * H), (W / 3, H / 4), 30.0)], H, W)[0]
    return image, mask, result


def launches(image, mask, result, reps):
    from blobctrl_amd import _lib, overlay
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    H, W = mask.shape
    tmp, out = torch.empty_like(mask), torch.empty_like(mask)
    ext = torch.empty(H, 2, dtype=torch.int32, device="cuda")
    box = torch.empty(4, dtype=torch.int32, device="cuda")
    comp = torch.empty_like(image)
    calls = {}
    for f in FACTORS:
        R, ww, fw = overlay.blur_params(f)
        calls[f"bc_box_blur3_rows (factor {f}, R = {R})"] = (
            lambda R=R, ww=ww, fw=fw: lib.bc_box_blur3_rows(mask.data_ptr(), 1, H, W, R, ww, fw, tmp.data_ptr(), stream), 2 * H * W)
        calls[f"bc_box_blur3_cols (factor {f}, R = {R})"] = (
            lambda R=R, ww=ww, fw=fw: lib.bc_box_blur3_cols(tmp.data_ptr(), 1, H, W, R, ww, fw, out.data_ptr(), stream), 2 * H * W)
    calls["bc_mask_bounds"] = (lambda: lib.bc_mask_bounds(mask.data_ptr(), 1, H, W, ext.data_ptr(), box.data_ptr(), stream), H * W + 16 * H + 16)
    calls["bc_overlay_composite"] = (lambda: lib.bc_overlay_composite(image.data_ptr(), mask.data_ptr(), result.data_ptr(), 1, H, W, H, W, 0, 0,
                                                                      comp.data_ptr(), stream), 10 * H * W)
    res = {}
    for launch, (fn, nbytes) in calls.items():
        _lib.check(fn(), launch)
        times = [event_ms(fn) for _ in range(reps + 2)][2:]
        res[launch] = (float(np.median(times)), nbytes)
    return res


def routes(image, mask, result, factor):
    from PIL import Image
    from blobctrl_amd import overlay
    from blobctrl_amd.image_processor import VaeImageProcessor
    proc = VaeImageProcessor()
    H, W = mask.shape

    def device():
        crop = overlay.crop_region(mask, W, H, 32)
        return overlay.apply_overlay(overlay.blur(mask, factor), image, result, crop)

    def host():
        m, init, res = Image.fromarray(mask.cpu().numpy()), Image.fromarray(image.cpu().numpy()), Image.fromarray(result.cpu().numpy())
        crop = proc.get_crop_region(m, W, H, 32)
        return torch.from_numpy(np.array(proc.apply_overlay(proc.blur(m, factor), init, res, crop))).to(image.device)

    return device, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="timed windows of INNER launches per entry point")
    ap.add_argument("--wall-reps", type=int, default=5, help="alternations of the device and the host route")
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("overlay_probe measures on the GPU; there is none here")
    res = {}
    launch_lines = ["| frame | launch | us | MB read + written | GB/s |\n|---|---|---|---|---|"]
    wall_lines = ["| frame | route | device ms | host ms | host / device | same result |\n|---|---|---|---|---|---|"]
    for H, W in FRAMES:
        image, mask, result = inputs(H, W)
        key = f"{H}x{W}"
        res[key] = {"launches_us": {}}
        for launch, (ms, nbytes) in launches(image, mask, result, args.reps).items():
            res[key]["launches_us"][launch] = round(1e3 * ms, 2)
            launch_lines.append(f"| {H} x {W} | {launch} | {1e3 * ms:.1f} | {nbytes * 1e-6:.2f} | {nbytes / ms * 1e-6:.0f} |")
        device, host = routes(image, mask, result, 4)
        device(), host()                                                   # warm-up: code objects, tables, allocator
        dev_ms, host_ms = [], []
        for _ in range(args.wall_reps):
            t, d = wall_ms(device)
            dev_ms.append(t)
            t, h = wall_ms(host)
            host_ms.append(t)
        dm, hm, ok = float(np.median(dev_ms)), float(np.median(host_ms)), bool(torch.equal(d, h))
        res[key].update(device_ms=round(dm, 3), host_ms=round(hm, 3), device_all_ms=[round(v, 3) for v in dev_ms],
                        host_all_ms=[round(v, 3) for v in host_ms], ratio=round(hm / dm, 2), same_result=ok)
        wall_lines.append(f"| {H} x {W} | crop region + blur 4 + apply_overlay with the crop | {dm:.2f} ({min(dev_ms):.2f} - {max(dev_ms):.2f}) | "
                          f"{hm:.2f} ({min(host_ms):.2f} - {max(host_ms):.2f}) | {hm / dm:.1f} | {'yes' if ok else 'NO'} |")
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write("# The finishing step of a zoomed edit on the device beside the host route (tools/overlay_probe.py)\n\n"
                    f"Medians; launches over {args.reps} windows of {INNER} back-to-back launches (HIP events) on one frame; wall times over "
                    f"{args.wall_reps} alternations of the two routes (min - max in brackets), device tensors in, device tensor out, each ending in "
                    "a device synchronise.  The host route is the copies down, Pillow, the copy up.  Bytes are those a launch must read and "
                    "write once (the blur's halo re-reads are not counted).  No gate: these are the numbers as measured.\n\n## Launches\n\n")
            f.write("\n".join(launch_lines) + "\n\n## Routes\n\n" + "\n".join(wall_lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
