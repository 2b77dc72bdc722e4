#!/usr/bin/env python3
"""What Pillow's resize costs on the device (blobctrl_amd/resample.py, include/blobctrl_resample.h) and on the host route it stands beside,
for the three resizes of an edit:
    512 x 512 -> 256 x 256 bicubic            DINOv2's input (then the 224 x 224 centre crop and the normalisation)
    1024 x 768 -> 512 x 512 lanczos           a VAE input of another size
    1365 x 2048 -> 683 x 1024 bilinear        SAM's input (long side 1024, then the normalisation and the padding)
  * HIP-event time of each launch - bc_resample_horizontal, bc_resample_vertical (uint8 epilogue) - for the whole resized frame, as the
    median over windows of INNER back-to-back launches, with GB/s against the source bytes it reads plus the output bytes it writes
    (computed here from the shapes and the tables);
  * wall time of the device route of each consumer (`dinov2_pixel_values`, `resize_images`, `sam_pixel_values`) from a device image to a
    device result, and of the host route for the same pixels in the same run: the copy down, Pillow (through the host processor the device
    route stands for), the copy up.  The two alternate, every wall time ends in a device synchronise, and their results are compared once
    (they must be equal).
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
CASES = [("DINOv2", 512, 512, 256, 256, "bicubic"), ("VAE", 1024, 768, 512, 512, "lanczos"), ("SAM", 1365, 2048, 683, 1024, "bilinear")]


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


def launches(image, oh, ow, name, reps):
    """launch -> (median ms, bytes read + written) for the whole resized frame of one image [H][W][3]"""
    from blobctrl_amd import _lib, resample
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    H, W, _ = image.shape
    dev = str(image.device)
    r0, rows = resample.source_rows(H, oh, name, 0, oh)
    bx, cx, kx = resample._device_tables(W, ow, name, dev)
    by, cy, ky = resample._device_tables(H, oh, name, dev)
    tmp = torch.empty(rows, ow, 3, dtype=torch.uint8, device=image.device)
    out = torch.empty(oh, ow, 3, dtype=torch.uint8, device=image.device)
    calls = {
        "bc_resample_horizontal": (lambda: lib.bc_resample_horizontal(image.data_ptr(), 1, H, W, r0, rows, bx.data_ptr(), cx.data_ptr(), kx, ow,
                                                                      0, ow, tmp.data_ptr(), stream), 3 * rows * (W + ow)),
        "bc_resample_vertical": (lambda: lib.bc_resample_vertical(tmp.data_ptr(), 1, rows, ow, r0, 0, by.data_ptr(), cy.data_ptr(), ky, oh, 0, oh,
                                                                  ow, out.data_ptr(), None, None, 0, 0, stream), 3 * ow * (rows + oh)),
    }
    res = {}
    for launch, (fn, nbytes) in calls.items():
        _lib.check(fn(), launch)
        times = [event_ms(fn) for _ in range(reps + 2)][2:]
        res[launch] = (float(np.median(times)), nbytes, kx if launch.endswith("horizontal") else ky)
    assert torch.equal(out, resample.resize_images(image, (oh, ow), name))
    return res


def routes(tag, image, oh, ow, name):
    """(device route, host route) of the consumer `tag`: device image in, device tensor out"""
    from PIL import Image
    from blobctrl_amd import resample, sam
    from blobctrl_amd.image_processor import Dinov2ImageProcessor
    flt = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]
    if tag == "DINOv2":
        proc = Dinov2ImageProcessor(shortest_edge=min(oh, ow), crop_size=224)
        return (lambda: resample.dinov2_pixel_values(image, proc),
                lambda: proc.preprocess(images=image.cpu().numpy())["pixel_values"].to(image.device))
    if tag == "SAM":
        return (lambda: resample.sam_pixel_values(image, max(oh, ow))[1],
                lambda: sam.preprocess_image(image.cpu().numpy(), max(oh, ow))[1].to(image.device))
    return (lambda: resample.resize_images(image, (oh, ow), name),
            lambda: torch.from_numpy(np.array(Image.fromarray(image.cpu().numpy()).resize((ow, oh), flt))).to(image.device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="timed windows of INNER launches per entry point")
    ap.add_argument("--wall-reps", type=int, default=7, help="alternations of the device and the host route")
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_resample_probe measures on the GPU; there is none here")
    res = {}
    launch_lines = ["| resize | filter | launch | taps | us | MB read + written | GB/s |\n|---|---|---|---|---|---|---|"]
    wall_lines = ["| consumer | resize | device route ms | host route ms | host / device | same result |\n|---|---|---|---|---|---|"]
    for tag, H, W, oh, ow, name in CASES:
        image = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(H))
        key, what = f"{tag}/{H}x{W}->{oh}x{ow}/{name}", f"{H} x {W} -> {oh} x {ow}"
        res[key] = {"launches_us": {}}
        for launch, (ms, nbytes, taps) in launches(image, oh, ow, name, args.reps).items():
            res[key]["launches_us"][launch] = round(1e3 * ms, 2)
            launch_lines.append(f"| {what} | {name} | {launch} | {taps} | {1e3 * ms:.1f} | {nbytes * 1e-6:.2f} | {nbytes / ms * 1e-6:.0f} |")
        device, host = routes(tag, image, oh, ow, name)
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
        wall_lines.append(f"| {tag} | {what} {name} | {dm:.2f} ({min(dev_ms):.2f} - {max(dev_ms):.2f}) | {hm:.2f} ({min(host_ms):.2f} - "
                          f"{max(host_ms):.2f}) | {hm / dm:.1f} | {'yes' if ok else 'NO'} |")
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write("# Pillow's resize on the device beside the host route (tools/image_resample_probe.py)\n\n"
                    f"Medians; launches over {args.reps} windows of {INNER} back-to-back launches (HIP events) on one image, for the whole resized "
                    f"frame; wall times over {args.wall_reps} alternations of the two routes (min - max in brackets), device image in, device "
                    "tensor out, each ending in a device synchronise.  The host route is the copy down, the host processor (Pillow), the copy "
                    "up.  No gate: these are the numbers as measured.\n\n## Launches\n\n")
            f.write("\n".join(launch_lines) + "\n\n## Routes\n\n" + "\n".join(wall_lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
