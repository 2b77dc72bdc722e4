#!/usr/bin/env python3
"""What the front half of an edit costs on the device (blobctrl_amd/edit_inputs.py, include/blobctrl_edit.h) and on the host path it stands
beside (blobctrl_amd/blob_edit.py), at 512 x 512 and 1024 x 1024, for one request and for a batch of 8:
  * HIP-event time of each new launch - bc_ellipse_cover, bc_ellipse_paint (k = 2), bc_mask_row_extents, bc_mask_cutout - as the median over
    windows of INNER back-to-back launches, with GB/s against the bytes the launch has to touch (computed here from the shapes and the masks);
  * wall time of the whole device front half, from the device masks to the pipeline's three inputs and the DINOv2 pixel values: extents +
    their copy + the host ellipse fits, cut-out, paint, splat, `vae_input` twice, the foreground copy and the PIL preprocessing for DINOv2;
  * wall time of the unchanged host path from the same device masks on the same box in the same run: `masks.cpu()`, `ellipse_from_mask`,
    `object_region_from_mask`, `build_edit_inputs`, `VaeImageProcessor.preprocess` twice + upload, `Dinov2ImageProcessor.preprocess`.
The two paths alternate, every wall time ends in a device synchronise, and their outputs are compared once (they must be equal).  Every
request is a "move": its own object mask (a filled ellipse, about 7 % of the frame), start ellipse = the fit, target = the fit shifted.
Prints one JSON line; --markdown FILE also writes the tables."""
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


def object_ellipses(n, S):
    """n objects of a frame S x S: ellipses of about 7 % of its area, each somewhere else and turned differently"""
    s = S / 512.0
    return [((s * (180.0 + 23.7 * i), s * (300.0 - 17.3 * i)), (s * (120.0 + 5.1 * i), s * (190.0 - 7.3 * i)), 20.0 + 19.9 * i) for i in range(n)]


def shifted(e, S):
    return ((e[0][0] + 0.11 * S, e[0][1] - 0.07 * S), e[1], e[2])


def launches(n, S, reps):
    """name -> (median ms of one launch, bytes it has to touch)"""
    from blobctrl_amd import _lib, edit_inputs
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    ells = object_ellipses(n, S)
    prm = torch.tensor([edit_inputs.ellipse_params(e) for e in ells], dtype=torch.float64).cuda()
    prm2 = torch.tensor([[edit_inputs.ellipse_params(e), edit_inputs.ellipse_params(shifted(e, S))] for e in ells], dtype=torch.float64).cuda()
    rgb = torch.tensor([[edit_inputs.WHITE, edit_inputs.BLACK]] * n, dtype=torch.uint8).cuda()
    masks = torch.empty(n, S, S, dtype=torch.uint8, device="cuda")
    images = torch.randint(0, 256, (n, S, S, 3), dtype=torch.uint8, device="cuda")
    ext = torch.empty(n, S, 2, dtype=torch.int32, device="cuda")
    cut = torch.empty(n, S, S, 3, dtype=torch.uint8, device="cuda")
    calls = {
        "bc_ellipse_cover": lambda: lib.bc_ellipse_cover(prm.data_ptr(), n, S, S, masks.data_ptr(), stream),
        "bc_ellipse_paint (k = 2)": lambda: lib.bc_ellipse_paint(images.data_ptr(), n, S, S, prm2.data_ptr(), rgb.data_ptr(), 2, stream),
        "bc_mask_row_extents": lambda: lib.bc_mask_row_extents(masks.data_ptr(), n, S, S, ext.data_ptr(), stream),
    }
    _lib.check(calls["bc_ellipse_cover"](), "bc_ellipse_cover")
    _, boxes = edit_inputs.ellipses_from_masks(masks)
    bt = torch.tensor(boxes, dtype=torch.int32).cuda()
    calls["bc_mask_cutout"] = lambda: lib.bc_mask_cutout(images[0].data_ptr(), masks.data_ptr(), bt.data_ptr(), n, S, S, cut.data_ptr(), stream)
    set_px = int((masks != 0).sum())
    painted = int((edit_inputs.ellipse_masks([shifted(e, S) for e in ells], S, S) | masks).ne(0).sum())
    box_px = int(sum(b[2] * b[3] for b in boxes))
    touched = {"bc_ellipse_cover": n * S * S + 48 * n, "bc_ellipse_paint (k = 2)": 3 * painted + 102 * n,
               "bc_mask_row_extents": n * S * S + 8 * n * S, "bc_mask_cutout": 3 * n * S * S + box_px + 3 * set_px + 16 * n}
    out = {}
    for name, fn in calls.items():
        _lib.check(fn(), name)
        times = [event_ms(fn) for _ in range(reps + 2)][2:]
        out[name] = (float(np.median(times)), touched[name])
    return out


def device_front_half(image, masks, dino_proc):
    from blobctrl_amd import edit_inputs
    n, S = masks.shape[0], masks.shape[1]
    ellipses, boxes = edit_inputs.ellipses_from_masks(masks)
    fg = edit_inputs.object_regions(image, masks, boxes)
    bg, score, strengths = edit_inputs.build_edit_inputs_batch(["move"] * n, image, ellipses, [shifted(e, S) for e in ellipses], [1.0] * n)
    fg_in, bg_in = edit_inputs.vae_input(fg), edit_inputs.vae_input(bg)
    px = dino_proc.preprocess(images=list(fg.cpu().numpy()))["pixel_values"].cuda()
    return dict(ellipses=ellipses, fg=fg, bg=bg, score=score, strengths=strengths, fg_in=fg_in, bg_in=bg_in, dino=px)


def host_front_half(image, masks, dino_proc, vae_proc):
    from PIL import Image
    from blobctrl_amd import blob_edit
    img, host_masks = image.cpu().numpy(), masks.cpu().numpy()
    S = img.shape[0]
    out = dict(ellipses=[], fg=[], bg=[], score=[], strengths=[], fg_in=[], bg_in=[], dino=[])
    for m in host_masks:
        e = blob_edit.ellipse_from_mask(m)
        fg = blob_edit.object_region_from_mask(m, img)
        bg, score, strength = blob_edit.build_edit_inputs("move", img, e, shifted(e, S), 1.0)
        out["ellipses"].append(e)
        out["fg"].append(fg)
        out["bg"].append(bg)
        out["score"].append(score)
        out["strengths"].append(strength)
        out["fg_in"].append(vae_proc.preprocess(Image.fromarray(fg)).cuda())
        out["bg_in"].append(vae_proc.preprocess(Image.fromarray(bg)).cuda())
        out["dino"].append(dino_proc.preprocess(images=fg)["pixel_values"].cuda())
    return out


def same(dev, host):
    ok = dev["ellipses"] == host["ellipses"] and dev["strengths"] == host["strengths"]
    ok = ok and np.array_equal(dev["fg"].cpu().numpy(), np.stack(host["fg"])) and np.array_equal(dev["bg"].cpu().numpy(), np.stack(host["bg"]))
    for k in ("score", "fg_in", "bg_in", "dino"):
        ok = ok and torch.equal(dev[k], torch.cat(host[k], 0))
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=10, help="timed windows of INNER launches per entry point")
    ap.add_argument("--wall-reps", type=int, default=3, help="alternations of the device and the host front half")
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edit_inputs_probe measures on the GPU; there is none here")
    from blobctrl_amd import edit_inputs
    from blobctrl_amd.image_processor import Dinov2ImageProcessor, VaeImageProcessor
    dino_proc, vae_proc = Dinov2ImageProcessor(), VaeImageProcessor()
    res, launch_lines, wall_lines = {}, [], []
    launch_lines.append("| frame | requests | launch | us | GB touched | GB/s |\n|---|---|---|---|---|---|")
    wall_lines.append("| frame | requests | device front half ms | host path ms | host / device | same outputs |\n|---|---|---|---|---|---|")
    for S in args.sizes:
        image = torch.randint(0, 256, (S, S, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(S))
        for n in args.batches:
            key = f"{S}/{n}"
            res[key] = {"launches_us": {}}
            for name, (ms, nbytes) in launches(n, S, args.reps).items():
                res[key]["launches_us"][name] = round(1e3 * ms, 2)
                launch_lines.append(f"| {S} x {S} | {n} | {name} | {1e3 * ms:.1f} | {nbytes * 1e-9:.4f} | {nbytes / ms * 1e-6:.0f} |")
            masks = edit_inputs.ellipse_masks(object_ellipses(n, S), S, S) != 0
            device_front_half(image, masks, dino_proc)                     # warm-up: code objects, the splat, allocator
            dev_ms, host_ms = [], []
            for _ in range(args.wall_reps):
                t, dev = wall_ms(lambda: device_front_half(image, masks, dino_proc))
                dev_ms.append(t)
                t, host = wall_ms(lambda: host_front_half(image, masks, dino_proc, vae_proc))
                host_ms.append(t)
            d, h, ok = float(np.median(dev_ms)), float(np.median(host_ms)), same(dev, host)
            res[key].update(device_ms=round(d, 2), host_ms=round(h, 2), device_all_ms=[round(v, 2) for v in dev_ms],
                            host_all_ms=[round(v, 2) for v in host_ms], ratio=round(h / d, 2), same_outputs=ok, set_pixels=int(masks[0].sum()))
            wall_lines.append(f"| {S} x {S} | {n} | {d:.1f} ({min(dev_ms):.1f} - {max(dev_ms):.1f}) | {h:.1f} ({min(host_ms):.1f} - {max(host_ms):.1f}) | "
                              f"{h / d:.1f} | {'yes' if ok else 'NO'} |")
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write("# The front half of an edit: device path beside the host path (tools/edit_inputs_probe.py)\n\n"
                    f"Medians; launches over {args.reps} windows of {INNER} back-to-back launches (HIP events), wall times over {args.wall_reps} "
                    "alternations of the two paths (min - max in brackets), each ending in a device synchronise.\n\n## Launches\n\n")
            f.write("\n".join(launch_lines) + "\n\n## Front half, from the device masks to the pipeline's inputs\n\n" + "\n".join(wall_lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
