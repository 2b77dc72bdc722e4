#!/usr/bin/env python3
"""HIP-event times of the small-region removal (blobctrl_amd/masks.py, include/blobctrl_masks.h) on 64 and 16 masks of 1024 x 1024:
  * `clean_masks` (holes, then islands) as a whole, and every launch group of bc_mask_remove_small on its own (bc_mask_remove_small_phase:
    label, merge, flatten + areas, roots, apply) with the bytes it has to move;
  * the route a user has without it, on the same box and the same masks: `masks.cpu()` alone, and `masks.cpu()` plus the package's
    remove_small_regions with scipy.ndimage.label in cv2's place (if scipy is importable; the copy alone if not);
  * `SamAutomaticMaskGenerator.generate` with and without `min_mask_region_area` (synthetic ViT weights, thresholds opened as in
    tools/sam_amg_probe.py, NMS threshold 1.0 so that every mask is kept: synthetic masks all span the frame).
Inputs: thresholded smooth noise (a few large components plus specks, like a real mask) and 0.5-density noise (the worst case: ~10^5
components per mask).  Warm-up and medians as in tools/sam_amg_probe.py.  Prints one JSON line; --markdown FILE also writes the tables."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PHASES = ("label", "merge", "flatten+area", "roots", "apply")


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def smooth_masks(n, S, seed):
    """A coarse random field, upsampled, plus a little white noise, thresholded: blobs with ragged edges, pinholes and specks."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    coarse = torch.randn(n, 1, 24, 24, device="cuda", generator=g)
    field = torch.nn.functional.interpolate(coarse, size=(S, S), mode="bicubic", align_corners=False)[:, 0]
    return (field + 0.35 * torch.randn(n, S, S, device="cuda", generator=g)) > 0.3


def noise_masks(n, S, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(n, S, S, device="cuda", generator=g) < 0.5


def phase_bytes(S):
    """Bytes per mask each launch group has to move: label reads the mask and writes labels and counts; merge touches the pixels on tile
    borders (32 x 64 tiles) and their three neighbours; flatten reads labels and counts; roots reads the counts; apply reads the labels."""
    hw = S * S
    borders = (-(-S // 32) - 1) * S + (-(-S // 64) - 1) * S
    return {"label": 9 * hw, "merge": 16 * borders, "flatten+area": 8 * hw, "roots": 4 * hw, "apply": 4 * hw}


def device_times(src, min_area, reps):
    from blobctrl_amd import _lib, masks
    lib = _lib.load()
    n, S, _ = src.shape
    step = masks._group(n, S, S)
    work = src.view(torch.uint8).clone()
    scratch = torch.empty(2, min(step, n), S, S, dtype=torch.int32, device="cuda")
    out = torch.empty(n, 6, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    per = {(mode, p): [] for mode in (0, 1) for p in range(len(PHASES))}
    whole = []
    for rep in range(reps + 2):
        work.copy_(src.view(torch.uint8))
        for lo in range(0, n, step):
            k = min(step, n - lo)
            for mode in (0, 1):
                for p in range(len(PHASES)):
                    t = event_ms(lambda: _lib.check(lib.bc_mask_remove_small_phase(work[lo].data_ptr(), k, S, S, min_area, mode, scratch[0].data_ptr(),
                                                                                   scratch[1].data_ptr(), out[lo].data_ptr(), p, stream), "phase"))
                    if rep >= 2:
                        per[mode, p].append(t)
        t = event_ms(lambda: masks.clean_masks(src, min_area))
        if rep >= 2:
            whole.append(t)
    groups = -(-n // step)
    cleaned, changed, stats = masks.clean_masks(src, min_area)
    assert torch.equal(cleaned, work.bool()), "the phases one by one and clean_masks disagree"
    table = {}
    for mode, mname in ((0, "holes"), (1, "islands")):
        for p, pname in enumerate(PHASES):
            table[f"{mname}/{pname}"] = float(np.median(np.array(per[mode, p]).reshape(-1, groups).sum(1))) if groups > 1 else float(np.median(per[mode, p]))
    return table, float(np.median(whole)), cleaned, int(changed.sum()), int((cleaned != src).sum())


def host_route(src, min_area):
    """masks.cpu(), then the package's remove_small_regions with scipy's labelling where the package calls cv2."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = src.cpu().numpy()
    t1 = time.perf_counter()
    try:
        from scipy import ndimage
    except ImportError:
        return 1e3 * (t1 - t0), None, None
    eight = np.ones((3, 3))
    res = np.empty_like(host)
    for k, m in enumerate(host):
        for holes in (True, False):
            working = holes ^ m
            lab, count = ndimage.label(working, structure=eight)
            sizes = np.bincount(lab.ravel(), minlength=count + 1)[1:]
            small = np.flatnonzero(sizes < min_area) + 1
            if len(small) == 0:
                continue
            if holes:
                m = ~working | np.isin(lab, small)
            else:
                keep = np.setdiff1d(np.arange(1, count + 1), small)
                if len(keep) == 0:
                    keep = [int(np.argmax(sizes)) + 1]
                m = np.isin(lab, keep)
        res[k] = m
    return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--min-area", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--layers", type=int, default=32, help="encoder depth of the generate() measurement (0: skip it)")
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    S, res, lines = args.size, {"size": args.size, "min_area": args.min_area}, []
    bytes_of = phase_bytes(S)
    for kind, make in (("smooth", smooth_masks), ("noise50", noise_masks)):
        for n in (64, 16):
            src = make(n, S, 7)
            table, whole, cleaned, changed, flipped = device_times(src, args.min_area, args.reps)
            copy_ms, host_ms, host_res = host_route(src, args.min_area)
            if host_res is not None:
                assert np.array_equal(host_res, cleaned.cpu().numpy()), "the host route and the device pass disagree"
            key = f"{kind}/{n}"
            res[key] = {"clean_masks_ms": round(whole, 4), "phases_ms": {k: round(v, 4) for k, v in table.items()}, "masks_changed": changed,
                        "pixels_flipped": flipped, "host_copy_ms": round(copy_ms, 3), "host_label_ms": None if host_ms is None else round(host_ms, 1)}
            lines.append(f"\n### {kind}, {n} masks of {S} x {S}, min_area {args.min_area}: {changed} masks changed, {flipped} pixels flipped\n")
            lines.append("| launch group | holes us/mask | GB/s | islands us/mask | GB/s |\n|---|---|---|---|---|")
            for p in PHASES:
                h, i = table[f"holes/{p}"], table[f"islands/{p}"]
                lines.append(f"| {p} | {1e3 * h / n:.2f} | {bytes_of[p] * n / h * 1e-6:.0f} | {1e3 * i / n:.2f} | {bytes_of[p] * n / i * 1e-6:.0f} |")
            total = sum(table.values())
            lines.append(f"| sum of the groups | {1e3 * sum(table[f'holes/{p}'] for p in PHASES) / n:.2f} | | {1e3 * sum(table[f'islands/{p}'] for p in PHASES) / n:.2f} | |")
            host_txt = "scipy not importable: not measured" if host_ms is None else f"{host_ms:.1f} ms ({host_ms / n:.2f} ms / mask)"
            lines.append(f"\n`clean_masks` (both modes, allocation included): {whole:.3f} ms = {1e3 * whole / n:.1f} us / mask; sum of the launch groups "
                         f"{total:.3f} ms.  Host route: `masks.cpu()` {copy_ms:.2f} ms; plus scipy labelling and removal {host_txt}.  Device pass "
                         f"{'<' if whole < copy_ms else '>='} the copy alone.")
    if args.layers > 0:
        from blobctrl_amd import synth
        from blobctrl_amd.sam import SamAutomaticMaskGenerator, SamConfig, SamModel
        glob = (7, 15, 23, 31) if args.layers == 32 else tuple(range(3, args.layers, 4)) or (args.layers - 1,)
        sd = synth.synth_state_dict(synth.sam_param_shapes(layers=args.layers, global_attn_indexes=glob), 131)
        model = SamModel(sd, SamConfig(num_heads=16, window_size=14, global_attn_indexes=glob))
        gen = SamAutomaticMaskGenerator(model, points_per_side=8, points_per_batch=64, pred_iou_thresh=-1e9, stability_score_thresh=0.0,
                                        stability_score_offset=0.05, box_nms_thresh=1.0, crop_nms_thresh=1.0)
        image = np.random.Generator(np.random.PCG64(5)).integers(0, 256, size=(S, S, 3), dtype=np.uint8)
        gen.generate(image)
        runs = {0: [], args.min_area: []}
        for _ in range(3):
            for m in runs:
                got = gen.generate(image, min_mask_region_area=m)
                runs[m].append(dict(gen.last_timing, returned=len(got)))
        med = lambda m, key: round(float(np.median([r[key] for r in runs[m]])), 3)
        res["generate"] = {str(m): {key: med(m, key) for key in ("generate_ms", "set_image_ms", "decode_ms", "resize_ms", "stats_ms", "regions_ms",
                                                                 "host_ms", "returned")} for m in runs}
        lines.append(f"\n### generate on a {S} x {S} image, {args.layers}-layer encoder, 8 x 8 points, every mask kept\n")
        lines.append("| min_mask_region_area | generate ms | set_image | decode | resize | stats | regions | host | masks |\n|---|---|---|---|---|---|---|---|---|")
        for m in runs:
            r = res["generate"][str(m)]
            lines.append(f"| {m} | {r['generate_ms']} | {r['set_image_ms']} | {r['decode_ms']} | {r['resize_ms']} | {r['stats_ms']} | {r['regions_ms']} | "
                         f"{r['host_ms']} | {int(r['returned'])} |")
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
