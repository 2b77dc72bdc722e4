#!/usr/bin/env python3
"""HIP-event times of "segment everything" at real ViT-H shape (synthetic weights: the arithmetic and the launches are those of the
released checkpoint), on a 1024 x 1024 image:
  * `set_image` (host preprocessing + encoder replay);
  * `SamAutomaticMaskGenerator.generate` split into decode (the batched decoder replays), resize (the two bilinear launches per batch),
    stats (bc_mask_stats and the filters around it) and host (everything else: copies to the host, NMS, dict building);
  * one `decode_batch(Bp)` replay per prompt beside the single-prompt `decode` replay, measured alternately in the same process;
  * bc_mask_stats alone on Bp x 3 masks of 1024 x 1024 against the bytes it has to read.
Synthetic weights predict IoUs and stabilities far below the package's thresholds, so the thresholds are opened (every mask reaches the stats
pass, none is dropped before the NMS): the generate figures are those of a scene in which every prompt yields masks.
Prints one JSON line.  --layers N runs a shallower encoder (default 32); --points-per-side and --batch size the generator."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps, warmup=2):
    """Median (and minimum) milliseconds of each callable, taking turns: a drift of the machine hits all of them alike."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            times[k].append(event_ms(fn))
    return [(float(np.median(t)), float(min(t))) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points-per-side", type=int, default=32)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    from blobctrl_amd import synth
    from blobctrl_amd.launch import run_graphed
    from blobctrl_amd.sam import SamAutomaticMaskGenerator, SamConfig, SamModel
    glob = (7, 15, 23, 31) if args.layers == 32 else tuple(range(3, args.layers, 4)) or (args.layers - 1,)
    sd = synth.synth_state_dict(synth.sam_param_shapes(layers=args.layers, global_attn_indexes=glob), 131)
    model = SamModel(sd, SamConfig(num_heads=16, window_size=14, global_attn_indexes=glob))
    Bp, S = args.batch, args.size
    gen = SamAutomaticMaskGenerator(model, points_per_side=args.points_per_side, points_per_batch=Bp, pred_iou_thresh=-1e9,
                                    stability_score_thresh=0.0, stability_score_offset=0.05, box_nms_thresh=0.7)
    rng = np.random.Generator(np.random.PCG64(5))
    image = rng.integers(0, 256, size=(S, S, 3), dtype=np.uint8)
    res = {"layers": args.layers, "image": [S, S], "points": args.points_per_side ** 2, "points_per_batch": Bp}
    gen.generate(image)                                               # planning + graph capture of the encoder and the decoder plan(s)
    plans = model.plans_recorded
    runs = []
    for _ in range(3):
        gen.generate(image)
        runs.append(dict(gen.last_timing))
    assert model.plans_recorded == plans
    for key in ("set_image_ms", "generate_ms", "decode_ms", "resize_ms", "stats_ms", "host_ms"):
        res[key] = round(float(np.median([r[key] for r in runs])), 3)
    res["masks_returned"] = runs[-1]["masks"]
    # the batched replay beside the single-prompt one, alternately
    g_ = model.grid
    pts = torch.from_numpy(rng.uniform(0, model.image_size, (Bp, 1, 2)).astype(np.float32)).cuda()
    labs = torch.ones(Bp, 1, dtype=torch.int32, device="cuda")
    model.decode_batch(pts, labs)
    model.decode(pts[0].cpu().numpy(), [1])
    PB, P1 = model._decoder_plan_batch(Bp, 1), model._decoder_plan(1)
    (b_med, b_min), (s_med, s_min) = alternate([lambda: run_graphed(PB.seg, model.device), lambda: run_graphed(P1.seg, model.device)], args.reps)
    res.update(decode_batch_ms=round(b_med, 4), decode_batch_min_ms=round(b_min, 4), decode_batch_ms_per_prompt=round(b_med / Bp, 5),
               decode_single_ms=round(s_med, 4), decode_single_min_ms=round(s_min, 4), per_prompt_ratio=round(b_med / Bp / s_med, 4),
               decode_batch_launches=len(PB.seg), decode_single_launches=len(P1.seg),
               decode_batch_buffer_mib=round(PB.rec.bytes_allocated / 2 ** 20, 1), decode_single_buffer_mib=round(P1.rec.bytes_allocated / 2 ** 20, 1))
    # the statistics pass alone: it reads every logit once
    logits = torch.randn(3 * Bp, S, S, device="cuda")
    (m_med, m_min), = alternate([lambda: model.mask_stats(logits, 0.0, 0.05)], args.reps)
    res.update(mask_stats_ms=round(m_med, 4), mask_stats_min_ms=round(m_min, 4), mask_stats_masks=3 * Bp,
               mask_stats_gb_per_s=round(logits.numel() * 4 / m_med * 1e-6, 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
