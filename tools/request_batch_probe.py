#!/usr/bin/env python3
"""(GPU) What the per-request form of a request batch costs: 512^2, batch 8, DDIM, 50 steps, synthetic weights and the mixed-operation
request batch of bench.py (BASELINE configs[2]), three variants of the same eight requests, alternating A, B, C, A, B, C, ... in one
process:

    A  the scalar request batch: one step count, guidance scale and window for the batch - today's plan
    B  the list form with eight equal values: the `requests` plan (bc_scheduler_step_requests, bc_timestep_embedding_rows)
    C  steps [50, 50, 40, 40, 30, 30, 20, 20] with eight different guidance scales and windows

Every variant is warmed up (plan recorded, whole-edit graph captured) before the first timed edit; an edit is timed on the host clock
around a device synchronise.  Reported: ms per edit and ms per step of the 50-step loop (median, minimum and maximum of the repeats) and
B's and C's latents against A's.  There is no pass / fail number: B differs from A in three elementwise launches per step and the
prologue's two embedding launches, C runs the same launches on other tables.  `--per-launch` adds the per-launch table
(bc_plan_run_timed, serial replay) of the launches in which A's and B's active step differ.

    python tools/request_batch_probe.py [--repeats 5] [--steps 50] [--batch 8] [--res 512] [--per-launch] [--json OUT]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402


def variants(B, steps):
    """name -> the keyword arguments that differ between the variants."""
    down = [max(1, steps - (steps // 5) * (b // 2)) for b in range(B)]          # 50, 50, 40, 40, 30, 30, 20, 20 at B = 8, steps = 50
    return {"A": dict(num_inference_steps=steps, guidance_scale=7.5, blobnet_control_guidance_start=0.0, blobnet_control_guidance_end=0.9),
            "B": dict(num_inference_steps=[steps] * B, guidance_scale=[7.5] * B, blobnet_control_guidance_start=[0.0] * B,
                      blobnet_control_guidance_end=[0.9] * B),
            "C": dict(num_inference_steps=down, guidance_scale=[3.0 + 0.75 * b for b in range(B)],
                      blobnet_control_guidance_start=[0.02 * b for b in range(B)], blobnet_control_guidance_end=[1.0 - 0.05 * b for b in range(B)])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--per-launch", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("request_batch_probe: needs an MI355X (no GPU found); nothing is measured without one")
    from blobctrl_amd.pipeline import BlobCtrlEngine
    dev = torch.device("cuda:0")
    ucfg, bcfg = bench.full_configs()
    usd, bsd = bench.synth_weights()
    eng = BlobCtrlEngine(usd, bsd, ucfg, bcfg, device=str(dev), scheduler="ddim")
    B, h = args.batch, args.res // 8
    rb = bench.make_request_batch(list(range(B)), h, h, dev)
    kws = variants(B, args.steps)

    def edit(name):
        return eng.denoise(rb["prompt"], rb["fg"], rb["bg"], rb["score"], rb["dino"], latents=rb["latents"],
                           blobnet_conditioning_scale=rb["strength"], **kws[name])
    out = {}
    for name in kws:                                                            # warm-up: record, capture, one replay
        edit(name)
        out[name] = edit(name)
        torch.cuda.synchronize()
    times = {name: [] for name in kws}
    for _ in range(args.repeats):
        for name in kws:                                                        # alternating: the variants share whatever else the box does
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            edit(name)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    res = dict(batch=B, res=args.res, steps=args.steps, repeats=args.repeats, cache_stats=dict(eng.cache_stats), variants={})
    for name, ts in times.items():
        res["variants"][name] = dict(ms_per_edit_median=round(statistics.median(ts), 3), ms_per_edit_min=round(min(ts), 3),
                                     ms_per_edit_max=round(max(ts), 3), ms_per_step_median=round(statistics.median(ts) / args.steps, 4),
                                     ms_per_step_min=round(min(ts) / args.steps, 4), ms_per_step_max=round(max(ts) / args.steps, 4))
        print(f"{name}: ms per edit median {statistics.median(ts):9.3f}  [{min(ts):9.3f} .. {max(ts):9.3f}]   ms per step "
              f"{statistics.median(ts) / args.steps:7.4f}  [{min(ts) / args.steps:7.4f} .. {max(ts) / args.steps:7.4f}]  ({len(ts)} edits)")
    a = out["A"].double()
    res["B_equals_A_bitwise"] = bool(torch.equal(out["A"], out["B"]))
    res["C_vs_A_max_abs_over_scale"] = float((out["C"].double() - a).abs().max() / a.abs().max())
    print(f"B == A bit for bit: {res['B_equals_A_bitwise']};  C vs A (other values: expected to differ) max-abs / scale "
          f"{res['C_vs_A_max_abs_over_scale']:.3e}")
    if args.per_launch:
        keys = list(eng._plans)
        pa = next(eng._plans[k] for k in keys if "requests" not in k)
        pb = next(eng._plans[k] for k in keys if "requests" in k)
        s = eng.stream.cuda_stream
        rows = []
        for seg in ("prologue", "step_active"):
            with torch.cuda.stream(eng.stream):                                 # (a replay reads the tables' row of the step counter)
                pa.step_idx.zero_()
                pb.step_idx.zero_()
            eng.stream.synchronize()
            ta, tb = getattr(pa, seg).run_timed(s), getattr(pb, seg).run_timed(s)
            assert len(ta) == len(tb), (seg, len(ta), len(tb))
            for (ma, msa), (mb, msb) in zip(ta, tb):
                if ma["kind"] in ("temb", "assemble", "cfg_step") and ma["shape"] is None:
                    rows.append(dict(segment=seg, kind=ma["kind"], A_us=round(msa * 1e3, 2), B_us=round(msb * 1e3, 2)))
                    print(f"{seg:12s} {ma['kind']:10s} A {msa * 1e3:8.2f} us   B {msb * 1e3:8.2f} us")
        res["per_launch"] = rows
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
