"""What a masked edit (the latent blend, include/blobctrl_blend.h) costs on an MI355X.

1. bc_blend_scheduler_step beside the step entry point it replaces (bc_cfg_scheduler_step) at 64^2 and 96^2 latents, batch 1 and 8,
   alternating in one process: HIP-event time per launch.  The blend reads three more operands per element (image, noise, a quarter of
   a mask) and writes nothing more.
2. bc_blend_mask at 512^2 and 768^2, one launch per edit.
3. ms per step of the flagship 512^2 edit (bench.py's synthetic weights and inputs, DDIM, whole-edit graph) with and without the blend,
   alternating edits in one process.

    python tools/latent_blend_probe.py [--markdown profiles/latent_blend.md] [--reps 20] [--steps 20] [--edits 4] [--no-step]

Every stand-alone launch is replayed `reps` times in one segment behind a warm-up replay; the figure is the median of the per-launch
event times.  Needs a GPU."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blobctrl_amd.launch import Recorder  # noqa: E402


def measure_steps(dev, B, h, reps, nsteps=4):
    """(plain step us, blend step us) at [B][4][h][h]."""
    rec = Recorder(dev)
    try:
        f = lambda *s: torch.randn(*s, device=dev)
        eps, lat, hist, out = f(2 * B, h, 2 * h, 4), f(B, 4, h, h), f(3, B * 4 * h * h), f(B, 4, h, h)
        coef, idx = torch.rand(nsteps, 16, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
        image, noise, mask, table = f(B, 4, h, h), f(B, 4, h, h), torch.rand(B, h, h, device=dev), torch.rand(nsteps, 2, device=dev)
        seg = rec.begin("probe")
        rec.keep.append((eps, lat, hist, out, coef, idx, image, noise, mask, table))
        for _ in range(reps):
            rec.call("bc_cfg_scheduler_step", eps, lat, coef, idx, hist, -1.0, B, h, h, out, 0, kind="plain")
            rec.call("bc_blend_scheduler_step", eps, lat, coef, idx, hist, None, image, noise, mask, table, B, h, h, None, nsteps, 0, 0, out, 0,
                     kind="blend")
        s = torch.cuda.current_stream().cuda_stream
        seg.run(s)
        torch.cuda.synchronize()
        timed = seg.run_timed(s)
        med = lambda kind: statistics.median(ms for m, ms in timed if m["kind"] == kind) * 1e3
        return med("plain"), med("blend")
    finally:
        rec.close()


def measure_mask(dev, n, H, reps):
    rec = Recorder(dev)
    try:
        mask = torch.randint(0, 256, (n, H, H), dtype=torch.uint8, device=dev)
        out = torch.empty(n, H // 8, H // 8, device=dev)
        seg = rec.begin("probe")
        rec.keep.append((mask, out))
        for _ in range(reps):
            rec.call("bc_blend_mask", mask, out, n, H, H, kind="blend_mask")
        s = torch.cuda.current_stream().cuda_stream
        seg.run(s)
        torch.cuda.synchronize()
        assert torch.equal(out, (mask[:, ::8, ::8] >= 128).float())
        return statistics.median(ms for _, ms in seg.run_timed(s)) * 1e3
    finally:
        rec.close()


def step_times(dev, steps, edits):
    """{setting: [ms per step of every timed edit]} of the 512^2 edit at batch 1."""
    import bench
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.splat import splat_features
    from blobctrl_amd.weights import PackedTrunk
    ucfg, bcfg = bench.full_configs()
    usd, bsd = bench.synth_weights()
    eng = BlobCtrlEngine(PackedTrunk(usd, dev, ucfg.block_out_channels), PackedTrunk(bsd, dev, bcfg.block_out_channels), ucfg, bcfg,
                         device=str(dev), scheduler="ddim", max_cached_plans=2)
    del usd, bsd
    h = w = 64
    inp = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in bench.synth_inputs(h, w, batch=1).items()}
    score = splat_features(**inp["blob"], score_size=(h, w), return_d_score=True, device=str(dev))
    mask = (torch.rand(1, 8 * h, 8 * w, device=dev) > 0.5).to(torch.uint8) * 255
    extra = {"plain": {}, "blend": dict(blend_image_latents=inp["bg"], blend_mask=mask)}

    def edit(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng(inp["prompt"], inp["fg"], inp["bg"], score, inp["dino"], num_inference_steps=steps, guidance_scale=7.5, latents=inp["latents"],
            **extra[name])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    for n in tuple(extra) * 2:                                             # record, capture, warm
        edit(n)
    times = {n: [] for n in extra}
    for _ in range(edits):
        for n in extra:
            times[n].append(edit(n))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--edits", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs an MI355X"
    dev = torch.device("cuda:0")
    med = statistics.median
    lines = ["# The latent blend of a masked edit on an MI355X (tools/latent_blend_probe.py)", "",
             "## The step launch alone, alternating with the entry point it replaces", "",
             "| latent | batch | bc_cfg_scheduler_step us | bc_blend_scheduler_step us |", "|---|---|---|---|"]
    for h in (64, 96):
        for B in (1, 8):
            plain, blend = measure_steps(dev, B, h, args.reps)
            lines.append(f"| {h} x {h} | {B} | {plain:.1f} | {blend:.1f} |")
    lines += ["", "## bc_blend_mask, one launch per edit", "", "| mask | us |", "|---|---|"]
    for n, H in ((1, 512), (8, 512), (1, 768)):
        lines.append(f"| [{n}][{H}][{H}] | {measure_mask(dev, n, H, args.reps):.1f} |")
    if not args.no_step:
        times = step_times(dev, args.steps, args.edits)
        lines += ["", f"## Step time, 512^2 edit, batch 1, DDIM, {args.steps} steps, whole-edit graph, alternating in one process", "",
                  "ms per step = the whole edit (prologue and the per-edit fills included) over its steps.", "",
                  "| setting | ms per step (median) | every edit |", "|---|---|---|"]
        for n, t in times.items():
            lines.append(f"| {n} | {med(t):.3f} | {' '.join(f'{v:.3f}' for v in t)} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
