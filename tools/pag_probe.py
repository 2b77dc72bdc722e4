"""What perturbed-attention guidance (PAG) costs on an MI355X.

1. ms per active denoise step of the flagship 512^2 edit (bench.py's synthetic weights and inputs, DDIM, whole-edit graph) at batch 1
   and 2, in three settings - without PAG, with "mid", with all 16 self-attention layers - alternating edits in one process, and the
   launches per active step of each plan.  A PAG plan runs the UNet at 3/2 of the batch ([uncond | cond | perturbed]); BlobNet stays.
2. bc_attention_identity (csrc/pag.hip) alone at the four UNet levels of that edit, one perturbed image: HIP-event time and achieved GB/s
   (algorithmic bytes: V^T read once, the output rows written once), beside the bc_attention launch of one image it stands for.

    python tools/pag_probe.py [--markdown profiles/pag.md] [--reps 20] [--steps 20] [--edits 4] [--bench-lines FILE]

`--bench-lines FILE`: lines to append under "bench.py headline" (the interleaved A/B of tools/ab_prev.sh, run beside this probe).
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

LEVELS = ((320, 64 * 128), (640, 32 * 64), (1280, 16 * 32), (1280, 8 * 16))      # (channels, tokens per image)
HEADS = 8


def measure_identity(dev, Cc, HW, reps):
    """(identity us, GB/s, bc_attention us for one image) at one level: B = 3 buffers, the last image perturbed."""
    rec = Recorder(dev)
    try:
        B, d = 3, Cc // HEADS
        ldvt = (HW + 63) // 64 * 64
        qk = torch.randn(B * HW, 2 * Cc, device=dev).half()
        vt = torch.randn(B, Cc, ldvt, device=dev).half()
        a = torch.empty(B * HW, Cc, device=dev, dtype=torch.float16)
        seg = rec.begin("probe")
        for _ in range(reps):
            rec.attention_identity(vt, a, B, B - 1, HW, Cc, ldvt, Cc)
            rec.attention(qk, qk, vt, a, 1, HEADS, d, HW, HW, 2 * Cc, 2 * Cc, ldvt, Cc, HW * 2 * Cc, HW * 2 * Cc, Cc * ldvt, HW * Cc, d ** -0.5,
                          q_off=0, k_off=Cc)
        s = torch.cuda.current_stream().cuda_stream
        seg.run(s)
        torch.cuda.synchronize()
        timed = seg.run_timed(s)
        ident = statistics.median(ms for m, ms in timed if m["kind"] == "attention_identity")
        att = statistics.median(ms for m, ms in timed if m["kind"] == "attention")
        nbytes = next(m["bytes"] for m, _ in timed if m["kind"] == "attention_identity")
        assert torch.equal(a[(B - 1) * HW:], vt[B - 1, :, :HW].t())
        return ident * 1e3, nbytes / (ident * 1e-3) / 1e9, att * 1e3
    finally:
        rec.close()


def step_times(dev, steps, edits, batches=(1, 2)):
    """{(batch, setting): [ms per step of every timed edit]}, {(batch, setting): launches per active step}."""
    import bench
    from blobctrl_amd import pag
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.splat import splat_features
    from blobctrl_amd.weights import PackedTrunk
    ucfg, bcfg = bench.full_configs()
    usd, bsd = bench.synth_weights()
    eng = BlobCtrlEngine(PackedTrunk(usd, dev, ucfg.block_out_channels), PackedTrunk(bsd, dev, bcfg.block_out_channels), ucfg, bcfg,
                         device=str(dev), scheduler="ddim", max_cached_plans=3)
    del usd, bsd
    h = w = 64
    layers = {"none": (), "mid": pag.resolve_layers(ucfg, "mid"), "all16": pag.resolve_layers(ucfg, ["down", "mid", "up"])}
    assert len(layers["all16"]) == 16
    times, launches = {}, {}
    for B in batches:
        inp = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in bench.synth_inputs(h, w, batch=B).items()}
        score = splat_features(**inp["blob"], score_size=(h, w), return_d_score=True, device=str(dev))

        def edit(name):
            extra = dict(pag_scale=3.0, pag_applied_layers=layers[name]) if name != "none" else {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng(inp["prompt"], inp["fg"], inp["bg"], score, inp["dino"], num_inference_steps=steps, guidance_scale=7.5, latents=inp["latents"], **extra)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / steps
        for n in tuple(layers) * 2:                                        # record, capture, warm (three plans of this batch stay cached)
            edit(n)
        for n in layers:
            times[(B, n)] = []
        for _ in range(edits):
            for n in layers:
                times[(B, n)].append(edit(n))
        for n in layers:
            launches[(B, n)] = len(eng.plan_for(B, h, w, 77, 768, steps, pag=layers[n]).step_active)
    return times, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--edits", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--bench-lines")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs an MI355X"
    dev = torch.device("cuda:0")
    med = statistics.median
    lines = ["# Perturbed-attention guidance on an MI355X (tools/pag_probe.py)", ""]
    if not args.no_step:
        times, launches = step_times(dev, args.steps, args.edits)
        lines += [f"## Step time, 512^2 edit, DDIM, {args.steps} steps, whole-edit graph, the three settings alternating in one process", "",
                  "ms per step = the whole edit (prologue included) over its steps.", "",
                  "| batch | setting | UNet batch | ms per step (median) | every edit | vs no PAG | launches per active step |", "|---|---|---|---|---|---|---|"]
        for (B, n), t in times.items():
            base = med(times[(B, "none")])
            label = {"none": "no PAG", "mid": 'PAG "mid" (1 layer)', "all16": "PAG, all 16 layers"}[n]
            lines.append(f"| {B} | {label} | {(2 if n == 'none' else 3) * B} | {med(t):.3f} | {' '.join(f'{v:.3f}' for v in t)} | {med(t) / base:.3f} x | "
                         f"{launches[(B, n)]} |")
        lines += ["", "The UNet of a PAG plan runs 3/2 of the images and no CFG-prefix sharing; BlobNet runs what it ran.  The expectation before this",
                  "measurement was a UNet part that grows by about 3/2; the table is what was measured."]
    lines += ["", "## bc_attention_identity alone, one perturbed image per level (B = 3 buffers, b0 = 2)", "",
              "| C | tokens | identity us | GB/s | bc_attention of one image us |", "|---|---|---|---|---|"]
    for Cc, HW in LEVELS:
        us, gbs, att = measure_identity(dev, Cc, HW, args.reps)
        lines.append(f"| {Cc} | {HW} | {us:.1f} | {gbs:.0f} | {att:.1f} |")
    lines += ["", "Bytes: V^T read once and the output rows written once, 2 x 2 x HW x C.  The launch replaces the attention of the perturbed image;",
              "whether folding it into the bc_attention launch would pay is the difference between a few microseconds of a launch on the UNet's",
              "queue and nothing: not pursued here."]
    if args.bench_lines and os.path.exists(args.bench_lines):
        lines += ["", "## bench.py headline, this commit beside its parent on the same box (tools/ab_prev.sh, interleaved)", ""]
        lines += open(args.bench_lines).read().rstrip().splitlines()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
