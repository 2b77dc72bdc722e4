#!/usr/bin/env python3
"""Time the AutoencoderTiny preview path on an MI355X and write profiles/tiny_vae.md (--markdown PATH).

For latents 64 x 64 and 96 x 96 at batch 1 and 8 (--sizes / --batches), in ONE process with the routes alternating:
  * `AutoencoderTiny.preview` and `.decode` (csrc/tiny_vae.hip; one graph of 1 + 35 launches),
  * `AutoencoderKL.decode` of this project on the same latents,
  * a plain-torch fp16 channels_last route written out here from the same state dict (F.conv2d / F.relu / F.interpolate(mode="nearest")):
    the vendor library's time for the same arithmetic,
each as the median of `--reps` windows of `--calls` calls between two device events, after a warm-up of every shape.  Then the launch list
alone, one event pair per launch (bc_plan_run_timed, median over passes), summed per stage and form with GFLOP/s and GB/s from the algorithmic
FLOPs and bytes of the shapes; the compiler's resource report of csrc/tiny_vae.hip; and (unless --no-edit) a 50-step 512 x 512 edit on
synthetic SD-1.5 weights with an empty step-end callback, with a preview every 5 steps and with one every step.
A run without a GPU fails: nothing here falls back."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from blobctrl_amd import synth                       # noqa: E402
from blobctrl_amd.tiny_vae import AutoencoderTiny, decoder_layers    # noqa: E402

HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fPIC"]


def resource_report():
    """[(kernel, VGPRs, AGPRs, scratch bytes / lane, occupancy, dynamic LDS bytes)] from -Rpass-analysis=kernel-resource-usage (no GPU needed).
    The LDS of tiny_conv3x3_kernel is dynamic: computed as csrc/tiny_vae.hip lays it out."""
    src = os.path.join(REPO, "blobctrl_amd", "csrc", "tiny_vae.hip")
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + HIPCC_FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                            os.path.join(d, "t.o")], capture_output=True, text=True)
    if p.returncode:
        return []
    rows, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = dict(name=m.group(1))
            rows.append(cur)
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    out = []
    for r in rows:
        m = re.search(r"tiny_conv3x3_kernelILi(\d+)ELi(\d+)E", r["name"])
        if m:
            ci, mt = int(m.group(1)), int(m.group(2))
            lds = (mt * 32 * (9 * ci + 8) + 340 * (ci + 8)) * 2 + 256
            out.append((f"tiny_conv3x3_kernel<{ci},{mt}>", r.get("vgpr"), r.get("agpr"), r.get("scratch"), r.get("occ"), lds))
        elif "tiny_latents_in" in r["name"]:
            out.append(("tiny_latents_in_kernel", r.get("vgpr"), r.get("agpr"), r.get("scratch"), r.get("occ"), 0))
    return out


def median_ms(fn, calls, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / calls)
    return statistics.median(ts), min(ts), max(ts)


class TorchRoute:
    """The decoder in plain torch, fp16 channels_last, from the same state dict."""

    def __init__(self, sd, device):
        cl = lambda t: t.to(device, torch.float16).contiguous(memory_format=torch.channels_last)
        self.layers = [(L["form"], cl(sd[L["name"] + ".weight"]),
                        sd[L["name"] + ".bias"].to(device, torch.float16) if L["name"] + ".bias" in sd else None) for L in decoder_layers()]

    @torch.no_grad()
    def __call__(self, z):
        x = (torch.tanh(z / 3) * 3).half().contiguous(memory_format=torch.channels_last)
        skip = None
        for form, w, b in self.layers:
            if form == "up":
                x = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, None, padding=1)
                continue
            y = F.conv2d(x, w, b, padding=1)
            if form == "out":
                return ((y.float() * 2 - 1) / 2 + 0.5).clamp(0, 1).mul(255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
            if form == "a":
                skip = x
            x = F.relu(y + skip) if form == "c" else F.relu(y)


def launch_table(tiny, B, h, w, passes=7):
    """Per (stage, form): launches, median-summed ms, GFLOP/s, GB/s - the preview segment replayed launch by launch."""
    P = tiny._plan(B, h, w)
    s = torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in range(passes + 1):
        runs.append([ms for _, ms in P.preview.run_timed(s)])
        torch.cuda.synchronize()
    runs = runs[1:]
    med = [statistics.median(r[i] for r in runs) for i in range(len(P.preview.meta))]
    agg = {}
    for m, ms in zip(P.preview.meta, med):
        sh = m["shape"]
        key = (sh[0], f"{sh[2]}x{sh[3]}")
        e = agg.setdefault(key, [0, 0.0, 0, 0])
        e[0] += 1
        e[1] += ms
        e[2] += m["flops"]
        e[3] += m["bytes"]
    return [(k[0], k[1], e[0], e[1], e[2] / (e[1] * 1e-3) / 1e9 if e[1] else 0.0, e[3] / (e[1] * 1e-3) / 1e9 if e[1] else 0.0) for k, e in agg.items()], sum(med)


def edit_times(tiny_sd, steps=50, res=512, edits=3):
    """ms of a `steps`-step edit at res x res on synthetic SD-1.5 weights: empty callback / preview every 5 steps / every step (median of
    `edits` edits each, alternating, after one warm-up edit of each kind)."""
    import bench
    from blobctrl_amd.pipeline import BlobCtrlEngine
    from blobctrl_amd.splat import splat_features
    ucfg, bcfg = bench.full_configs()
    usd, bsd = bench.synth_weights()
    pipe = BlobCtrlEngine(usd, bsd, ucfg, bcfg, scheduler="unipc")
    pipe.load_preview_vae(tiny_sd)
    h = w = res // 8
    inp = bench.synth_inputs(h, w)
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}
    score = splat_features(**inp["blob"], score_size=(h, w), return_d_score=True, device="cuda:0")
    kept = []

    def cb_every(n):
        def cb(p, i, t, d):
            if n and i % n == 0:
                kept.append(p.preview(d["latents"], "uint8"))
            return {}
        return cb

    def edit(n):
        del kept[:]
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pipe(dev["prompt"], dev["fg"], dev["bg"], score, dev["dino"], num_inference_steps=steps, guidance_scale=7.5, latents=dev["latents"],
             callback_on_step_end=cb_every(n))
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    kinds = (("empty callback", 0), ("preview every 5 steps", 5), ("preview every step", 1))
    for _, n in kinds:
        edit(n)
    times = {k: [] for k, _ in kinds}
    for _ in range(edits):
        for k, n in kinds:
            times[k].append(edit(n))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", default=None, help="write the report there (e.g. profiles/tiny_vae.md)")
    ap.add_argument("--sizes", default="64,96")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-edit", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiny_vae_probe: no GPU - a time is measured on the MI355X or not at all")
    from blobctrl_amd.vae import AutoencoderKL
    sd = synth.synth_state_dict(synth.tiny_vae_param_shapes(), 33)
    tiny = AutoencoderTiny(sd)
    route = TorchRoute(sd, "cuda:0")
    kl = AutoencoderKL(synth.synth_state_dict(synth.vae_param_shapes(), 33))
    out = [f"# AutoencoderTiny preview on {torch.cuda.get_device_name(0)}", "",
           "Written by `tools/tiny_vae_probe.py`.  Times are medians (min .. max) of "
           f"{args.reps} windows of {args.calls} calls between two device events, the routes alternating in one process after a warm-up of every "
           "shape; weights are synthetic (`synth`, seed 33).  `preview` and `decode` are one graph replay of 1 + 35 launches each.", ""]
    res = resource_report()
    out += ["## Compiler resource report (csrc/tiny_vae.hip, gfx950)", "", "| kernel | VGPRs | AGPRs | scratch B/lane | waves/SIMD | LDS bytes (dynamic) |",
            "|---|---|---|---|---|---|"] + [f"| `{r[0]}` | {r[1]} | {r[2]} | {r[3]} | {r[4]} | {r[5]} |" for r in res] + [""]
    out += ["## Calls", "", "| latents | batch | tiny preview ms | tiny decode ms | AutoencoderKL.decode ms | KL / preview | torch fp16 channels_last ms | torch / preview |",
            "|---|---|---|---|---|---|---|---|"]
    tables, checks = [], []
    for hw in (int(v) for v in args.sizes.split(",")):
        for B in (int(v) for v in args.batches.split(",")):
            z = torch.randn(B, 4, hw, hw, generator=torch.Generator().manual_seed(hw + B)).cuda() * 2
            fns = {"preview": lambda: tiny.preview(z), "decode": lambda: tiny.decode(z), "torch": lambda: route(z), "kl": lambda: kl.decode(z)}
            ok = {}
            for k, fn in fns.items():                     # warm-up: plans, graphs, the vendor library's algorithm search
                try:
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    ok[k] = fn
                except torch.cuda.OutOfMemoryError:
                    torch.cuda.empty_cache()
            same = torch.equal(tiny.preview(z), ((tiny.decode(z).sample / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1))
            diff = (tiny.preview(z).int() - route(z).int()).abs()
            t = {k: median_ms(fn, args.calls if k != "kl" else max(3, args.calls // 4), args.reps) for k, fn in ok.items()}
            f = lambda k: f"{t[k][0]:.3f} ({t[k][1]:.3f} .. {t[k][2]:.3f})" if k in t else "not measured (out of memory)"
            ratio = lambda k: f"{t[k][0] / t['preview'][0]:.2f}" if k in t else "-"
            out.append(f"| {hw} x {hw} | {B} | {f('preview')} | {f('decode')} | {f('kl')} | {ratio('kl')} | {f('torch')} | {ratio('torch')} |")
            checks.append(f"- {hw} x {hw}, batch {B}: `preview` equals the quantised `decode`: {same}; bytes against the torch route (fp16 bias, skip and "
                          f"ReLU arithmetic there): largest difference {int(diff.max())} levels, {100 * float((diff > 0).float().mean()):.1f} % of the bytes differ")
            print(out[-1], checks[-1], flush=True)
            tables.append((hw, B, launch_table(tiny, B, hw, hw)))
            kl._plans.clear()                             # (a full-size KL plan holds gigabytes of activations: one shape at a time)
            torch.cuda.empty_cache()
    out += ["", "Results of the same run, compared:", ""] + checks
    out += ["", "## The launch list, launch by launch (`bc_plan_run_timed`: an event pair per launch, serial; GFLOP/s and GB/s from the shapes)", ""]
    for hw, B, (rows, total) in tables:
        out += [f"### latents {hw} x {hw}, batch {B}: {total:.3f} ms over 36 launches", "", "| form | output | launches | ms | GFLOP/s | GB/s |", "|---|---|---|---|---|---|"]
        out += [f"| {r[0]} | {r[1]} | {r[2]} | {r[3]:.4f} | {r[4]:.0f} | {r[5]:.0f} |" for r in rows] + [""]
    if not args.no_edit:
        et = edit_times(sd)
        base = et["empty callback"][0]
        out += ["## A 50-step 512 x 512 edit with previews from `callback_on_step_end` (synthetic SD-1.5 weights, eager loop: a callback is set)", "",
                "| callback | ms per edit, median (min .. max) of 3 | over the empty callback |", "|---|---|---|"]
        out += [f"| {k} | {v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f}) | {v[0] - base:+.1f} ms |" for k, v in et.items()] + [""]
    text = "\n".join(out) + "\n"
    print(text)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
